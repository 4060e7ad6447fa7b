"""The streaming global attention of the ViT encoder (csrc/fw_gattn.hip gattn_stream_fwd_kernel, and the backward body with a
run-time tile count): every N = 64 nt from 128 to 1024 except 256, plain softmax + Dropout, no `lamb`.

  1  fw_gattn_fwd / fw_gattn_bwd against an f64 statement of encoder_ViT.py:76-96 on the dtype-rounded operands with the SAME Dropout
     masks (oracle/dropout_hash.py): `out` and `dqkv` through GlobalAttnFn, `lse` through the library call.  N = 128 is the first
     rescale, 192 an odd tile count, 576 / 1024 the sizes of 384x384 / 512x512 inputs.
  2  the limits can fail: the same reference with the last key tile left out (and renormalised) is rejected by the `out` limit.
  3  rescaling in both directions: K rows scaled per tile so that the row maximum moves by more than 100 between the first and the
     last tile (exp(100) overflows f32: rescaling l without O, or neither, gives inf, NaN or a wrong row).
  4  order independence: permuting the keys across tiles leaves `out` where it was.
  5  layout: qkv rows wider than 3 * heads * 64 with NaN pads, sentinel rows behind out / lse / dqkv.
  6  domain: `lamb` at these N, N = 96 and N = 1088 are argument errors; Transformer.run refuses a band re-weighting there.

Limits (helpers.close, relative to the maximum) are those of test_vit256_gpu.py::test_gattn_kernel: fp32 2e-5 on out, 1e-4 on dqkv;
bf16 1.5e-2 / 3e-2; lse 2e-5 in both (the reference sees the rounded operands, scores and sums are f32)."""
import functools

import pytest
import torch

import dropout_hash as DH
from helpers import close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HEADS, SEED, SITE = 2, 777, 41
LIMITS = {'fp32': (2e-5, 1e-4), 'bf16': (1.5e-2, 3e-2)}
LSE_LIMIT = 2e-5
TORCH_DT = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def set_dtype(name):
    from fwair import functional as Fn
    Fn.config.compute_dtype = TORCH_DT[name]
    Fn.config.direct_grads = False
    return Fn.config.compute_dtype


def batch_of(N):
    return 1 if N >= 1024 else 2


def ref_attention(qkv, B, N, heads, drop=None, keys=None):
    """encoder_ViT.py:76-96 in f64 on the CPU -> (out [B*N, heads*64], lse [B, heads, N]).  keys: attend to the first `keys` keys
    only (softmax renormalised over them)."""
    x = qkv.double().reshape(B, N, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    dots = (q @ k.transpose(-1, -2)) * 64 ** -0.5
    if keys is not None:
        dots, v = dots[..., :keys], v[:, :, :keys]
    attn = dots.softmax(-1)
    if drop is not None:
        seed, site, p = drop
        mask = torch.from_numpy(DH.keep_mask(seed, site, (B, heads, N, N), p)).double()
        attn = attn * mask[..., :attn.shape[-1]] / (1.0 - p)
    return (attn @ v).transpose(1, 2).reshape(B * N, heads * 64), torch.logsumexp(dots, -1)


def inputs(N, p, dtype, B):
    g = torch.Generator().manual_seed(N + int(p * 100))
    qkv = (torch.randn(B * N, 3 * HEADS * 64, generator=g) * 0.8).to(dtype)
    dout = (torch.randn(B * N, HEADS * 64, generator=g) * 0.5).to(dtype)
    return qkv, dout


@functools.lru_cache(maxsize=None)
def problem(N, p, dt):
    """operands, and the f64 reference (out, lse, dqkv, out without the last key tile) computed once"""
    B, dtype = batch_of(N), TORCH_DT[dt]
    qkv, dout = inputs(N, p, dtype, B)
    drop = (SEED, SITE, p) if p > 0 else None
    qr = qkv.float().clone().requires_grad_(True)
    ref, lse = ref_attention(qr, B, N, HEADS, drop)
    (ref * dout.double()).sum().backward()
    short, _ = ref_attention(qkv.float(), B, N, HEADS, drop, keys=N - 64)
    return B, qkv, dout, ref.detach(), lse.detach(), qr.grad, short


def lib_forward(qkv, B, N, p, lamb=None, nb=0):
    """fw_gattn_fwd on a [B*N, >= 3*heads*64] buffer -> (out, lse)"""
    from fwair.lib import call, dt
    inner = HEADS * 64
    out = torch.empty((B * N, inner), dtype=qkv.dtype, device=DEV)
    lse = torch.empty((B, HEADS, N), dtype=torch.float32, device=DEV)
    seed = torch.tensor([SEED], dtype=torch.int32, device=DEV)
    call('fw_gattn_fwd', dt(qkv.dtype), qkv, qkv[:, inner:], qkv[:, 2 * inner:], qkv.stride(0), out, out.stride(0), lse, B, HEADS, N,
         64 ** -0.5, seed if p > 0 else None, SITE, float(p), lamb, nb, 1, None, None)
    torch.cuda.synchronize()
    return out, lse


def run_fn(qkv, dout, B, N, p):
    """GlobalAttnFn forward + backward -> (out, dqkv)"""
    from fwair import functional as Fn
    from fwair import vit as V
    Fn.set_dropout_seed(SEED, DEV, frozen=True)
    try:
        qk = qkv.to(DEV).requires_grad_(True)
        out = V.GlobalAttnFn.apply(qk, None, (B, N, HEADS, p, SITE, None))
        out.backward(dout.to(DEV))
        torch.cuda.synchronize()
    finally:
        Fn.set_dropout_seed(1, DEV, frozen=False)
    return out.detach(), qk.grad


# ------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('N', [128, 192, 576, 1024])
def test_stream_kernel_vs_f64(dt, N, p):
    dtype = set_dtype(dt)
    B, qkv, dout, ref, lse_ref, dqkv_ref, short = problem(N, p, dt)
    t1, t2 = LIMITS[dt]
    out, dqkv = run_fn(qkv, dout, B, N, p)
    out2, lse = lib_forward(qkv.to(DEV), B, N, p)
    scale = lambda t: float(t.abs().max())
    errs = (float((out.double().cpu() - ref).abs().max()) / scale(ref), float((dqkv.double().cpu() - dqkv_ref).abs().max()) / scale(dqkv_ref),
            float((lse.double().cpu() - lse_ref).abs().max()) / scale(lse_ref), float((short - ref).abs().max()) / scale(ref))
    print(f'stream N {N} p {p} {dt}: out {errs[0]:.3e} (limit {t1:.1e})  dqkv {errs[1]:.3e} (limit {t2:.1e})  lse {errs[2]:.3e} '
          f'(limit {LSE_LIMIT:.1e})  out of the reference without the last key tile {errs[3]:.3e}')
    close(out.float(), ref, t1, 'out')
    assert torch.equal(out, out2), 'GlobalAttnFn and the library call disagree on out'
    close(dqkv.float(), dqkv_ref, t2, 'dqkv')
    close(lse, lse_ref, LSE_LIMIT, 'lse')
    # the limit tells this output from an attention that misses its last 64 keys
    with pytest.raises(AssertionError):
        close(short, ref, t1, 'out without the last key tile')
    with pytest.raises(AssertionError):
        close(out.float(), short, t1, 'kernel against the reference without the last key tile')
    assert dtype == out.dtype


# ------------------------------------------------------------------------------------------------ 3
def ramped(N, dt, rising):
    """inputs of (1) with the K rows of tile t scaled by 2^e(t), e from 0 to 8 (or 8 to 0) over the tiles.  Q and K are first rounded
    to multiples of 1/8: every product is then a multiple of 2^-6 and every partial sum of a score stays below 2^14, so an f32
    accumulator holds the scores exactly in any order of summation and the test sees the rescaling alone.  With unrounded operands
    the scores reach several hundred, their f32 rounding (a few ulp of 2^12 before the 1/8 scale) moves rows whose two largest scores
    nearly tie, and ANY f32 evaluation -- a tile loop in torch on the CPU included -- is 2e-5 .. 4e-5 away from the f64 `out`, at
    or above the fp32 limit, which says nothing about the rescaling."""
    B, dtype, nt = batch_of(N), TORCH_DT[dt], N // 64
    qkv, dout = inputs(N, 0.0, torch.float32, B)
    qkv[:, :2 * HEADS * 64] = (qkv[:, :2 * HEADS * 64] * 8).round() / 8
    e = torch.round(torch.arange(nt, dtype=torch.float64) * 8 / (nt - 1))
    if not rising:
        e = e.flip(0)
    f = (2.0 ** e).float().repeat_interleave(64).repeat(B)[:, None]
    inner = HEADS * 64
    qkv[:, inner:2 * inner] *= f
    return B, qkv.to(dtype), dout.to(dtype)


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('rising', [True, False], ids=['rising', 'falling'])
@pytest.mark.parametrize('N', [192, 576])
def test_stream_rescaling(dt, N, rising):
    set_dtype(dt)
    B, qkv, dout = ramped(N, dt, rising)
    qr = qkv.float().clone().requires_grad_(True)
    ref, lse_ref = ref_attention(qr, B, N, HEADS)
    (ref * dout.double()).sum().backward()
    assert torch.isfinite(ref).all() and torch.isfinite(lse_ref).all() and torch.isfinite(qr.grad).all()
    x = qkv.double().reshape(B, N, 3, HEADS, 64)
    dots = (x[:, :, 0].transpose(1, 2) @ x[:, :, 1].transpose(1, 2).transpose(-1, -2)) * 64 ** -0.5
    first, last = dots[..., :64].amax(-1), dots[..., -64:].amax(-1)
    gap = (last - first) if rising else (first - last)
    assert float(gap.min()) > 100, f'row maximum moves by only {float(gap.min()):.1f} between the first and the last key tile'
    out, dqkv = run_fn(qkv, dout, B, N, 0.0)
    _, lse = lib_forward(qkv.to(DEV), B, N, 0.0)
    t1, t2 = LIMITS[dt]
    print(f'rescaling N {N} {dt} {"rising" if rising else "falling"}: row maximum moves by {float(gap.min()):.0f} .. {float(gap.max()):.0f}; '
          f'out {float((out.double().cpu() - ref).abs().max() / ref.abs().max()):.3e}  '
          f'dqkv {float((dqkv.double().cpu() - qr.grad).abs().max() / qr.grad.abs().max()):.3e}  '
          f'lse {float((lse.double().cpu() - lse_ref).abs().max() / lse_ref.abs().max()):.3e}')
    close(out.float(), ref.detach(), t1, 'out')
    close(dqkv.float(), qr.grad, t2, 'dqkv')
    close(lse, lse_ref.detach(), LSE_LIMIT, 'lse')


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
def test_stream_key_order(dt):
    set_dtype(dt)
    N = 576
    B, qkv, dout, ref, _, _, _ = problem(N, 0.0, dt)
    inner = HEADS * 64
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    assert int((perm // 64 != torch.arange(N) // 64).sum()) > N // 2          # most keys change their tile
    rows = (torch.arange(B)[:, None] * N + perm[None, :]).reshape(-1)
    shuffled = qkv.clone()
    shuffled[:, inner:] = qkv[rows, inner:]                                     # K rows and V rows together; Q stays
    out, _ = lib_forward(qkv.to(DEV), B, N, 0.0)
    out_p, _ = lib_forward(shuffled.to(DEV), B, N, 0.0)
    t1, _ = LIMITS[dt]
    print(f'key order N {N} {dt}: permuted against unpermuted {float((out_p.double() - out.double()).abs().max() / out.double().abs().max()):.3e}')
    close(out_p.float(), out.float(), t1, 'out with permuted keys against out')
    close(out_p.float(), ref, t1, 'out with permuted keys against the reference')


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('N', [128, 1024])
def test_stream_padded_layout(dt, N):
    """qkv rows of 3 * heads * 64 + 8 elements with NaN in the pad, out / dout rows of heads * 64 + 8; four sentinel rows behind out
    and dqkv, 64 sentinel floats behind lse and dvec."""
    from fwair.lib import call, dt as dtc
    dtype = set_dtype(dt)
    p = 0.1
    B, qkv, dout, ref, lse_ref, dqkv_ref, _ = problem(N, p, dt)
    inner, rows, nan = HEADS * 64, B * N, float('nan')
    buf = torch.full((rows, 3 * inner + 8), nan, dtype=dtype, device=DEV)
    buf[:, :3 * inner] = qkv.to(DEV)
    out = torch.full((rows + 4, inner + 8), 7.0, dtype=dtype, device=DEV)
    dob = torch.full((rows, inner + 8), nan, dtype=dtype, device=DEV)
    dob[:, :inner] = dout.to(DEV)
    lse = torch.full((B * HEADS * N + 64,), 7.0, dtype=torch.float32, device=DEV)
    dvec = torch.full((B * HEADS * N + 64,), 7.0, dtype=torch.float32, device=DEV)
    dqkv = torch.full((rows + 4, 3 * inner + 8), 7.0, dtype=dtype, device=DEV)
    seed = torch.tensor([SEED], dtype=torch.int32, device=DEV)
    call('fw_gattn_fwd', dtc(dtype), buf, buf[:, inner:], buf[:, 2 * inner:], buf.stride(0), out, out.stride(0), lse, B, HEADS, N,
         64 ** -0.5, seed, SITE, p, None, 0, 1, None, None)
    call('fw_gattn_bwd', dtc(dtype), buf, buf[:, inner:], buf[:, 2 * inner:], buf.stride(0), out, out.stride(0), dob, dob.stride(0),
         lse, dvec, dqkv, dqkv[:, inner:], dqkv[:, 2 * inner:], dqkv.stride(0), B, HEADS, N, 64 ** -0.5, seed, SITE, p,
         None, None, 0, 1, None, None)
    torch.cuda.synchronize()
    t1, t2 = LIMITS[dt]
    close(out[:rows, :inner].float(), ref, t1, 'out')
    close(lse[:B * HEADS * N].view(B, HEADS, N), lse_ref, LSE_LIMIT, 'lse')
    close(dqkv[:rows, :3 * inner].float(), dqkv_ref, t2, 'dqkv')
    same = lambda t: bool((t.float() == 7.0).all())
    assert same(out[rows:]) and same(out[:, inner:]), 'the forward wrote behind or beside out'
    assert same(lse[B * HEADS * N:]) and same(dvec[B * HEADS * N:]), 'lse / dvec written past [B][heads][N]'
    assert same(dqkv[rows:]) and same(dqkv[:, 3 * inner:]), 'the backward wrote behind or beside dqkv'


# ------------------------------------------------------------------------------------------------ 6
def test_stream_domain_of_the_library():
    set_dtype('fp32')
    qkv = lambda N: torch.zeros((N, 3 * HEADS * 64), device=DEV)
    out, lse = lib_forward(qkv(128), 1, 128, 0.0)                             # the plain call at N = 128 has a kernel
    close(lse, torch.full((1, HEADS, 128), 128.0).log(), LSE_LIMIT, 'lse of zero scores')
    lamb = torch.zeros((2, 1, HEADS), device=DEV)
    with pytest.raises(RuntimeError, match='argument check'):
        lib_forward(qkv(128), 1, 128, 0.0, lamb=lamb, nb=2)
    for N in (96, 1088):
        with pytest.raises(RuntimeError, match='argument check'):
            lib_forward(qkv(N), 1, N, 0.0)


def test_band_reweighting_is_refused_at_streaming_sizes():
    """Transformer.run at N = 128: plain attention runs, a band re-weighting (masks on the N x N grid) raises."""
    from fwair import vit as V
    set_dtype('fp32')
    torch.manual_seed(0)
    plain = V.Transformer(128, 1, 2, 64, 256, decompose_type='none').to(DEV)
    x = torch.randn(128, 128, device=DEV)
    with torch.no_grad():
        y = plain.run(x, 1)
    assert y.shape == x.shape and torch.isfinite(y).all()
    for ftype in ('DC', '3_bands'):
        banded = V.Transformer(128, 1, 2, 64, 256, decompose_type=ftype, band_grid='tokens').to(DEV)
        with pytest.raises(NotImplementedError, match='band re-weighting'), torch.no_grad():
            banded.run(x, 1)
