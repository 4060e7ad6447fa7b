"""GPU parity of `--vit_band_grid tokens` at N = 576 and N = 1024 tokens (384x384 / 512x512 inputs): the ViT's band re-weighting with
masks sized by the attention map on the streaming sizes.  '<n>_bands' runs the tiled N x N DFT filter between a probabilities and an
apply kernel (csrc/fw_gattn.hip bandsn_pass_kernel, fw_gattn_bands_fwd / bwd), 'DC' the affine form inside the streaming forward
(gattn_stream_fwd_kernel<T, true>, gattn_dc_rows_kernel / gattn_dc_bwd_kernel with a run-time tile count).

  1  kernel against the f64 FFT statement of encoder_ViT.py:85-92 with N x N masks (convnets_oracle.attn_band_masks(type, N)) and the
     same counter Dropout masks: out, dqkv, dlamb.  Limits (helpers.close, relative to the maximum) are those of
     tests/test_vit_token_bands_gpu.py: fp32 2e-5 / 1e-4 / 2e-4, bf16 1.5e-2 / 3e-2 / 3e-2.  The rounding of an f32 transform chain of
     length 1024 had not been measured, so in fp32 each limit is max(project limit, 4 x the error of the SAME statement evaluated in
     f32 with torch.fft on the CPU against the f64 one); 4 because the MFMA DFT sums in another order.  Nothing is derived from the
     kernel's output.  Printed on the MI355X, fp32, worst case over the cases (out / dqkv / dlamb):
         N  576: f32 statement 4.9e-07 / 7.4e-07 / 7.2e-07,  kernel 1.3e-06 / 1.4e-06 / 1.6e-06
         N 1024: f32 statement 7.8e-07 / 5.7e-07 / 4.4e-07,  kernel 2.0e-06 / 2.4e-06 / 2.9e-06
         ramped scores (3): f32 statement 8.0e-07 / 3.3e-07 / 3.0e-07,  kernel 1.4e-05 / 3.4e-05 / 2.5e-06
     so 4 x the f32 statement's error stays below every project limit and the limits apply unwidened.  bf16: <= 4.7e-03 / 4.1e-03 / 2.1e-06.
  2  invariants (fp32, Dropout off): lamb = 0 is the plain streaming kernel, equal bands scale by 1 + c, 'DC' is the affine form in f64.
  3  tile-walk traps: padded row strides with NaN pads and sentinels around every output; scores that rise / fall by more than 100
     across the key tiles (the online lse feeds the probabilities pass).
  4  domain of the new entry points and of fw_gattn_fwd with lamb.
  5  ViTEncoder at 384x384 with lamb against the CPU oracle (masks re-sized to 576), train mode with Dropout; the engine's graph step."""
import functools

import pytest
import torch
import torch.nn.functional as F

import airnet_oracle as O
import convnets_oracle as C
import dropout_hash as DH
from helpers import close, make_opt, rnd, synth_batch
from test_gattn_stream_gpu import lib_forward, ramped
from test_vit256_gpu import set_dtype
from test_vit384_gpu import VIT, sized_schema

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HEADS, SEED, SITE = 2, 777, 41
LIMITS = {'fp32': (2e-5, 1e-4, 2e-4), 'bf16': (1.5e-2, 3e-2, 3e-2)}
TORCH_DT = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def batch_of(N):
    return 1 if N >= 1024 else 2


def ref_attention(qkv, B, N, heads, drop=None, lamb=None, ftype=None, prec=torch.float64):
    """encoder_ViT.py:76-96 on the CPU in `prec` with N x N band masks: -> (out [B*N, heads*64], softmax map)."""
    x = qkv.to(prec).reshape(B, N, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    attn = ((q @ k.transpose(-1, -2)) * 64 ** -0.5).softmax(-1)
    soft = attn
    if lamb is not None:
        masks = C.attn_band_masks(ftype, N).to(prec)
        spec = torch.fft.fft2(attn)
        bands = torch.stack([torch.fft.ifft2(spec * m).real for m in masks], 0)
        attn = attn + (bands * lamb.to(prec)[:, :, :, None, None]).sum(0)
    if drop is not None:
        seed, site, p = drop
        attn = attn * torch.from_numpy(DH.keep_mask(seed, site, tuple(attn.shape), p)).to(prec) / (1.0 - p)
    return (attn @ v).transpose(1, 2).reshape(B * N, heads * 64), soft


def statement(qkv0, dout0, lamb0, B, N, p, ftype, prec):
    """(out, dqkv, dlamb) of the statement in `prec` on the dtype-rounded operands"""
    qr = qkv0.float().clone().requires_grad_(True)
    lr = lamb0.clone().requires_grad_(True) if lamb0 is not None else None
    out, _ = ref_attention(qr, B, N, HEADS, (SEED, SITE, p) if p > 0 else None, lr, ftype, prec)
    (out * dout0.to(prec)).sum().backward()
    return out.detach().double(), qr.grad.double(), (lr.grad.double() if lr is not None else None)


def operands(N, dtype, tag, B):
    g = torch.Generator().manual_seed(N + tag)
    qkv0 = (torch.randn(B * N, 3 * HEADS * 64, generator=g) * 0.8).to(dtype)
    dout0 = (torch.randn(B * N, HEADS * 64, generator=g) * 0.5).to(dtype)
    return g, qkv0, dout0


@functools.lru_cache(maxsize=None)
def problem(N, p, ftype, batchwise, dt):
    """operands, lamb ~ 0.5 randn, the f64 statement and (fp32) the f32 statement's error against it, computed once"""
    B, dtype = batch_of(N), TORCH_DT[dt]
    nb = 2 if ftype == 'DC' else int(ftype.split('_')[0])
    g, qkv0, dout0 = operands(N, dtype, int(p * 100) + 7 * batchwise + nb, B)
    lamb0 = torch.randn(nb, B if batchwise else 1, HEADS, generator=g) * 0.5
    ref = statement(qkv0, dout0, lamb0, B, N, p, ftype, torch.float64)
    e32 = None
    if dt == 'fp32':
        e32 = tuple(err(a, b) for a, b in zip(statement(qkv0, dout0, lamb0, B, N, p, ftype, torch.float32), ref))
    return B, qkv0, dout0, lamb0, ref, e32


def err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def limits(dt, e32):
    """project limits; fp32: max(project limit, 4 x the f32 statement's own error)"""
    lim = LIMITS[dt]
    return lim if e32 is None else tuple(max(t, 4 * e) for t, e in zip(lim, e32))


def tables(ftype, N):
    """What Transformer.run hands to the kernel: nothing for 'DC' (affine form), the N x N tables for <n>_bands."""
    from fwair import vit as V
    return None if ftype == 'DC' else V._spectral_tables('bands', int(ftype.split('_')[0]), torch.device(DEV), n=N)


def run_kernel(qkv0, dout0, lamb0, B, N, p, ftype='DC'):
    from fwair import functional as Fn
    from fwair import vit as V
    Fn.set_dropout_seed(SEED, DEV, frozen=True)
    try:
        qk = qkv0.to(DEV).requires_grad_(True)
        lk = torch.nn.Parameter(lamb0.to(DEV)) if lamb0 is not None else None
        out = V.GlobalAttnFn.apply(qk, lk, (B, N, HEADS, p, SITE, tables(ftype, N) if lamb0 is not None else None))
        out.backward(dout0.to(DEV))
        torch.cuda.synchronize()
    finally:
        Fn.set_dropout_seed(1, DEV, frozen=False)
    return out.detach(), qk.grad, (lk.grad if lk is not None else None)


CASES = [(576, 0.0, '3_bands', False), (576, 0.1, '3_bands', False), (576, 0.0, '5_bands', False), (576, 0.1, 'DC', False),
         (576, 0.1, 'DC', True), (576, 0.1, '3_bands', True),
         (1024, 0.0, '3_bands', False), (1024, 0.1, '3_bands', False), (1024, 0.0, '5_bands', False), (1024, 0.1, 'DC', False)]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('N,p,ftype,batchwise', CASES)
def test_kernel_vs_f64_fft_statement(dt, N, p, ftype, batchwise):
    set_dtype(dt)
    B, qkv0, dout0, lamb0, ref, e32 = problem(N, p, ftype, batchwise, dt)
    out, dqkv, dlamb = run_kernel(qkv0, dout0, lamb0, B, N, p, ftype)
    t1, t2, t3 = limits(dt, e32)
    f32s = 'f32 statement out {:.3e} dqkv {:.3e} dlamb {:.3e}; '.format(*e32) if e32 else ''
    print(f'N {N} {ftype} p={p} batchwise={batchwise} {dt}: {f32s}kernel out {err(out, ref[0]):.3e} (limit {t1:.1e}) '
          f'dqkv {err(dqkv, ref[1]):.3e} (limit {t2:.1e}) dlamb {err(dlamb, ref[2]):.3e} (limit {t3:.1e})')
    assert out.dtype == TORCH_DT[dt] and dlamb.shape == lamb0.shape
    close(out.float(), ref[0], t1, 'out')
    close(dqkv.float(), ref[1], t2, 'dqkv')
    close(dlamb, ref[2], t3, 'dlamb')


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('ftype', ['3_bands', 'DC'])
@pytest.mark.parametrize('N', [576, 1024])
def test_invariants_without_an_fft_reference(N, ftype):
    """fp32, Dropout off: lamb = 0 is the plain streaming kernel; all bands equal to c scale the output by 1 + c (the bands sum to
    the map); 'DC' is the affine form (1 + lamb1) A + (lamb0 - lamb1) / N evaluated in f64."""
    dtype = set_dtype('fp32')
    B = batch_of(N)
    nb = 2 if ftype == 'DC' else 3
    g, qkv0, dout0 = operands(N, dtype, 3, B)
    base, dbase, _ = run_kernel(qkv0, dout0, None, B, N, 0.0)
    out, dqkv, _ = run_kernel(qkv0, dout0, torch.zeros(nb, 1, HEADS), B, N, 0.0, ftype)
    close(out, base, 2e-5, 'lamb = 0: out')
    close(dqkv, dbase, 1e-4, 'lamb = 0: dqkv')
    c = 0.375
    out, dqkv, _ = run_kernel(qkv0, dout0, torch.full((nb, 1, HEADS), c), B, N, 0.0, ftype)
    close(out, (1 + c) * base, 2e-5, 'equal bands: out')
    close(dqkv, (1 + c) * dbase, 1e-4, 'equal bands: dqkv')
    if ftype == 'DC':
        lamb0 = torch.randn(2, B, HEADS, generator=g) * 0.5
        _, soft = ref_attention(qkv0, B, N, HEADS)
        l0, l1 = (lamb0[i].double()[:, :, None, None] for i in range(2))
        v = qkv0.double().reshape(B, N, 3, HEADS, 64)[:, :, 2].transpose(1, 2)
        affine = (((1 + l1) * soft + (l0 - l1) / N) @ v).transpose(1, 2).reshape(B * N, HEADS * 64)
        out, _, _ = run_kernel(qkv0, dout0, lamb0, B, N, 0.0)
        close(out, affine, 2e-5, 'affine form')


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('ftype', ['3_bands', 'DC'])
def test_padded_layout(dt, ftype):
    """qkv rows of 3 * heads * 64 + 8 elements with NaN in the pad, out / dout rows of heads * 64 + 8; four sentinel rows behind out
    and dqkv, 64 sentinel floats behind lse and dvec, sentinel columns beside out and dqkv."""
    from fwair.lib import call, dt as dtc
    dtype = set_dtype(dt)
    N, p = 576, 0.1
    B, qkv0, dout0, lamb0, ref, e32 = problem(N, p, ftype, False, dt)
    nb = lamb0.shape[0]
    inner, rows, nan, maps = HEADS * 64, B * N, float('nan'), B * HEADS
    buf = torch.full((rows, 3 * inner + 8), nan, dtype=dtype, device=DEV)
    buf[:, :3 * inner] = qkv0.to(DEV)
    out = torch.full((rows + 4, inner + 8), 7.0, dtype=dtype, device=DEV)
    dob = torch.full((rows, inner + 8), nan, dtype=dtype, device=DEV)
    dob[:, :inner] = dout0.to(DEV)
    lse = torch.full((maps * N + 64,), 7.0, dtype=torch.float32, device=DEV)
    dvec = torch.full((maps * N + 64,), 7.0, dtype=torch.float32, device=DEV)
    dqkv = torch.full((rows + 4, 3 * inner + 8), 7.0, dtype=dtype, device=DEV)
    seed = torch.tensor([SEED], dtype=torch.int32, device=DEV)
    lam = lamb0.to(DEV)
    dlam = torch.zeros_like(lam)
    q, k, v = buf, buf[:, inner:], buf[:, 2 * inner:]
    if ftype == 'DC':
        call('fw_gattn_fwd', dtc(dtype), q, k, v, buf.stride(0), out, out.stride(0), lse, B, HEADS, N, 64 ** -0.5, seed, SITE, p,
             lam, nb, 1, None, None)
        call('fw_gattn_bwd', dtc(dtype), q, k, v, buf.stride(0), out, out.stride(0), dob, dob.stride(0), lse, dvec, dqkv, dqkv[:, inner:],
             dqkv[:, 2 * inner:], dqkv.stride(0), B, HEADS, N, 64 ** -0.5, seed, SITE, p, lam, dlam, nb, 1, None, None)
    else:
        bidx, panels = tables(ftype, N)
        amap = torch.full((maps * N * N + 64,), 7.0, dtype=torch.float32, device=DEV)
        pmap, gmap = torch.full_like(amap, 7.0), torch.full_like(amap, 7.0)
        work = torch.full((6 * maps * N * N + 64,), 7.0, dtype=torch.float32, device=DEV)
        call('fw_gattn_bands_fwd', dtc(dtype), q, k, v, buf.stride(0), out, out.stride(0), lse, B, HEADS, N, 64 ** -0.5, seed, SITE, p,
             lam, nb, 1, bidx, panels, amap, work)
        torch.cuda.synchronize()
        assert bool((work[4 * maps * N * N:] == 7.0).all()), 'the forward wrote past its 4 * maps * N * N floats of work'
        call('fw_gattn_bands_bwd', dtc(dtype), q, k, v, buf.stride(0), dob, dob.stride(0), lse, dvec, dqkv, dqkv[:, inner:],
             dqkv[:, 2 * inner:], dqkv.stride(0), B, HEADS, N, 64 ** -0.5, seed, SITE, p, lam, dlam, nb, 1, bidx, panels, amap, pmap,
             gmap, work)
        torch.cuda.synchronize()
        for name, t in (('amap', amap), ('pmap', pmap), ('gmap', gmap)):
            assert bool((t[maps * N * N:] == 7.0).all()), f'{name} written past [B*heads][N][N]'
        assert bool((work[6 * maps * N * N:] == 7.0).all()), 'the backward wrote past its 6 * maps * N * N floats of work'
    torch.cuda.synchronize()
    t1, t2, t3 = limits(dt, e32)
    close(out[:rows, :inner].float(), ref[0], t1, 'out')
    close(dqkv[:rows, :3 * inner].float(), ref[1], t2, 'dqkv')
    close(dlam, ref[2], t3, 'dlamb')
    same = lambda t: bool((t.float() == 7.0).all())
    assert same(out[rows:]) and same(out[:, inner:]), 'the forward wrote behind or beside out'
    assert same(lse[maps * N:]) and same(dvec[maps * N:]), 'lse / dvec written past [B][heads][N]'
    assert same(dqkv[rows:]) and same(dqkv[:, 3 * inner:]), 'the backward wrote behind or beside dqkv'


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('rising', [True, False], ids=['rising', 'falling'])
def test_bands_on_ramped_scores(dt, rising):
    """'3_bands' at N = 576 on the inputs of test_gattn_stream_gpu.test_stream_rescaling: the row maximum moves by more than 100
    between the first and the last key tile, so a probabilities pass fed by a wrongly rescaled lse writes inf, NaN or a wrong map."""
    set_dtype(dt)
    N, ftype = 576, '3_bands'
    B, qkv0, dout0 = ramped(N, dt, rising)
    lamb0 = torch.randn(3, 1, HEADS, generator=torch.Generator().manual_seed(11)) * 0.5
    ref = statement(qkv0, dout0, lamb0, B, N, 0.0, ftype, torch.float64)
    assert all(torch.isfinite(t).all() for t in ref)
    e32 = None
    if dt == 'fp32':
        e32 = tuple(err(a, b) for a, b in zip(statement(qkv0, dout0, lamb0, B, N, 0.0, ftype, torch.float32), ref))
    out, dqkv, dlamb = run_kernel(qkv0, dout0, lamb0, B, N, 0.0, ftype)
    t1, t2, t3 = limits(dt, e32)
    f32s = 'f32 statement out {:.3e} dqkv {:.3e} dlamb {:.3e}; '.format(*e32) if e32 else ''
    print(f'ramped {"rising" if rising else "falling"} {dt}: {f32s}kernel out {err(out, ref[0]):.3e} (limit {t1:.1e}) '
          f'dqkv {err(dqkv, ref[1]):.3e} (limit {t2:.1e}) dlamb {err(dlamb, ref[2]):.3e} (limit {t3:.1e})')
    close(out.float(), ref[0], t1, 'out')
    close(dqkv.float(), ref[1], t2, 'dqkv')
    close(dlamb, ref[2], t3, 'dlamb')


# ------------------------------------------------------------------------------------------------ 4
def test_domain_of_the_library():
    from fwair import vit as V
    from fwair.lib import call
    set_dtype('fp32')
    lamb = torch.zeros((3, 1, HEADS), device=DEV)
    for N in (128, 640):
        qkv = torch.zeros((N, 3 * HEADS * 64), device=DEV)
        inner = HEADS * 64
        out = torch.empty((N, inner), device=DEV)
        lse = torch.empty((1, HEADS, N), device=DEV)
        bidx, panels = V._spectral_tables('bands', 3, torch.device(DEV), n=N)
        maps = [torch.empty((HEADS, N, N), device=DEV) for _ in range(3)]
        work = torch.empty((6, HEADS, N, N), device=DEV)
        with pytest.raises(RuntimeError, match='argument check'):
            call('fw_gattn_bands_fwd', 0, qkv, qkv[:, inner:], qkv[:, 2 * inner:], qkv.stride(0), out, out.stride(0), lse, 1, HEADS, N,
                 64 ** -0.5, None, SITE, 0.0, lamb, 3, 1, bidx, panels, maps[0], work)
        dqkv, dvec, dlamb = torch.empty_like(qkv), torch.empty_like(lse), torch.zeros_like(lamb)
        with pytest.raises(RuntimeError, match='argument check'):
            call('fw_gattn_bands_bwd', 0, qkv, qkv[:, inner:], qkv[:, 2 * inner:], qkv.stride(0), out, out.stride(0), lse, dvec, dqkv,
                 dqkv[:, inner:], dqkv[:, 2 * inner:], dqkv.stride(0), 1, HEADS, N, 64 ** -0.5, None, SITE, 0.0, lamb, dlamb, 3, 1, bidx,
                 panels, maps[0], maps[1], maps[2], work)
    dc = torch.zeros((2, 1, HEADS), device=DEV)
    out, lse = lib_forward(torch.zeros((576, 3 * HEADS * 64), device=DEV), 1, 576, 0.0, lamb=dc, nb=2)     # 'DC' without tables: has a kernel now
    close(lse, torch.full((1, HEADS, 576), 576.0).log(), 2e-5, 'lse of zero scores')
    assert bool((out == 0).all())
    with pytest.raises(RuntimeError, match='argument check'):
        lib_forward(torch.zeros((128, 3 * HEADS * 64), device=DEV), 1, 128, 0.0, lamb=dc, nb=2)
    with pytest.raises(RuntimeError, match='argument check'):                   # more than two bands need the tables and the other entry
        lib_forward(torch.zeros((576, 3 * HEADS * 64), device=DEV), 1, 576, 0.0, lamb=lamb, nb=3)


# ------------------------------------------------------------------------------------------------ 5
def seeded_vit_lamb(size, dt, lamb_shape, **kw):
    """test_vit384_gpu.seeded_vit with name-seeded non-zero lamb in both encoder copies"""
    from net.model import AirNet
    from fwair import functional as Fn
    Fn.config.direct_grads = False
    opt = make_opt('all3', compute_dtype=dt, patch_size=size, **dict(VIT, **kw))
    net = AirNet(opt)
    st = O.fill_state_seeded(sized_schema(size))
    for enc in ('E.E.encoder_q.', 'E.E.encoder_k.'):
        for i in range(12):
            key = f'transformer.layers.{i}.0.fn.lamb'
            st[enc + key] = O.seeded_tensor('E.E.encoder_q.' + key, lamb_shape) / 0.02 * 0.3
    sd = net.state_dict()
    st['E.E.queue'] = F.normalize(O.seeded_tensor('E.E.queue', tuple(sd['E.E.queue'].shape)) / 0.02, dim=1)
    for k in sd:
        assert k in st, k
        if st.get(k) is not None and sd[k].is_floating_point():
            assert tuple(sd[k].shape) == tuple(st[k].shape), k
            sd[k] = st[k]
    net.load_state_dict(sd)
    Fn.set_droppath_override(lambda name, n, rate, device: None)
    return net.to(DEV), opt, st


def test_vit384_encoder_with_lamb_vs_oracle(monkeypatch):
    """ViTEncoder at 384x384, '3_bands' on the 576x576 grid, train mode with every Dropout at p = 0.1, fp32, B = 1, against the CPU
    oracle with its masks re-sized to 576x576: fea, inter and the logits at the limit of test_vit512_encoder_vs_oracle (1e-4), the
    gradient of lamb in the first and the last layer under a fixed cotangent on inter at 2e-3 (test_vit256_train_step_vs_oracle)."""
    from fwair import functional as Fn
    original = C.attn_band_masks
    monkeypatch.setattr(C, 'attn_band_masks', lambda t, n=64: original(t, 576))
    seed = 4242
    net, opt, st = seeded_vit_lamb(384, 'fp32', (3, 1, 12), batch_size=1, frequency_decompose_type='3_bands', vit_band_grid='tokens')
    enc = net.E.E.encoder_q.train()
    pre = 'E.E.encoder_q.'
    names = [f'{pre}transformer.layers.{i}.0.fn.lamb' for i in (0, 11)]
    assert all(float(st[n].abs().min()) > 0 for n in names)
    x = rnd('vit384lamb.x', (1, 3, 384, 384), 0.5)
    cot = rnd('vit384lamb.dinter', (1, 3, 384, 384))
    for n in names:
        st[n] = st[n].clone().requires_grad_(True)
    rfea, rout, rinter = C.vit_encoder(st, pre, opt, x, True, drop=(seed, DH.site_base(pre), 0.1))
    (rinter * cot).sum().backward()
    Fn.set_dropout_seed(seed, DEV, frozen=True)
    try:
        fea, out, inter = enc(x.to(DEV))
        (inter * cot.to(DEV)).sum().backward()
    finally:
        Fn.set_dropout_seed(1, DEV, frozen=False)
    close(fea, rfea, 1e-4, 'fea')
    close(out[0], rout[0], 1e-4, 'logits')
    close(inter, rinter, 1e-4, 'inter')
    params = dict(net.named_parameters())
    for n in names:
        print(n, close(params[n].grad, st[n].grad, 2e-3, n))


def test_engine_trains_lamb_at_384():
    """ViT(384) + 3_bands + tokens, bf16, whole-step graph: finite losses, every lamb of the query encoder moves, the key encoder's follows by EMA."""
    from fwair import engine as E
    from fwair import functional as Fn
    net, opt, st = seeded_vit_lamb(384, 'bf16', (3, 1, 12), batch_size=1, frequency_decompose_type='3_bands', vit_band_grid='tokens')
    net.train()
    lq = [l[0].fn.lamb for l in net.E.E.encoder_q.transformer.layers]
    lk = [l[0].fn.lamb for l in net.E.E.encoder_k.transformer.layers]
    before = [p.detach().clone() for p in lq]
    eng = E.TrainEngine(net, lr=1e-4, contrast_loss_weight=0.6, use_graph=True)
    clean, q_, k_ = (t.to(DEV) for t in synth_batch(1, 384, 'vit384bandsgraph.'))
    losses = [eng.step(q_, k_, clean).clone() for _ in range(3)]
    torch.cuda.synchronize()
    Fn.config.direct_grads = False
    assert torch.isfinite(torch.stack(losses)).all()
    m = float(net.E.E.m)
    for i, (a, b, k) in enumerate(zip(before, lq, lk)):
        assert not torch.equal(a, b.detach()), f'layer {i}: lamb did not move'
        assert not torch.equal(a, k.detach()), f'layer {i}: the key encoder lamb did not follow'
        # k <- m k + (1 - m) q three times from k = q = a: |k - a| <= (1 - m^3) max_j |q_j - a|, and one Adam step moves an
        # element by at most lr (1 - beta1) / sqrt(1 - beta2) = 3.17 lr
        dk = (k.detach() - a).abs().max().item()
        assert dk <= (1 - m ** 3) * 3 * 3.17 * 1e-4 * 1.01, f'layer {i}: |dk| {dk:.3e}'


def test_head_dim_grid_at_384_still_raises():
    for ftype, nb in (('3_bands', 3), ('DC', 2)):
        from net.model import AirNet
        net = AirNet(make_opt('all3', compute_dtype='fp32', patch_size=384, vit_band_grid='head_dim', frequency_decompose_type=ftype, **VIT)).to(DEV)
        assert tuple(net.E.E.encoder_q.transformer.layers[0][0].fn.lamb.shape) == (nb, 1, 12)
        net.eval()
        with pytest.raises(NotImplementedError), torch.no_grad():
            net.E.E.encoder_q(torch.zeros(1, 3, 384, 384, device=DEV))
