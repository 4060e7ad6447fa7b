"""The kernels at the layouts fwair/functional.py runs them at, which the unit tests of test_ops_gpu.py (contiguous operands, square
images, fwair.ops wrappers) never reach:

  A  window attention on the q | pad | k | v buffer of QKVFn / WindowAttnFn (k at column roundup(C, 8), fw_attn_bwd's dq_pad zero
     fill, NaN in every pad column an operand has), at H != W, and with more windows than workgroups of the chunked kernels;
  B  LayerNorm backward over more rows than one pass of its capped grid covers, its twin output (the DropPath-scaled operand copy of
     LnResFn.backward), rows with ld > C, and the partial-sums form folded by fw_slab_reduce;
  C  im2col4 / col2im4, pixel_shuffle / pixel_unshuffle and the small depthwise-convolution kernels at H != W;
  D  one training step of the model with every activation buffer (functional.act_empty) born as NaN, pads included.

Every reference is an f64 / f32 statement on the host; limits are those of test_ops_gpu.py unless a test says otherwise."""
import copy
import functools
import sys

import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import (TOL, check_downsample_conv, check_dwconv, check_upsample_convT, close, lam_to_coef, q,
                          ref_window_attention, rnd)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]
NAN = float('nan')


def ops():
    from fwair import ops as _ops
    return _ops


def call(*a):
    from fwair.lib import call as _c
    return _c(*a)


def dt(dtype):
    from fwair.lib import dt as _dt
    return _dt(dtype)


def up8(n):
    return (n + 7) // 8 * 8


def padded(t, ld, dtype, fill):
    """device buffer [rows, ld] of `dtype`, every element `fill`, with the host tensor t in its first columns"""
    buf = torch.full((t.shape[0], ld), fill, dtype=dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV, dtype)
    return buf


def all_equal(t, v):
    return bool((t.float() == v).all())


# ================================================================================================ A. window attention
class AttnCase:
    """One attention problem in the layout of functional.WindowAttnFn: qkv [rows, Cp + 2C] with NaN in columns C .. Cp-1, out / dout
    rows of ld = Cp with NaN pads, dqkv / d2 pre-filled with 7.0.  The reference (ref_window_attention, autograd) sees the unpadded
    operands."""

    def __init__(self, dtype, C, heads, B, H, W, L, mode, shift, lfs=0):
        self.dtype, self.C, self.heads, self.geo = dtype, C, heads, (B, H, W, L, mode, shift)
        self.lfs, self.nb = lfs, {0: 0, 1: 2, 2: 3}[lfs]
        self.D, self.Cp, self.nkt = C // heads, up8(C), (1 if mode == 0 else L - 1)
        self.rows = L * B * H * W
        self.qkv = q(rnd(self.rows, 3 * C), dtype).requires_grad_(True)
        self.tables = (rnd(L * L, 225, heads, seed=1) * 0.5).requires_grad_(True)
        self.lam = (rnd(B, self.nb - 1, heads, seed=2) * 0.3).requires_grad_(True) if lfs else None
        self.ref = ref_window_attention(self.qkv, C, B, H, W, heads, L, mode, shift, self.tables, self.lam, self.nb)
        self.dout = q(rnd(self.rows, C, seed=3), dtype)
        self.ref.backward(self.dout)
        self.lam_grad = self.lam.grad.clone() if lfs else None
        self.ld = up8(self.Cp + 2 * C)
        host = self.qkv.detach()
        self.buf = torch.full((self.rows, self.ld), NAN, dtype=dtype, device=DEV)
        self.buf[:, :C] = host[:, :C].to(DEV, dtype)
        self.buf[:, self.Cp:self.Cp + 2 * C] = host[:, C:].to(DEV, dtype)
        self.tab_d = self.tables.detach().to(DEV)
        self.coef = lam_to_coef(self.lam, self.nb).detach().to(DEV).contiguous() if lfs else None
        self.lfs_tab = ops()._lfs.device_table(dtype, self.buf.device) if lfs == 2 else None

    def forward(self):
        B, H, W, L, mode, shift = self.geo
        C, Cp, buf = self.C, self.Cp, self.buf
        self.out = torch.full((self.rows, Cp), NAN, dtype=self.dtype, device=DEV)
        self.lse = torch.empty((B * (H // 8) * (W // 8) * L * self.heads, 64), dtype=torch.float32, device=DEV)
        call('fw_attn_fwd', dt(self.dtype), self.D, self.nkt, self.lfs, buf, buf[:, Cp:], buf[:, Cp + C:], buf.stride(0), self.out,
             self.out.stride(0), self.lse, self.tab_d, self.coef, self.lfs_tab, B, H, W, self.heads, L, mode, shift, float(self.D) ** -0.5)
        if Cp > C:
            assert bool(torch.isnan(self.out[:, C:]).all()), 'the forward wrote into the pad columns of out'
        return self.out[:, :C]

    def backward(self, dq_pad):
        """-> (dqkv buffer, d2 buffer or None, dbias, dcoef): exactly the call of WindowAttnFn.backward"""
        B, H, W, L, mode, shift = self.geo
        C, Cp, buf = self.C, self.Cp, self.buf
        dout = padded(self.dout, Cp, self.dtype, NAN)
        dqkv = torch.full((self.rows, self.ld), 7.0, dtype=self.dtype, device=DEV)
        d2 = torch.full((self.rows, self.ld), 7.0, dtype=self.dtype, device=DEV) if self.nkt == 2 else None
        dbias = torch.zeros(L * L, 225, self.heads, device=DEV)
        dcoef = torch.zeros(B, self.heads, 3, device=DEV) if self.lfs else None
        call('fw_attn_bwd', dt(self.dtype), self.D, self.nkt, self.lfs, buf, buf[:, Cp:], buf[:, Cp + C:], buf.stride(0), self.out,
             self.out.stride(0), dout, dout.stride(0), self.lse, self.tab_d, self.coef, self.lfs_tab, dqkv, dqkv[:, Cp:], dqkv[:, Cp + C:],
             d2[:, Cp:] if d2 is not None else None, d2[:, Cp + C:] if d2 is not None else None, dqkv.stride(0), dbias, dcoef,
             B, H, W, self.heads, L, mode, shift, float(self.D) ** -0.5, dq_pad)
        if d2 is not None:
            call('fw_add_rows', dt(self.dtype), d2[:, Cp:], d2.stride(0), dqkv[:, Cp:], dqkv.stride(0), self.rows, 2 * C)
        return dqkv, d2, dbias, dcoef

    def check(self, dqkv, dbias, dcoef, tol, tol_sums, what=''):
        C, Cp = self.C, self.Cp
        close(torch.cat([dqkv[:, :C], dqkv[:, Cp:Cp + 2 * C]], 1), self.qkv.grad, tol, what + 'dq | dk | dv')
        close(dbias, self.tables.grad, tol_sums, what + 'dbias tables')
        if self.lfs:
            self.lam.grad = None
            (lam_to_coef(self.lam, self.nb) * dcoef.cpu()).sum().backward()       # chain rule coef -> lambda on the host
            close(self.lam.grad, self.lam_grad, tol_sums, what + 'dlambda')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('L,mode', [(1, 0), (3, 0), (3, 1), (2, 1)])
def test_attention_c28_padded_buffer_and_dq_pad(dtype, L, mode):
    """C = 28, one head (encoder stage 0): k sits at column 32 of 88-column rows, columns 28..31 hold NaN.  (1, 0) and (3, 0) run
    attn2_bwd_kernel, (3, 1) attn2x_bwd_kernel (two key tiles, second gradient slot d2), (2, 1) attn_bwd_kernel.  With dq_pad = 4
    the kernel owes zeros in columns 28..31 of dqkv (QKVFn.backward feeds the whole buffer to one GEMM); with dq_pad = 0 it owes
    them nothing and must leave them alone."""
    case = AttnCase(dtype, 28, 1, 2, 16, 16, L, mode, 4)
    close(case.forward(), case.ref, TOL[dtype], 'out')
    C, Cp = case.C, case.Cp
    for dq_pad in (Cp - C, 0):
        dqkv, d2, dbias, dcoef = case.backward(dq_pad)
        case.check(dqkv, dbias, dcoef, TOL[dtype] * 4, TOL[dtype] * 4, f'dq_pad {dq_pad}: ')
        assert all_equal(dqkv[:, C:Cp], 0.0 if dq_pad else 7.0), \
            f'dq_pad {dq_pad}: pad columns of dqkv must ' + ('be zero in every row' if dq_pad else 'keep what they held')
        if d2 is not None:
            assert all_equal(d2[:, :Cp], 7.0), 'the second key-gradient slot has no dq and no pad to write'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shift', [0, 4])
@pytest.mark.parametrize('H,W', [(16, 24), (24, 16)])
@pytest.mark.parametrize('lfs', [0, 2])
def test_attention_decoder_rectangle(dtype, lfs, H, W, shift):
    """test_attention_decoder at H != W (2 x 3 and 3 x 2 windows per image): window order, roll and shift mask per axis."""
    case = AttnCase(dtype, 112, 2, 2, H, W, 1, 0, shift, lfs)
    close(case.forward(), case.ref, TOL[dtype], 'out')
    dqkv, _, dbias, dcoef = case.backward(0)
    tol = TOL[dtype] * (3 if dtype == torch.bfloat16 else 4)
    case.check(dqkv, dbias, dcoef, tol, tol)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shift', [0, 4])
@pytest.mark.parametrize('H,W', [(16, 24), (24, 16)])
@pytest.mark.parametrize('mode', [0, 1])
def test_attention_encoder_rectangle(dtype, mode, H, W, shift):
    """test_attention_encoder at H != W, three bands, C = 28 in the padded layout (intra: attn2 kernels, inter: attn2x kernels)."""
    case = AttnCase(dtype, 28, 1, 2, H, W, 3, mode, shift)
    close(case.forward(), case.ref, TOL[dtype], 'out')
    dqkv, d2, dbias, dcoef = case.backward(case.Cp - case.C)
    case.check(dqkv, dbias, dcoef, TOL[dtype] * 4, TOL[dtype] * 4)
    assert all_equal(dqkv[:, case.C:case.Cp], 0.0)
    if d2 is not None:
        assert all_equal(d2[:, :case.Cp], 7.0)


def chunk_walk(nwin, chunks):
    """(windows per workgroup, workgroups with work, windows of the last of them, idle workgroups) of the chunked kernels:
    per = ceil(nwin / grid), workgroup i takes [i * per, min(nwin, (i + 1) * per))"""
    per = -(-nwin // chunks)
    busy = -(-nwin // per)
    return per, busy, nwin - (busy - 1) * per, chunks - busy


@pytest.mark.parametrize('dtype', DTYPES)
def test_attention_decoder_ragged_chunks(dtype):
    """attn2_fwd / attn2_bwd (D = 56, LFS 2, 2 heads, L = 1) launch chunks = 256 * per_cu / (heads * L) workgroups per head, per_cu = 2
    if two workgroups' LDS fit 160 KiB, else 1.  LDS bytes (Smem2<T, 56, 2>): bf16 forward 59 904 -> 256 chunks, bf16 backward
    108 032 -> 128; f32 forward 104 960 and backward 157 184 -> 128 each.  B = 1, 56 x 296 is 7 x 37 = 259 windows, the smallest
    count above 256 that leaves a remainder at both 256 and 128 chunks and fits H, W >= 16 (257 is prime):
      256 chunks: 2 windows each, 130 workgroups busy (the last with 1 window), 126 idle;
      128 chunks: 3 windows each, 87 busy (the last with 1), 41 idle.
    Idle workgroups must pass every barrier and add a zero bias gradient."""
    B, H, W, heads = 1, 56, 296, 2
    nwin = B * (H // 8) * (W // 8)
    assert nwin == 259
    for chunks in (256, 128):
        per, busy, last, idle = chunk_walk(nwin, chunks)
        assert per > 1 and last < per and idle > 0, (chunks, per, busy, last, idle)
    case = AttnCase(dtype, 56 * heads, heads, B, H, W, 1, 0, 4, lfs=2)
    close(case.forward(), case.ref, TOL[dtype], 'out')
    dqkv, _, dbias, dcoef = case.backward(0)
    tol = TOL[dtype] * (3 if dtype == torch.bfloat16 else 4)
    case.check(dqkv, dbias, dcoef, tol, tol * 2)


@pytest.mark.parametrize('dtype', DTYPES)
def test_attention_encoder_ragged_chunks(dtype):
    """attn2x_fwd / attn2x_bwd (D = 28, L = 3 inter, 1 head) launch 256 * per_cu / 3 chunks.  LDS bytes (Smem2X<T, 28>): bf16 forward
    39 936 and backward 60 416 -> per_cu 2, 170 chunks; f32 forward 72 704 -> 170, f32 backward 109 568 -> per_cu 1, 85 chunks.
    B = 1, 40 x 280 is 5 x 35 = 175 windows:
      170 chunks: 2 windows each, 88 workgroups busy (the last with 1 window), 82 idle;
       85 chunks: 3 windows each, 59 busy (the last with 1), 26 idle.
    (171 = 9 x 19 windows would be smaller but divides by 3: no remainder in the f32 backward; 173 is prime.)"""
    B, H, W = 1, 40, 280
    nwin = B * (H // 8) * (W // 8)
    assert nwin == 175
    for chunks in (170, 85):
        per, busy, last, idle = chunk_walk(nwin, chunks)
        assert per > 1 and last < per and idle > 0, (chunks, per, busy, last, idle)
    case = AttnCase(dtype, 28, 1, B, H, W, 3, 1, 4)
    close(case.forward(), case.ref, TOL[dtype], 'out')
    dqkv, d2, dbias, dcoef = case.backward(case.Cp - case.C)
    tol = TOL[dtype] * 4
    case.check(dqkv, dbias, dcoef, tol, tol * 2)
    assert all_equal(dqkv[:, case.C:case.Cp], 0.0)
    assert all_equal(d2[:, :case.Cp], 7.0)


# ================================================================================================ B. LayerNorm backward
def ln_step_rows(C):
    """rows one workgroup of ln_bwd_kernel takes per pass: 256 / G lane groups x U rows each (LN_DISPATCH of csrc/fw_norm.hip)"""
    G = 8 if C <= 32 else 16 if C <= 64 else 32 if C <= 128 else 64
    U = 4 if C <= 256 else 2 if C <= 512 else 1
    return 256 // G * U


def ln_blocks(rows, C):
    from fwair.lib import lib
    return lib().fw_layernorm_bwd_blocks(rows, C)


@functools.lru_cache(maxsize=2)
def ln_problem(rows, C):
    """inputs and the forward on the device, shared by the dtypes of a case: x, gamma, beta on the host; x, gamma, mean, rstd on the device"""
    x, g, b = rnd(rows, C) * 2 + 0.3, 1 + 0.1 * rnd(C, seed=1), 0.1 * rnd(C, seed=2)
    xd, gd = x.to(DEV), g.to(DEV)
    _, mean, rstd = ops().layernorm_fwd(xd, gd, b.to(DEV), torch.float32)
    return x, g, b, xd, gd, mean, rstd


def ln_reference(x, g, b, dy, dres=None):
    """f64 autograd through F.layer_norm -> (y, dx [+ dres], dgamma, dbeta)"""
    xr = x.double().requires_grad_(True)
    gr, br = g.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.layer_norm(xr, (x.shape[1],), gr, br)
    y.backward(dy.double())
    return y.detach(), xr.grad + (dres.double() if dres is not None else 0), gr.grad, br.grad


def ln_bwd2(dy, x, g, mean, rstd, rows, C, dx, dres=None, dg=None, db=None, twin=None, twscale=None, rps=1):
    """fw_layernorm_bwd2 on 2-D row-major views (any ld); -> partial sums [blocks, 2C]"""
    partial = torch.empty((ln_blocks(rows, C), 2 * C), dtype=torch.float32, device=DEV)
    call('fw_layernorm_bwd2', dt(dy.dtype), dy, dy.stride(0), x, x.stride(0), g, mean, rstd, dres, dres.stride(0) if dres is not None else 0,
         dx, dx.stride(0), dg, db, partial, rows, C, twin, twin.stride(0) if twin is not None else 0, twscale, rps)
    return partial


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,rows', [(896, 2051), (448, 4101), (224, 16389), (112, 65541), (28, 262221)])
def test_layernorm_bwd_many_passes(dtype, C, rows):
    """More rows than one pass of the capped grid covers, so the loop of ln_bwd_kernel runs 3 times: two full passes and a ragged
    third (3 to 77 rows).  Column sums of 262 221 rows stayed within 1e-4 of the f64 sums, so the limits of test_layernorm hold
    unchanged."""
    blocks, step = ln_blocks(rows, C), ln_step_rows(C)
    assert rows > blocks * step, f'{rows} rows fit one pass of {blocks} blocks x {step} rows: the grid cap moved'
    assert rows % (blocks * step) % step != 0, 'the last pass must end in a partly filled row group'
    x, g, b, xd, gd, mean, rstd = ln_problem(rows, C)
    dy, dres = q(rnd(rows, C, seed=3), dtype), rnd(rows, C, seed=4)
    _, dx_ref, dg_ref, db_ref = ln_reference(x, g, b, dy, dres)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops().layernorm_bwd(dy.to(DEV, dtype), xd, gd, mean, rstd, dg, db, dres=dres.to(DEV))
    close(dx, dx_ref, 1e-4, 'dx')
    close(dg, dg_ref, 1e-4, 'dgamma')
    close(db, db_ref, 1e-4, 'dbeta')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,rps', [(28, 43711), (112, 10925), (896, 343)])
def test_layernorm_bwd_twin(dtype, C, rps):
    """twin = T(dx * twscale[row // rows_per_scale]): the operand of the producing Linear's backward GEMMs.  Three images of rps rows;
    3 * rps is just above one pass of the grid (twin rows of a second pass) and no multiple of the row step."""
    B = 3
    rows = B * rps
    assert rows > ln_blocks(rows, C) * ln_step_rows(C) and rows % ln_step_rows(C) != 0
    x, g, b, xd, gd, mean, rstd = ln_problem(rows, C)
    dy = rnd(rows, C, seed=3).to(DEV, dtype)
    dres = rnd(rows, C, seed=4).to(DEV)
    scale = torch.tensor([0.0, 1 / 0.9, 1 / 0.75])
    dx0 = torch.empty(rows, C, device=DEV)
    ln_bwd2(dy, xd, gd, mean, rstd, rows, C, dx0, dres)
    for twscale in (scale, None):
        dx = torch.empty(rows, C, device=DEV)
        twin = torch.full((rows, C), 7.0, dtype=dtype, device=DEV)
        ln_bwd2(dy, xd, gd, mean, rstd, rows, C, dx, dres, twin=twin, twscale=twscale.to(DEV) if twscale is not None else None, rps=rps)
        assert torch.equal(dx, dx0), 'dx changed with the twin output present'
        want = dx0.cpu() * scale.repeat_interleave(rps)[:, None] if twscale is not None else dx0.cpu()
        got = twin.float().cpu()
        assert torch.isfinite(got).all()
        if dtype == torch.float32:
            assert torch.equal(got, want), f'f32 twin differs from dx * scale by up to {(got - want).abs().max():.3e}'
        elif twscale is None:
            assert torch.equal(got, want.to(torch.bfloat16).float()), 'bf16 twin without a scale must be dx rounded to bf16'
        else:
            over = (got - want).abs() - 2.0 ** -8 * want.abs()
            assert float(over.max()) <= 0.0, f'bf16 twin is {float(over.max()):.3e} beyond one bf16 ulp of dx * scale'
        if twscale is not None:
            assert bool((got[:rps] == 0).all()), 'rows of the image with scale 0 must be exactly zero'
            assert float(got[rps:].abs().max()) > 0.0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,ld,rows', [(28, 32, 1000), (112, 120, 515)])
def test_layernorm_padded_rows(dtype, C, ld, rows):
    """y, dy, twin, dres (and x, dx) as rows of wider buffers, the way functional.act_empty hands them out: inputs carry NaN in
    the pad columns, outputs are pre-filled with 7.0 and must keep it there.  Results as in test_layernorm; mean and rstd are f32
    statistics of at most 112 values, held to the f32 limit TOL[float32]."""
    x, g, b = rnd(rows, C) * 2 + 0.3, 1 + 0.1 * rnd(C, seed=1), 0.1 * rnd(C, seed=2)
    dy, dres = q(rnd(rows, C, seed=3), dtype), rnd(rows, C, seed=4)
    y_ref, dx_ref, dg_ref, db_ref = ln_reference(x, g, b, dy, dres)
    xb, gd, bd = padded(x, ld, torch.float32, NAN), g.to(DEV), b.to(DEV)
    yb = torch.full((rows, ld), 7.0, dtype=dtype, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    call('fw_layernorm_fwd', dt(dtype), xb, ld, gd, bd, yb, ld, mean, rstd, rows, C, 1e-5)
    close(yb[:, :C], y_ref, TOL[dtype], 'y')
    assert all_equal(yb[:, C:], 7.0), 'forward wrote into the pad columns of y'
    close(mean, x.double().mean(1), TOL[torch.float32], 'mean')
    close(rstd, (x.double().var(1, unbiased=False) + 1e-5).rsqrt(), TOL[torch.float32], 'rstd')
    dyb, dresb = padded(dy, ld, dtype, NAN), padded(dres, ld, torch.float32, NAN)
    dxb = torch.full((rows, ld), 7.0, device=DEV)
    twb = torch.full((rows, ld), 7.0, dtype=dtype, device=DEV)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ln_bwd2(dyb[:, :C], xb[:, :C], gd, mean, rstd, rows, C, dxb[:, :C], dresb[:, :C], dg, db, twin=twb[:, :C])
    close(dxb[:, :C], dx_ref, 1e-4, 'dx')
    close(dg, dg_ref, 1e-4, 'dgamma')
    close(db, db_ref, 1e-4, 'dbeta')
    assert torch.equal(twb[:, :C].float(), dxb[:, :C].to(dtype).float()), 'twin without a scale must be T(dx)'
    assert all_equal(dxb[:, C:], 7.0) and all_equal(twb[:, C:], 7.0), 'backward wrote into the pad columns of dx / twin'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,rows', [(28, 1000), (112, 515), (896, 2051)])
def test_layernorm_bwd_partials_fold(dtype, C, rows):
    """dgamma == dbeta == NULL (fwair.ops.layernorm_bwd: the fold is deferred to the end of the backward pass): the block partials
    folded by fw_slab_reduce give the sums of the immediate form."""
    x, g, b, xd, gd, mean, rstd = ln_problem(rows, C)
    dy = rnd(rows, C, seed=3).to(DEV, dtype)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = torch.empty(rows, C, device=DEV)
    ln_bwd2(dy, xd, gd, mean, rstd, rows, C, dx, dg=dg, db=db)
    dx2 = torch.empty(rows, C, device=DEV)
    partial = ln_bwd2(dy, xd, gd, mean, rstd, rows, C, dx2)
    dg2, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    call('fw_slab_reduce', partial, partial.shape[0], C, 2 * C, dg2, 1, db2, C, C)
    assert torch.equal(dx, dx2)
    close(dg2, dg, 1e-6, 'dgamma from the partials')
    close(db2, db, 1e-6, 'dbeta from the partials')
    assert float(dg.abs().max()) > 0 and float(db.abs().max()) > 0


# ================================================================================================ C. layout kernels at H != W
RECT_CONV = [(8, 24), (24, 8)]
RECT_DW = [(16, 40), (40, 16)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('H,W', RECT_CONV)
def test_downsample_conv_rectangle(dtype, H, W):
    check_downsample_conv(dtype, 2, H, W)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('H,W', RECT_CONV)
def test_upsample_convT_rectangle(dtype, H, W):
    check_upsample_convT(dtype, 2, H, W)


@pytest.mark.parametrize('twin', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('H,W', RECT_DW)
def test_dwconv_rectangle(dtype, twin, H, W):
    assert 2 * H * W * 112 < 10_000_000          # below the switch to the tiled kernels: the small dwconv kernels run
    check_dwconv(dtype, twin, 2, H, W)


# ================================================================================================ D. poisoned activation pool
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_train_step_on_poisoned_activation_pool(monkeypatch, dtype):
    """functional.act_empty hands out uninitialised [rows, roundup(cols, 8)] buffers.  Born as NaN (pads included), one eager training
    step of the smallest golden configuration must stay finite and agree with the same step on ordinary buffers -- a consumer that
    reads a column nobody defined (a pad multiplied by a zero weight row, say) shows as NaN.  Limits: those test_train_step_fp32 /
    test_eval_and_train_bf16 hold against their goldens."""
    from fwair import functional as Fn
    from helpers import synth_batch
    from test_model_gpu import build
    real = Fn.act_empty

    def poisoned(rows, cols, dtype, device):
        return torch.full((rows, up8(cols)), NAN, dtype=dtype, device=device)[:, :cols]

    try:
        net, opt = build('all2_L2', dtype)
        state = copy.deepcopy(net.state_dict())
        clean, qi, ki = (t.to(DEV) for t in synth_batch(2, 128, 'model.'))
        CE = torch.nn.CrossEntropyLoss()
        runs = []
        for poison in (False, True):
            net.load_state_dict(state)
            for p_ in net.parameters():
                p_.grad = None
            if poison:
                for mod in list(sys.modules.values()):            # the function and every by-name import of it
                    name = getattr(mod, '__name__', '')
                    if (name.split('.')[0] in ('fwair', 'net')) and getattr(mod, 'act_empty', None) is real:
                        monkeypatch.setattr(mod, 'act_empty', poisoned)
                assert Fn.act_empty is poisoned
            net.train()
            restored, logits, labels = net(x_query=qi, x_key=ki)
            loss = torch.nn.L1Loss()(restored, clean) + opt.contrast_loss_weight * sum(CE(logits[i], labels[i]) for i in range(opt.L)) / opt.L
            loss.backward()
            torch.cuda.synchronize()
            runs.append((restored.detach().float().cpu(), torch.stack(logits).detach().cpu(), loss.detach().cpu(),
                         {n: p_.grad.detach().cpu().clone() for n, p_ in net.named_parameters() if p_.grad is not None}))
    finally:
        Fn.config.compute_dtype = torch.float32
    (r0, l0, loss0, g0), (r1, l1, loss1, g1) = runs
    assert set(g0) == set(g1) and len(g0) > 100
    assert torch.isfinite(loss1).all(), 'loss is not finite on NaN-born buffers'
    bad = [n for n, t in g1.items() if not torch.isfinite(t).all()]
    assert not bad, f'{len(bad)} gradients are not finite on NaN-born buffers, e.g. {bad[:5]}'
    names = sorted(g0)
    n0 = torch.tensor([g0[n].norm().item() for n in names])
    n1 = torch.tensor([g1[n].norm().item() for n in names])
    if dtype == 'fp32':
        close(r1, r0, 1e-4, 'restored')
        close(l1, l0, 2e-4, 'logits')
        close(loss1, loss0, 1e-4, 'loss')
        rel = (n1 - n0).abs() / n0.clamp_min(float(n0.max()) * 1e-6)
        worst = int(rel.argmax())
        assert rel.max() < 5e-3, f'grad norm of {names[worst]}: {n1[worst]:.6e} vs {n0[worst]:.6e}'
        for n in names:      # tensors that are ~0 by cancellation only see float-atomic ordering noise (as in test_train_step_fp32)
            close(g1[n], g0[n], 5e-3 if float(g0[n].norm()) > 1e-6 * float(n0.max()) else 5e-2, 'grad ' + n)
    else:
        assert abs(float(loss1) - float(loss0)) / float(loss0) < 2e-2
        rel = (n1 - n0).abs() / n0.clamp_min(1e-12)
        big = n0 > n0.max() * 1e-3
        assert rel[big].median() < 5e-2, f'median relative grad-norm deviation {rel[big].median():.3e}'
