"""Window attention (csrc/fw_attn.hip) at the paths training runs and no other test reaches, through the C ABI, f32 and bf16, every
output held to the element-wise bounds of helpers.attn_reference (proven on the host by test_window_attention_bounds_cpu.py) AND
to the rel-to-max limits of test_ops_gpu.py:

  B1  a workgroup's walk crosses an image while LFS is on (attn2_fwd re-reads (a, b, c), attn2_bwd flushes the dcoef partial sums);
  B2  the bottleneck geometry H = W = 8, 16 heads: every window is its own image, the image changes at every step of every walk;
  B3  the v1 kernels at size: attn_fwd_kernel's item loop past the 4 096-workgroup grid, attn_bwd_kernel's walk over 5 windows;
  B4  the v1 forms <56> and <64>;
  B5  scores of standard deviation 35: the running max, exp(s - lse) in the backward, the literal -100 of the shift mask;
  B6  the ABI's contracts: dbias / dcoef are accumulated into, nothing is written outside out, lse, the gradients.

Buffers: q | k | v rows of stride 3C + 8 (the 8 pad columns hold NaN in operands and the sentinel in outputs), every output between
guard words (helpers.guarded).  Each case asserts its own walk from the launch arithmetic of fw_attn.hip, for per_cu 1 and 2.

Headroom when these cases were written (largest |error| / bound over all cases, per output; every case prints its own):
  bf16  out 0.82  lse 0.10  dq 0.87  dk 0.92  dv 0.93  dbias 0.12  dcoef 0.16
  f32   out 0.05  lse 0.12  dq 0.12  dk 0.11  dv 0.13  dbias 0.11  dcoef 0.001
The bf16 figures are near 1 because that part of the bound is attained, not padded: with a peaked softmax an output is one product
rounded twice, and the bound allows exactly those two roundings."""

import pytest
import torch

from helpers import (GUARD, SENTINEL, assert_bits, assert_bound_1d, attn1_bwd_chunks, attn2_chunks, attn_inputs, attn_key_slot,
                     attn_outputs_flat, attn_reference, attn_walk, attn_with_prefill, guarded, walk_crossings)
from test_ops_gpu import TOL, close

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]
NAN = float('nan')
PAD = 8


def call(*a):
    from fwair.lib import call as _c
    return _c(*a)


def dt(dtype):
    from fwair.lib import dt as _dt
    return _dt(dtype)


def lfs_table(dtype):
    from fwair import lfs
    return lfs.device_table(dtype, torch.device(DEV))


class Run:
    """fw_attn_fwd + fw_attn_bwd of one helpers.WAttnCase on guarded, padded buffers; results gathered into window order."""

    def __init__(self, c, dbias0=None, dcoef0=None):
        self.c = c
        B, H, W, L, mode, shift = c.geo
        C, rows, T = c.C, L * B * H * W, c.dtype
        self.ld, self.ldo, self.rows = 3 * C + PAD, C + PAD, rows
        qkv = torch.full((rows, self.ld), NAN, dtype=T, device=DEV)
        qkv[:, :3 * C] = c.qkv.to(DEV, T)
        dout = torch.full((rows, self.ldo), NAN, dtype=T, device=DEV)
        dout[:, :C] = c.dout.to(DEV, T)
        tab = c.tables.to(DEV)
        coef = c.coef.to(DEV) if c.lfs else None
        ftab = lfs_table(T) if c.lfs == 2 else None
        nlse = c.nwin * L * c.heads * 64
        self.bufs = {}

        def out_buf(name, n, dtype, init=None):
            buf, view = guarded(n, dtype, DEV)
            if init is not None:
                view.copy_(init.reshape(-1).to(DEV, dtype))
            self.bufs[name] = (buf, view)
            return view
        out = out_buf('out', rows * self.ldo, T).view(rows, self.ldo)
        lse = out_buf('lse', nlse, torch.float32)
        dqkv = out_buf('dqkv', rows * self.ld, T).view(rows, self.ld)
        d2 = out_buf('d2', rows * self.ld, T).view(rows, self.ld) if c.nkt == 2 else None
        self.dbias0 = dbias0 if dbias0 is not None else torch.zeros(L * L, 225, c.heads)
        self.dcoef0 = (dcoef0 if dcoef0 is not None else torch.zeros(B, c.heads, 3)) if c.lfs else None
        dbias = out_buf('dbias', L * L * 225 * c.heads, torch.float32, self.dbias0)
        dcoef = out_buf('dcoef', B * c.heads * 3, torch.float32, self.dcoef0) if c.lfs else None
        geo = (B, H, W, c.heads, L, mode, shift, c.scale)
        call('fw_attn_fwd', dt(T), c.D, c.nkt, c.lfs, qkv, qkv[:, C:], qkv[:, 2 * C:], self.ld, out, self.ldo, lse, tab, coef, ftab, *geo)
        call('fw_attn_bwd', dt(T), c.D, c.nkt, c.lfs, qkv, qkv[:, C:], qkv[:, 2 * C:], self.ld, out, self.ldo, dout, self.ldo, lse, tab,
             coef, ftab, dqkv, dqkv[:, C:], dqkv[:, 2 * C:], d2[:, C:] if d2 is not None else None,
             d2[:, 2 * C:] if d2 is not None else None, self.ld, dbias, dcoef, *geo, 0)
        torch.cuda.synchronize()
        self.out_m, self.dqkv_m, self.d2_m = out.cpu(), dqkv.cpu(), d2.cpu() if d2 is not None else None
        self.lse_flat = lse.cpu()
        res = dict(out=c.gather(self.out_m), dq=c.gather(self.dqkv_m))
        res['lse'] = self.lse_flat.view(c.nwin, L, c.heads, 64).transpose(0, 1).double()
        slots = [self.dqkv_m, self.d2_m]
        gk = [[c.gather(m[:, C:]) if m is not None else None for m in slots], [c.gather(m[:, 2 * C:]) if m is not None else None for m in slots]]
        for name, per_slot in (('dk', gk[0]), ('dv', gk[1])):
            res[name] = [[per_slot[attn_key_slot(lq, lk) if c.nkt == 2 else 0][lk] for lk in c.keys(lq)] for lq in range(L)]
        res['dbias'] = dbias.cpu().view(L * L, 225, c.heads).double()
        if c.lfs:
            res['dcoef'] = dcoef.cpu().view(B, c.heads, 3).double()
        self.res = res

    def check_untouched(self):
        """guards and pad columns hold the sentinel bit for bit; no sentinel is left inside lse; what no (query, key) band pair owns
        in the second key-gradient slot is untouched too"""
        c, C = self.c, self.c.C
        for name, (buf, view) in self.bufs.items():
            want = torch.full((GUARD,), SENTINEL, dtype=buf.dtype)
            assert_bits(buf[:GUARD], want, f'{name}: guard in front')
            assert_bits(buf[-GUARD:], want, f'{name}: guard behind')
        for name, m, c0 in (('out', self.out_m, C), ('dqkv', self.dqkv_m, 3 * C), ('d2', self.d2_m, 3 * C)):
            if m is not None:
                assert_bits(m[:, c0:], torch.full_like(m[:, c0:], SENTINEL), f'{name}: pad columns')
        if self.d2_m is not None:
            assert_bits(self.d2_m[:, :C], torch.full_like(self.d2_m[:, :C], SENTINEL), 'd2: no query gradient lives in the second slot')
        assert not bool((self.lse_flat == SENTINEL).any()), 'lse: an element was never written'

    def check(self, what, v1=False):
        """every output within the element-wise bound (the backward's from the lse the kernel itself produced) and the rel-to-max limit"""
        c, T = self.c, self.c.dtype
        lse_in = self.res['lse']
        ref = attn_reference(c, lse_in=lse_in, v1=v1)
        if bool(self.dbias0.any()) or (c.lfs and bool(self.dcoef0.any())):
            ref = attn_with_prefill(ref, c, self.dbias0, self.dcoef0, v1)
        val = attn_outputs_flat({n: v for n, (v, _) in ref.items()})
        tol = attn_outputs_flat({n: t for n, (_, t) in ref.items()})
        got = attn_outputs_flat(self.res)
        grad = TOL[T] * (3 if T == torch.bfloat16 else 4)
        limit = dict(out=TOL[T], dq=grad, dk=grad, dv=grad, dbias=2 * grad, dcoef=2 * grad)
        worst = {}
        for n in ('out', 'lse', 'dq', 'dk', 'dv', 'dbias', 'dcoef'):
            if n not in val:
                continue
            assert torch.isfinite(got[n]).all(), f'{what} {n}: non-finite values'
            ratio = ((got[n] - val[n]).abs() / tol[n]).nan_to_num(0.0)
            worst[n] = float(ratio.max())
            print(f'{what} [{str(T)[6:]}] {n}: worst error / bound {worst[n]:.3f}, median bound {float(tol[n].median()):.3e}, '
                  f'median |ref| {float(val[n].abs().median()):.3e}')
        for n in worst:
            assert_bound_1d(got[n], val[n], tol[n], f'{what} {n}')
            if n == 'dcoef':                                     # as d(lambda) weighs it: b enters with 1 / 64
                wts = torch.tensor([1.0, 1 / 64, 1.0]).repeat(val[n].numel() // 3)
                close(got[n] * wts, val[n] * wts, limit[n], f'{what} {n}')
            elif n != 'lse':
                close(got[n], val[n], limit[n], f'{what} {n}')
        self.check_untouched()
        return worst


def assert_v2_walk(c, expect):
    """expect: {per_cu: (chunks, per, busy, last, idle)} of attn2_* / attn2x_*"""
    for per_cu, want in expect.items():
        chunks = attn2_chunks(c.nwin, c.heads, c.geo[3], per_cu)
        assert (chunks,) + attn_walk(c.nwin, chunks) == want, (per_cu, chunks, attn_walk(c.nwin, chunks), want)


def assert_one_window_per_workgroup(c, v1):
    """the 12 windows of the small cases: as many workgroups as windows, nobody walks (B5, B6 are about values, not walks)"""
    L = c.geo[3]
    for chunks in ([attn1_bwd_chunks(c.nwin, c.heads, L)] if v1 else [attn2_chunks(c.nwin, c.heads, L, p) for p in (1, 2)]):
        assert (chunks,) + attn_walk(c.nwin, chunks) == (c.nwin, 1, c.nwin, 1, 0)


# ================================================================================================ B1
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lfs', [1, 2])
def test_walk_crosses_an_image_with_lfs(dtype, lfs):
    """D 56, 8 heads (C 448), B 3, 40 x 56 = 35 windows per image, 105 in all, shift 4, coefficients differ per image.  32 chunks
    (per_cu 1) walk 4 windows each, 64 chunks 2 each; neither divides 35, so windows 35 and 70 lie inside a walk: the first case in
    which attn2_fwd_kernel<.., LFS> re-reads (a, b, c) in mid-walk and attn2_bwd_kernel flushes its dcoef partial sums there; also the
    first run of LFS 1 and of attn2_* with more than 4 heads."""
    c = attn_inputs(dtype, 56, 8, 3, 40, 56, 1, 0, 4, lfs)
    assert c.nW == 35 and c.nwin == 105
    assert_v2_walk(c, {1: (32, 4, 27, 1, 5), 2: (64, 2, 53, 1, 11)})
    for per_cu in (1, 2):
        chunks = attn2_chunks(c.nwin, c.heads, 1, per_cu)
        crossed = walk_crossings(c.nwin, chunks, c.nW)
        assert crossed and set(crossed) <= {35, 70}, (chunks, crossed)
    assert len({tuple(c.coef[b].reshape(-1).tolist()) for b in range(3)}) == 3
    Run(c).check(f'B1 lfs {lfs}')


# ================================================================================================ B2
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lfs', [0, 2])
def test_bottleneck_geometry(dtype, lfs):
    """H = W = 8 (one window per image), 16 heads (C 896), B 40, shift 0: 16 chunks walk 3 windows each (the last 1), 32 chunks 2 each;
    the image -- and with LFS the coefficients and the dcoef words -- changes at every step.  First kernel test at H = W = 8 and at
    16 heads."""
    c = attn_inputs(dtype, 56, 16, 40, 8, 8, 1, 0, 0, lfs)
    assert c.nW == 1 and c.nwin == 40
    assert_v2_walk(c, {1: (16, 3, 14, 1, 2), 2: (32, 2, 20, 2, 12)})
    Run(c).check(f'B2 lfs {lfs}')


# ================================================================================================ B3
@pytest.mark.parametrize('dtype', DTYPES)
def test_v1_kernels_at_size(dtype):
    """L = 2, mode 1, D 28, 2 heads, B 2, 136 x 248 = 527 windows per image, 1 054 in all, shift 4.  attn_fwd_kernel<28>: 4 216 items
    on a grid capped at 4 096, so 120 workgroups take a second item (the trailing barrier between items).  attn_bwd_kernel<28>:
    1024 / (2 * 2) = 256 chunks of 5 windows, 211 busy (the last with 4), 45 idle; 527 is no multiple of 5, so a walk crosses the
    image.  Before this the v1 kernels only ever saw 32 items and one window per workgroup."""
    c = attn_inputs(dtype, 28, 2, 2, 136, 248, 2, 1, 4, 0)
    assert c.nW == 527 and c.nwin == 1054
    items = c.nwin * 2 * c.heads
    assert items == 4216 and items - 4096 == 120
    chunks = attn1_bwd_chunks(c.nwin, c.heads, 2)
    assert (chunks,) + attn_walk(c.nwin, chunks) == (256, 5, 211, 4, 45)
    assert walk_crossings(c.nwin, chunks, c.nW) == [527]
    Run(c).check('B3', v1=True)


# ================================================================================================ B4
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', [56, 64])
def test_v1_forms_56_and_64(dtype, D):
    """attn_fwd_kernel / attn_bwd_kernel <56> and <64>: L = 2, mode 1, one head, B 2, 16 x 16, shift 4.  The model in its default
    configuration cannot reach them: inter-band attention exists in the Uformer encoder only, whose head dimension is
    encoder_embed_dim (28) at every stage (dim 28 * 2^i over 2^i heads).  An encoder built with encoder_embed_dim 56 or 64 and L = 2
    would, and the C ABI does: the dispatch instantiates them, so they have to be right."""
    c = attn_inputs(dtype, D, 1, 2, 16, 16, 2, 1, 4, 0)
    chunks = attn1_bwd_chunks(c.nwin, 1, 2)
    assert (chunks,) + attn_walk(c.nwin, chunks) == (8, 1, 8, 1, 0)
    Run(c).check(f'B4 D {D}', v1=True)


# ================================================================================================ B5
LARGE = {'decoder lfs 0': (56, 2, 2, 16, 24, 1, 0, 4, 0), 'decoder lfs 2': (56, 2, 2, 16, 24, 1, 0, 4, 2),
         'intra L 3': (28, 2, 2, 16, 24, 3, 0, 4, 0), 'inter L 3': (28, 2, 2, 16, 24, 3, 1, 4, 0), 'inter L 2': (28, 2, 2, 16, 24, 2, 1, 4, 0)}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(LARGE))
def test_large_scores(dtype, name):
    """q and k scaled so that the scores have a standard deviation of 35: row maxima pass 88.7 (exp overflows in f32 unless the running
    max is subtracted), exp(s - lse) in the backward spans the whole f32 range, and a masked key (-100) is no longer negligible next
    to an unmasked one -- the reference with -50 is rejected on these inputs (test_window_attention_bounds_cpu.py).  Everything must
    be finite and inside the bounds; lse against the f64 log-sum-exp."""
    c = attn_inputs(dtype, *LARGE[name], score_std=35.0)
    assert_one_window_per_workgroup(c, v1=name == 'inter L 2')
    Run(c).check(f'B5 {name}', v1=name == 'inter L 2')


# ================================================================================================ B6
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['decoder lfs 2', 'inter L 3'])
def test_gradient_buffers_are_accumulated_into(dtype, name):
    """include/fwair.h: dbias and dcoef are ACCUMULATED into.  Both are pre-filled with seeded values of the gradient's own magnitude
    (the rms of the reference gradient, per component of dcoef): the result is pre-fill + gradient within the bound plus one rounding
    of |pre-fill| per atomic addition.  Guards, pad columns and lse coverage are checked as in every case of this file."""
    c = attn_inputs(dtype, *LARGE[name])
    assert_one_window_per_workgroup(c, v1=False)
    ref = attn_reference(c)
    g = torch.Generator().manual_seed(11)
    rms = lambda t, dims: (t * t).mean(dims, keepdim=True).sqrt()
    dbias0 = (torch.randn(ref['dbias'][0].shape, generator=g) * rms(ref['dbias'][0], (0, 1, 2))).float()
    dcoef0 = (torch.randn(ref['dcoef'][0].shape, generator=g) * rms(ref['dcoef'][0], (0, 1))).float() if c.lfs else None
    run = Run(c, dbias0, dcoef0)
    run.check(f'B6 {name}')
    moved = (run.res['dbias'] - dbias0.double()).abs().max()
    assert float(moved) > 0.1 * float(ref['dbias'][0].abs().max()), 'dbias: the gradient did not arrive on top of the pre-fill'
