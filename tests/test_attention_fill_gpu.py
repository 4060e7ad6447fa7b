"""Window attention (csrc/fw_attn.hip) at the grids the v2 kernels launch since their fill follows the runtime's occupancy query:
grid.x = 256 * (workgroups of the compiled kernel one CU holds) / (heads * L), clamped to the window count, the backward held at two
per CU while a third would leave walks of fewer than 4 windows.  Through the C ABI on guarded, padded buffers
(test_window_attention_pin_gpu.Run), every output held to helpers.attn_reference and its element-wise bounds; every walk is taken
from fw_attn_chunks, the same code the launch runs, never from a copy of its arithmetic.

  F1  fewer windows than workgroups: B = 1 at 8 x 8 (one window, 16 heads) and 16 x 16 (4 windows): grid.x is the window count,
      each workgroup owns one window;
  F2  ragged walks at the new fill, per KERNEL (forward and backward hold different numbers of workgroups per CU): geometry chosen
      from fw_attn_chunks (attn_fill_cases.choose_ragged) so that the last busy workgroup is short, at least one workgroup is idle
      and an image boundary lies inside a walk; shift 0 and 4; LFS with per-image coefficients;
  F3  the ABI's contracts at such a grid: dbias / dcoef pre-filled are accumulated into (one more rounding of the pre-fill per
      atomic addition, counted from the walk fw_attn_chunks reports), guards and pad columns untouched (every case checks those).

helpers.attn_reference counts the roundings of the dbias / dcoef chains from the walks of one and two workgroups per CU; at three to
six the chains are shorter per workgroup and longer across workgroups.  The u-terms involved are two orders below the bounds' other
terms (headroom printed per case)."""

import functools

import pytest
import torch

from attn_fill_cases import FAMILIES, choose_ragged, walk_properties
from helpers import U32, attn_inputs, attn_outputs_flat, attn_reference, attn_walk, assert_bound_1d
from test_ops_gpu import TOL, close
from test_window_attention_pin_gpu import Run, dt

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def chunks_of(dtype, family, backward, nwin, heads):
    """grid.x of the launch, from the library"""
    from fwair import lib
    D, _, L, mode, lfs = FAMILIES[family]
    n = lib.lib().fw_attn_chunks(dt(dtype), D, 1 if mode == 0 else L - 1, lfs, int(backward), nwin, heads, L)
    assert n > 0, f'fw_attn_chunks -> {n}'
    return n


class FillRun(Run):
    def check(self, what, chunks_bwd):
        """Run.check with the pre-fill's roundings counted from the backward's own walk: one atomic addition per busy workgroup lands
        on a dbias word, one per wave of every workgroup holding windows of the image on a dcoef word"""
        c, T = self.c, self.c.dtype
        ref = attn_reference(c, lse_in=self.res['lse'])
        per, busy, _, _ = attn_walk(c.nwin, chunks_bwd)
        if bool(self.dbias0.any()):
            ref['dbias'] = (ref['dbias'][0] + self.dbias0.double(), ref['dbias'][1] + busy * U32 * self.dbias0.double().abs())
        if c.lfs and bool(self.dcoef0.any()):
            adds = 4 * (-(-c.nW // per) + 1)
            ref['dcoef'] = (ref['dcoef'][0] + self.dcoef0.double(), ref['dcoef'][1] + adds * U32 * self.dcoef0.double().abs())
        val = attn_outputs_flat({n: v for n, (v, _) in ref.items()})
        tol = attn_outputs_flat({n: t for n, (_, t) in ref.items()})
        got = attn_outputs_flat(self.res)
        grad = TOL[T] * (3 if T == torch.bfloat16 else 4)
        limit = dict(out=TOL[T], dq=grad, dk=grad, dv=grad, dbias=2 * grad, dcoef=2 * grad)
        for n in ('out', 'lse', 'dq', 'dk', 'dv', 'dbias', 'dcoef'):
            if n not in val:
                continue
            assert torch.isfinite(got[n]).all(), f'{what} {n}: non-finite values'
            ratio = ((got[n] - val[n]).abs() / tol[n]).nan_to_num(0.0)
            print(f'{what} [{str(T)[6:]}] {n}: worst error / bound {float(ratio.max()):.3f}')
            assert_bound_1d(got[n], val[n], tol[n], f'{what} {n}')
            if n == 'dcoef':
                wts = torch.tensor([1.0, 1 / 64, 1.0]).repeat(val[n].numel() // 3)
                close(got[n] * wts, val[n] * wts, limit[n], f'{what} {n}')
            elif n != 'lse':
                close(got[n], val[n], limit[n], f'{what} {n}')
        self.check_untouched()


def case_of(dtype, family, heads, B, H, W, shift):
    D, _, L, mode, lfs = FAMILIES[family]
    return attn_inputs(dtype, D, heads, B, H, W, L, mode, shift, lfs)


@functools.lru_cache(maxsize=None)
def checked(dtype, family, heads, B, H, W, shift):
    """one forward + backward of the case, checked; the forward's and the backward's ragged cases often share a geometry"""
    c = case_of(dtype, family, heads, B, H, W, shift)
    FillRun(c).check(f'{family} {B}x{H}x{W} shift {shift}', chunks_of(dtype, family, True, c.nwin, heads))
    return True


# ================================================================================================ F1
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('side', [8, 16])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_fewer_windows_than_workgroups(family, side, dtype):
    """B = 1, 16 heads, 8 x 8 (one window; shift 0, the only legal one) and 16 x 16 (4 windows, shift 4): 256 * per_cu / (16 L) is
    at least 5, so grid.x is clamped to the window count and every workgroup owns exactly one window -- at 8 x 8 one workgroup per
    (head, band) is the whole launch."""
    nwin = (side // 8) ** 2
    for backward in (False, True):
        assert chunks_of(dtype, family, backward, nwin, 16) == nwin
        assert chunks_of(dtype, family, backward, 1 << 20, 16) > nwin
    assert checked(dtype, family, 16, 1, side, side, 0 if side == 8 else 4)


# ================================================================================================ F2
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shift', [0, 4])
@pytest.mark.parametrize('backward', [False, True], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_ragged_walk_at_the_new_fill(family, backward, shift, dtype):
    """For the kernel (family, forward | backward, dtype): the smallest B x H x W, H != W, whose walk under the grid fw_attn_chunks
    reports leaves a remainder, idles at least one workgroup and holds an image boundary inside a range -- at the kernel's full
    fill (grid.x equals that of an unbounded problem).  All three are asserted here from fw_attn_chunks, so a later change of rule
    cannot hollow the case out.  LFS: the three coefficients differ per image, so a stale (a, b, c) or an unflushed dcoef partial sum
    shows in out / dcoef."""
    D, heads_c, L, mode, lfs = FAMILIES[family]
    heads, B, H, W = choose_ragged(lambda nwin, heads: chunks_of(dtype, family, backward, nwin, heads), heads_c)
    nW = (H // 8) * (W // 8)
    nwin = B * nW
    chunks = chunks_of(dtype, family, backward, nwin, heads)
    per, busy, last, idle = attn_walk(nwin, chunks)
    rem, idle2, crossed = walk_properties(nwin, nW, chunks)
    print(f'{family} {"bwd" if backward else "fwd"} [{str(dtype)[6:]}]: heads {heads}, {B} x {H} x {W}: {nwin} windows in {chunks} ranges of {per}, '
          f'{busy} busy (last {last}), {idle} idle, images begin inside a range at windows {crossed}')
    assert H != W and chunks < nwin and chunks == chunks_of(dtype, family, backward, 1 << 20, heads)
    assert rem != 0 and last < per, 'the last busy workgroup must be short'
    assert idle >= 1 and idle == idle2, 'at least one workgroup must be idle'
    assert crossed, 'an image boundary must lie inside a walk'
    if lfs:
        c = case_of(dtype, family, heads, B, H, W, shift)
        assert len({tuple(c.coef[b].reshape(-1).tolist()) for b in range(B)}) == B
    assert checked(dtype, family, heads, B, H, W, shift)


# ================================================================================================ F3
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('family', ['attn2<28,0>', 'attn2x<28>', 'attn2<56,2>'])
def test_prefilled_gradients_are_accumulated_into_at_a_ragged_grid(family, dtype):
    """include/fwair.h: dbias and dcoef are ACCUMULATED into.  The backward's ragged case (shift 4) with both pre-filled with seeded
    values of the gradient's own rms: the result is pre-fill + gradient within the bound plus one rounding of |pre-fill| per atomic
    addition of the walk; idle workgroups add nothing (their +0.0 would not show, a stray partial sum would); guards, pad columns and
    lse coverage as in every case."""
    D, heads_c, L, mode, lfs = FAMILIES[family]
    heads, B, H, W = choose_ragged(lambda nwin, heads: chunks_of(dtype, family, True, nwin, heads), heads_c)
    c = case_of(dtype, family, heads, B, H, W, 4)
    ref = attn_reference(c)
    g = torch.Generator().manual_seed(19)
    rms = lambda t, dims: (t * t).mean(dims, keepdim=True).sqrt()
    dbias0 = (torch.randn(ref['dbias'][0].shape, generator=g) * rms(ref['dbias'][0], (0, 1, 2))).float()
    dcoef0 = (torch.randn(ref['dcoef'][0].shape, generator=g) * rms(ref['dcoef'][0], (0, 1))).float() if lfs else None
    run = FillRun(c, dbias0, dcoef0)
    run.check(f'F3 {family}', chunks_of(dtype, family, True, c.nwin, heads))
    moved = (run.res['dbias'] - dbias0.double()).abs().max()
    assert float(moved) > 0.1 * float(ref['dbias'][0].abs().max()), 'dbias: the gradient did not arrive on top of the pre-fill'
    # tables no (query band, key band) pair of the mode uses stay exactly the pre-fill
    used = {lq * L + lk for lq in range(L) for lk in c.keys(lq)}
    for t in set(range(L * L)) - used:
        assert torch.equal(run.res['dbias'][t], dbias0[t].double()), f'dbias table {t} belongs to no band pair and was written'
