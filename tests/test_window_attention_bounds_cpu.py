"""The element-wise bounds of tests/test_window_attention_pin_gpu.py (helpers.attn_reference), proven on the host:

  * the f64 reference is the operation test_ops_gpu.ref_window_attention states (values and autograd gradients);
  * the one measured constant, the band filter's own rounding error, is re-measured from the reference alone and printed;
  * an honest emulation of the kernels (f32 arithmetic, the operand type's rounding where the kernels round, the emulated filter)
    has no element outside the bounds -- forward and backward, lfs 0 / 1 / 2, intra and inter band, ordinary and large scores;
  * the wrong kernels the bounds exist to catch are rejected: the share of the elements of each affected output at which the bound
    of the WRONG reference rejects the honest emulation is printed and asserted.

No GPU, no library."""
import pytest
import torch

from helpers import (ATTN_FILTER_MARGIN, ATTN_FILTER_RMS, ATTN_FILTER_SIGMAS, WAttnCase, _attn_band, attn_emulate, attn_filter_emulated,
                     attn_filter_f64, attn_inputs, attn_outputs_flat, attn_reference, attn_walks, walk_crossings)
from test_ops_gpu import lam_to_coef, ref_window_attention, rnd

DTYPES = [torch.float32, torch.bfloat16]
DECODER = (56, 2, 3, 16, 24, 1, 0, 4)                 # D, heads, B, H, W, L, mode, shift: 6 windows per image, 18 in all
CROSSING = (56, 8, 3, 40, 56, 1, 0, 4)                # case B1 of the GPU file: walks of 4 (or 2) windows cross windows 35 and 70
MIN_REJECTED = 0.02


def flat(ref):
    return attn_outputs_flat({n: v for n, (v, _) in ref.items()}), attn_outputs_flat({n: t for n, (_, t) in ref.items()})


def outside(y, value, tol):
    return ~((y.double() - value).abs() <= tol)


# ------------------------------------------------------------------------------------------------ the reference is the operation
@pytest.mark.parametrize('L,mode,lfs', [(1, 0, 0), (1, 0, 1), (1, 0, 2), (3, 0, 0), (3, 1, 0), (2, 1, 0)])
def test_reference_is_the_oracle_operation(L, mode, lfs):
    B, H, W, heads, shift = 2, 16, 24, 2, 4
    D = 56 if L == 1 else 28
    C, nb = D * heads, {0: 0, 1: 2, 2: 3}[lfs]
    qkv = rnd(L * B * H * W, 3 * C).double().requires_grad_(True)
    tables = (rnd(L * L, 225, heads, seed=1) * 0.5).double().requires_grad_(True)
    lam = (rnd(B, nb - 1, heads, seed=2) * 0.3).double().requires_grad_(True) if lfs else None
    dout = rnd(L * B * H * W, C, seed=3).double()
    ref = ref_window_attention(qkv, C, B, H, W, heads, L, mode, shift, tables, lam, nb)
    ref.backward(dout)
    coef = lam_to_coef(lam, nb).detach() if lfs else None                       # kept in f64: no storage rounding in this comparison
    c = WAttnCase(torch.float32, D, heads, B, H, W, L, mode, shift, lfs, qkv.detach(), dout, tables.detach(), coef)
    c.scale = float(D) ** -0.5
    got = {n: v for n, (v, _) in attn_reference(c, v1=(L == 2)).items()}

    def scatter(win):                                                           # [L, nwin, heads, 64, D] -> [rows, C]
        m = torch.zeros(L * B * H * W, C, dtype=torch.float64)
        m[c.rows.reshape(-1)] = win.transpose(2, 3).reshape(-1, C)
        return m
    assert (scatter(got['out']) - ref.detach()).abs().max() < 1e-12
    dk, dv = torch.zeros_like(got['dq']), torch.zeros_like(got['dq'])
    for lq in range(L):
        for kt, lk in enumerate(c.keys(lq)):
            dk[lk] += got['dk'][lq][kt]
            dv[lk] += got['dv'][lq][kt]
    grad = torch.cat([scatter(got['dq']), scatter(dk), scatter(dv)], 1)
    assert (grad - qkv.grad).abs().max() < 1e-11
    assert (got['dbias'] - tables.grad).abs().max() < 1e-10
    if lfs:
        want = lam.grad.clone()
        lam.grad = None
        (lam_to_coef(lam, nb) * got['dcoef']).sum().backward()
        assert (lam.grad - want).abs().max() < 1e-10


# ------------------------------------------------------------------------------------------------ the measured constant
@pytest.mark.parametrize('dtype', DTYPES)
def test_filter_allowance_is_the_measured_one(dtype):
    """helpers.ATTN_FILTER_RMS: the largest rms of the emulated filter's error over one row or one column of a map, relative to
    max |x| of the map, on P and dP' of these tests' inputs; and the error has no mean to speak of (the contraction argument)."""
    exact, _ = attn_filter_f64()
    emulated = attn_filter_emulated(dtype)
    worst = 0.0
    for std in (None, 4.0, 35.0):
        c = attn_inputs(dtype, *DECODER, 2, score_std=std)
        r = _attn_band(c, 0, torch.float64, lambda t: t, exact, None, None, attn_walks(c.nwin, c.heads, 1, False))
        for name in ('P', 'dPp'):
            x = r[name]
            e = emulated(x) - exact(x)
            rms = torch.maximum((e * e).mean(-1).sqrt().amax(-1), (e * e).mean(-2).sqrt().amax(-1)) / x.abs().amax((-1, -2))
            mean = e.mean((-1, -2)).abs() / (e * e).mean((-1, -2)).sqrt()
            print(f'filter error [{str(dtype)[6:]}] score std {std or 1}, {name}: rms / max|x| {float(rms.max()):.3e}, '
                  f'largest |error| / max|x| {float((e.abs().amax((-1, -2)) / x.abs().amax((-1, -2))).max()):.3e}, '
                  f'|mean| / rms {float(mean.max()):.3e}')
            worst = max(worst, float(rms.max()))
            assert float(mean.max()) < 0.05
    print(f'filter error [{str(dtype)[6:]}]: measured {worst:.3e}, constant {ATTN_FILTER_RMS[dtype]:.1e}, allowance '
          f'{ATTN_FILTER_SIGMAS:g} x {ATTN_FILTER_MARGIN:g} x that per contraction')
    slack = 1.5 if dtype == torch.bfloat16 else 4.0           # f32: the figure moves with the host BLAS's order of accumulation
    assert ATTN_FILTER_RMS[dtype] / slack <= worst <= ATTN_FILTER_RMS[dtype], 'the constant is the measured figure, not a wider one'


# ------------------------------------------------------------------------------------------------ the honest kernel stays inside
HONEST = {'decoder lfs 0': DECODER + (0,), 'decoder lfs 1': DECODER + (1,), 'decoder lfs 2': DECODER + (2,),
          'intra L 3': (28, 2, 2, 16, 24, 3, 0, 4, 0), 'inter L 3': (28, 2, 2, 16, 24, 3, 1, 4, 0), 'inter L 2': (28, 2, 2, 16, 24, 2, 1, 4, 0),
          'bottleneck lfs 2': (56, 16, 5, 8, 8, 1, 0, 0, 2)}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('std', [None, 35.0])
@pytest.mark.parametrize('name', list(HONEST))
def test_honest_emulation_is_inside_the_bounds(dtype, name, std):
    c = attn_inputs(dtype, *HONEST[name], score_std=std)
    em = attn_emulate(c)
    got = attn_outputs_flat(em)
    # the backward's bounds both ways: from the lse the (emulated) forward handed over, and for an lse anywhere within its bound
    for lse_in in (em['lse'], None):
        val, tol = flat(attn_reference(c, lse_in=lse_in, v1=name == 'inter L 2'))
        for n in val:
            assert torch.isfinite(got[n]).all()
            bad = outside(got[n], val[n], tol[n])
            ratio = float(((got[n].double() - val[n]).abs() / tol[n]).nan_to_num(0.0).max())
            print(f'{name} [{str(dtype)[6:]}] score std {std or 1}, {n}: worst error / bound {ratio:.3f}')
            assert not bool(bad.any()), f'{name} {n}: {int(bad.sum())} of {bad.numel()} elements outside'


# ------------------------------------------------------------------------------------------------ the wrong kernels fall outside
# mutation -> (geometry, lfs, score std, lambda scale, affected outputs).  Inputs are strengthened where the honest bf16 rounding
# would hide the defect: a filter term 10 % short needs peaked maps (score std 4) and |lambda| ~ 1 to stand clear of 2^-8 |P'|.
MUTANTS = {
    'bias_swapped': (DECODER, 2, None, 0.3, ('out', 'lse', 'dq', 'dk', 'dv', 'dbias')),
    'drop_key63': (DECODER, 2, None, 0.3, ('out', 'lse', 'dq', 'dk', 'dv', 'dbias')),
    'no_const': (DECODER, 2, None, 0.3, ('out', 'dv')),
    'filter_09': (DECODER, 2, 4.0, 1.0, ('out', 'dq', 'dk', 'dv')),
    'dcoef_first_image': (CROSSING, 2, None, 0.3, ('dcoef',)),
    'mask50': ((56, 2, 2, 16, 24, 1, 0, 4), 0, 35.0, 0.3, ('out', 'lse', 'dq', 'dk', 'dv')),
}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mutation', list(MUTANTS))
def test_bounds_reject_the_wrong_kernels(dtype, mutation):
    geo, lfs, std, lam_scale, affected = MUTANTS[mutation]
    c = attn_inputs(dtype, *geo, lfs, score_std=std, lam_scale=lam_scale)
    got = attn_outputs_flat(attn_emulate(c))
    val, tol = flat(attn_reference(c, mutation=mutation))
    if mutation == 'dcoef_first_image':
        per, chunks = attn_walks(c.nwin, c.heads, 1, False)[0]
        assert walk_crossings(c.nwin, chunks, c.nW) == [35, 70]
    for n in affected:
        share = float(outside(got[n], val[n], tol[n]).double().mean())
        print(f'{mutation} [{str(dtype)[6:]}] {n}: rejected at {share:.4f} of the elements')
        assert share >= MIN_REJECTED, f'{mutation} {n}: the bound rejects only {share:.4f} of the elements'


@pytest.mark.parametrize('dtype', DTYPES)
def test_bounds_reject_stale_coefficients_in_the_first_window_of_an_image(dtype):
    """the first window of every image b > 0 computed with image b - 1's (a, b, c): rejected at half the elements of THOSE windows"""
    c = attn_inputs(dtype, *DECODER, 2)
    em = attn_emulate(c)
    ref = attn_reference(c, mutation='stale_coef')
    first = torch.arange(c.nW, c.nwin, c.nW)
    for n in ('out', 'dq'):
        bad = outside(em[n][:, first], ref[n][0][:, first], ref[n][1][:, first])
        share = float(bad.double().mean())
        print(f'stale_coef [{str(dtype)[6:]}] {n}: rejected at {share:.4f} of the elements of windows {first.tolist()}')
        assert share >= 0.5
