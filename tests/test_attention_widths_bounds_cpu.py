"""The element-wise bounds of helpers.attn_reference at the head dimensions of the decoder widths 32 and 64
(tests/test_attention_widths_gpu.py holds the kernels to them): the honest emulation of the kernels lies inside, the wrong
kernels of test_window_attention_bounds_cpu.MUTANTS, re-run at D = 32, fall outside at the share that file asks for.

At D = 32 a score is a 32-term contraction (one 64-byte chunk per bf16 row), an output row two 16-row d-tiles; at D = 64 nothing is
padded.  The bound machinery takes D from the case, so nothing here is widened: same constants, same MIN_REJECTED.

No GPU, no library."""
import pytest
import torch

from helpers import attn_emulate, attn_inputs, attn_outputs_flat, attn_reference, attn_walks, walk_crossings
from test_window_attention_bounds_cpu import MIN_REJECTED, MUTANTS, flat, outside

DTYPES = [torch.float32, torch.bfloat16]
WIDTHS = [32, 64]
# D is put in front: (heads, B, H, W, L, mode, shift, lfs)
HONEST = {'decoder lfs 0': (2, 3, 16, 24, 1, 0, 4, 0), 'decoder lfs 1': (2, 3, 16, 24, 1, 0, 4, 1), 'decoder lfs 2': (2, 3, 16, 24, 1, 0, 4, 2),
          'bottleneck lfs 2': (16, 5, 8, 8, 1, 0, 0, 2)}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('std', [None, 35.0])
@pytest.mark.parametrize('name', list(HONEST))
@pytest.mark.parametrize('D', WIDTHS)
def test_honest_emulation_is_inside_the_bounds(D, name, std, dtype):
    c = attn_inputs(dtype, D, *HONEST[name], score_std=std)
    em = attn_emulate(c)
    got = attn_outputs_flat(em)
    # the backward's bounds both ways: from the lse the (emulated) forward handed over, and for an lse anywhere within its bound
    for lse_in in (em['lse'], None):
        val, tol = flat(attn_reference(c, lse_in=lse_in))
        for n in val:
            assert torch.isfinite(got[n]).all()
            bad = outside(got[n], val[n], tol[n])
            ratio = float(((got[n].double() - val[n]).abs() / tol[n]).nan_to_num(0.0).max())
            print(f'D {D} {name} [{str(dtype)[6:]}] score std {std or 1}, {n}: worst error / bound {ratio:.3f}')
            assert not bool(bad.any()), f'D {D} {name} {n}: {int(bad.sum())} of {bad.numel()} elements outside'


@pytest.mark.parametrize('D', WIDTHS)
def test_crossing_case_keeps_its_walks(D):
    """the walk arithmetic has no D in it: the crossing case of the pin file crosses windows 35 and 70 at these widths too"""
    c = attn_inputs(torch.float32, D, 8, 3, 40, 56, 1, 0, 4, 2)
    (_, c1), (_, c2) = attn_walks(c.nwin, c.heads, 1, False)
    assert walk_crossings(c.nwin, c1, c.nW) == [35, 70] and walk_crossings(c.nwin, c2, c.nW) == [35]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mutation', list(MUTANTS))
def test_bounds_reject_the_wrong_kernels_at_32(dtype, mutation):
    """MUTANTS of the D = 56 file with the head dimension replaced by 32: same geometry, lfs, score std, lambda scale, outputs and share"""
    geo, lfs, std, lam_scale, affected = MUTANTS[mutation]
    c = attn_inputs(dtype, 32, *geo[1:], lfs, score_std=std, lam_scale=lam_scale)
    got = attn_outputs_flat(attn_emulate(c))
    val, tol = flat(attn_reference(c, mutation=mutation))
    if mutation == 'dcoef_first_image':
        per, chunks = attn_walks(c.nwin, c.heads, 1, False)[0]
        assert walk_crossings(c.nwin, chunks, c.nW) == [35, 70]
    for n in affected:
        share = float(outside(got[n], val[n], tol[n]).double().mean())
        print(f'{mutation} D 32 [{str(dtype)[6:]}] {n}: rejected at {share:.4f} of the elements')
        assert share >= MIN_REJECTED, f'{mutation} {n}: the bound rejects only {share:.4f} of the elements'
