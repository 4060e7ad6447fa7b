"""Window attention (csrc/fw_attn.hip) at the head dimensions of the decoder widths 32 and 64: attn2_fwd_kernel / attn2_bwd_kernel
<T, 32, lfs> and <T, 64, lfs>, lfs 0 / 1 / 2, through the C ABI as tests/test_window_attention_pin_gpu.py does it (q | k | v rows of
stride 3C + 8 with NaN pads, every output between guard words).  Every output is held to the element-wise bounds of
helpers.attn_reference (proven for these D by test_attention_widths_bounds_cpu.py), to the rel-to-max limits of test_ops_gpu.TOL and
to check_untouched.  Before the dispatch took these forms every case here ended in code -1000.

What is new against D = 56 / 28: Geo<T, 32> has one 64-byte chunk per bf16 row (KC 1; f32: 2), two 16-row d-tiles (DT 2), no padding
granule and ONE TileLoad round per tile; Geo<T, 64> has CH == SL (nothing to zero-pad) next to the LFS scratch.

Workgroups per CU.  fwd2_launch / bwd2_launch take per_cu = 2 where 2 * Smem2 bytes <= 160 KB, and the grid -- hence the walk -- follows:
  LDR = KB + 16, KB = D * SZ rounded up to 64;  TILE_D = 64 * LDR;  SCR = max(2 * 64 * (32 SZ + 16), 64 * (64 SZ + 16));
  TAB = lfs 2 ? 160 * (64 SZ + 16) + 6144 : 0;  RA = max(SCR, TILE_D);  NTF = (lfs 2 and bf16) ? 2 : 1;
  FWD = TAB + 1024 + 2 RA + TILE_D;   BWD = TAB + 1024 + 4 TILE_D + 2 NTF SCR.
                      TILE_D    SCR     TAB     FWD lfs 0/1  BWD lfs 0/1   FWD lfs 2   BWD lfs 2
  D 32 bf16            5 120  10 240  29 184      26 624 (2)   41 984 (2)   55 808 (2)   91 648 (1)
  D 32 f32             9 216  18 432  49 664      47 104 (2)   74 752 (2)   96 768 (1)  124 416 (1)
  D 64 bf16            9 216  10 240  29 184      30 720 (2)   58 368 (2)   59 904 (2)  108 032 (1)
  D 64 f32            17 408  18 432  49 664      55 296 (2)  107 520 (1)  104 960 (1)  157 184 (1)
(per_cu in brackets; 2 * 81 920 = 163 840 is the limit.)  D = 56 has the D = 64 row: the padding granule is inside KB.  smem2_bytes()
below is that arithmetic, held to the table; the crossing case asserts the walk of the per_cu of its own (D, dtype, lfs, direction)."""

import pytest
import torch

from helpers import attn2_chunks, attn_inputs, attn_reference, attn_walk, walk_crossings
from test_window_attention_pin_gpu import Run, assert_v2_walk

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
WIDTHS = [32, 64]
DECODER = (2, 3, 16, 24, 1, 0, 4)                     # heads, B, H, W, L, mode, shift: 6 windows per image, 18 in all, shifted
CROSSING = (8, 3, 40, 56, 1, 0, 4)                    # 35 windows per image, 105 in all
BOTTLENECK = (16, 5, 8, 8, 1, 0, 0)                   # every window its own image

BYTES = {   # (D, bf16?) -> ((fwd, bwd) at lfs 0 / 1, (fwd, bwd) at lfs 2)
    (32, True): ((26624, 41984), (55808, 91648)), (32, False): ((47104, 74752), (96768, 124416)),
    (64, True): ((30720, 58368), (59904, 108032)), (64, False): ((55296, 107520), (104960, 157184)),
}


def smem2_bytes(D, dtype, lfs):
    """(FWD_BYTES, BWD_BYTES) of Smem2<T, D, lfs>"""
    sz = 2 if dtype == torch.bfloat16 else 4
    tile = 64 * (-(-D * sz // 64) * 64 + 16)
    ldp, ldv = 64 * sz + 16, 32 * sz + 16
    scr = max(2 * 64 * ldv, 64 * ldp)
    tab = 160 * ldp + 48 * 32 * 4 if lfs == 2 else 0
    ra, ntf = max(scr, tile), 2 if lfs == 2 and sz == 2 else 1
    return tab + 1024 + 2 * ra + tile, tab + 1024 + 4 * tile + 2 * ntf * scr


def per_cu(D, dtype, lfs):
    """(forward, backward) workgroups per CU the launches size their grids for"""
    return tuple(2 if 2 * b <= 160 * 1024 else 1 for b in smem2_bytes(D, dtype, lfs))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', WIDTHS)
def test_lds_bytes_and_workgroups_per_cu(D, dtype):
    bf = dtype == torch.bfloat16
    assert (smem2_bytes(D, dtype, 0), smem2_bytes(D, dtype, 2)) == BYTES[(D, bf)] and smem2_bytes(D, dtype, 1) == smem2_bytes(D, dtype, 0)
    assert max(smem2_bytes(D, dtype, 2)) <= 160 * 1024                                    # every form fits the CU's LDS
    want = {(32, True): ((2, 2), (2, 1)), (32, False): ((2, 2), (1, 1)), (64, True): ((2, 2), (2, 1)), (64, False): ((2, 1), (1, 1))}
    assert (per_cu(D, dtype, 1), per_cu(D, dtype, 2)) == want[(D, bf)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lfs', [0, 1, 2])
@pytest.mark.parametrize('D', WIDTHS)
def test_shifted_windows(D, lfs, dtype):
    """2 heads, B 3, 16 x 24, shift 4: the last window row / column carry the -100 mask; one window per workgroup"""
    c = attn_inputs(dtype, D, *DECODER, lfs)
    assert c.nW == 6 and c.nwin == 18
    assert_v2_walk(c, {1: (18, 1, 18, 1, 0), 2: (18, 1, 18, 1, 0)})
    Run(c).check(f'W1 D {D} lfs {lfs}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lfs', [1, 2])
@pytest.mark.parametrize('D', WIDTHS)
def test_walk_crosses_an_image_with_lfs(D, lfs, dtype):
    """8 heads, B 3, 40 x 56, shift 4, coefficients differ per image.  per_cu 1: 32 chunks of 4 windows, windows 35 and 70 inside a walk;
    per_cu 2: 64 chunks of 2, window 35 inside a walk.  Forward and backward may differ (table above): each direction's walk is asserted
    for the per_cu its launch takes."""
    c = attn_inputs(dtype, D, *CROSSING, lfs)
    assert c.nW == 35 and c.nwin == 105
    walks = {1: (32, 4, 27, 1, 5), 2: (64, 2, 53, 1, 11)}
    crossed = {1: [35, 70], 2: [35]}
    for direction, p in zip(('fwd', 'bwd'), per_cu(D, dtype, lfs)):
        assert_v2_walk(c, {p: walks[p]})
        assert walk_crossings(c.nwin, attn2_chunks(c.nwin, c.heads, 1, p), c.nW) == crossed[p], direction
    assert len({tuple(c.coef[b].reshape(-1).tolist()) for b in range(3)}) == 3
    Run(c).check(f'W2 D {D} lfs {lfs}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lfs', [0, 2])
@pytest.mark.parametrize('D', WIDTHS)
def test_bottleneck_geometry(D, lfs, dtype):
    """H = W = 8, 16 heads (C 512 / 1024), B 5: the image changes with every window"""
    c = attn_inputs(dtype, D, *BOTTLENECK, lfs)
    assert c.nW == 1 and c.nwin == 5
    for p in set(per_cu(D, dtype, lfs)):
        assert (attn2_chunks(c.nwin, 16, 1, p),) + attn_walk(c.nwin, attn2_chunks(c.nwin, 16, 1, p)) == (5, 1, 5, 1, 0)
    Run(c).check(f'W3 D {D} lfs {lfs}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', WIDTHS)
def test_large_scores(D, dtype):
    """scores of standard deviation 35 with the band filter on: the running max, exp(s - lse) in the backward, the literal -100"""
    c = attn_inputs(dtype, D, *DECODER, 2, score_std=35.0)
    Run(c).check(f'W4 D {D}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', WIDTHS)
def test_gradient_buffers_are_accumulated_into(D, dtype):
    """dbias and dcoef pre-filled with seeded values of the gradient's own magnitude: the result is pre-fill + gradient"""
    c = attn_inputs(dtype, D, *DECODER, 2)
    ref = attn_reference(c)
    g = torch.Generator().manual_seed(11)
    rms = lambda t, dims: (t * t).mean(dims, keepdim=True).sqrt()
    dbias0 = (torch.randn(ref['dbias'][0].shape, generator=g) * rms(ref['dbias'][0], (0, 1, 2))).float()
    dcoef0 = (torch.randn(ref['dcoef'][0].shape, generator=g) * rms(ref['dcoef'][0], (0, 1))).float()
    run = Run(c, dbias0, dcoef0)
    run.check(f'W5 D {D}')
    moved = (run.res['dbias'] - dbias0.double()).abs().max()
    assert float(moved) > 0.1 * float(ref['dbias'][0].abs().max()), 'dbias: the gradient did not arrive on top of the pre-fill'
