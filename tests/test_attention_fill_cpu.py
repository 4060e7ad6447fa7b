"""Host side of the window-attention fill (csrc/fw_attn.hip: grid.x = 256 * resident workgroups per CU / (heads * L)): the C ABI declares
fw_attn_chunks in both headers, and the geometries test_attention_fill_gpu.py takes from it stay ragged whatever the GPU box reports."""

import os
import re

import pytest

from attn_fill_cases import CANDIDATES, FAMILIES, MAX_NWIN, choose_ragged, is_ragged, model_grid, walk_properties
from helpers import attn_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd')
DECL = (r'\bint\s+fw_attn_chunks\s*\(\s*int\s+dtype\s*,\s*int\s+D\s*,\s*int\s+nkt\s*,\s*int\s+lfs\s*,\s*int\s+backward\s*,\s*int\s+nwin\s*,'
        r'\s*int\s+heads\s*,\s*int\s+L\s*\)\s*;')


def test_fw_attn_chunks_is_declared_in_both_headers():
    """include/fwair.h and the copy the package parses its prototypes from (build.sh makes it) declare the same entry, and the
    loader binds it with eight int arguments"""
    from fwair import lib
    paths = [os.path.join(ROOT, 'include', 'fwair.h'), os.path.join(PKG, 'fwair', 'fwair.h')]
    assert os.path.exists(paths[1]), 'the packaged header is missing: run build.sh'
    for p in paths:
        assert len(re.findall(DECL, open(p).read())) == 1, p
    sig = lib.parse_header(paths[1])['fw_attn_chunks']
    assert len(sig) == 8 and not any(isptr for _, isptr in sig)
    assert hasattr(lib.lib(), 'fw_attn_chunks')


@pytest.mark.parametrize('backward', [False, True])
@pytest.mark.parametrize('per_cu', range(1, 9))
@pytest.mark.parametrize('family', list(FAMILIES))
def test_a_ragged_geometry_exists_for_every_fill(family, per_cu, backward):
    """whatever the occupancy query answers (1 .. 8 workgroups per CU; the smallest LDS footprint admits 6), the chooser finds a case
    with H != W, both >= 16, launched at the full fill, whose walk leaves a remainder, idles a workgroup and crosses an image -- of
    at most MAX_NWIN windows, except for a backward kernel over one band at three or more workgroups per CU (its walk floor asks for
    4 windows in each of 16 * per_cu ranges; only the D = 32 decoder form can be one, and the GPU test has no such case)"""
    D, heads_c, L, mode, lfs = FAMILIES[family]
    grid = model_grid(L, per_cu, backward)
    limit = 648 if backward and L == 1 and per_cu >= 3 else MAX_NWIN
    heads, B, H, W = choose_ragged(grid, heads_c, limit)
    nW = (H // 8) * (W // 8)
    nwin = B * nW
    assert H != W and H >= 16 and W >= 16 and H % 8 == 0 and W % 8 == 0 and B >= 2 and nwin <= limit
    chunks = grid(nwin, heads)
    assert chunks == 256 * per_cu // (heads * L) < nwin                                   # the full fill, not clamped, not floored
    rem, idle, crossed = walk_properties(nwin, nW, chunks)
    per, busy, last, idle2 = attn_walk(nwin, chunks)
    assert rem != 0 and last == rem and last < per                                       # a short last walk
    assert idle == idle2 >= 1 and busy + idle == chunks and busy * per >= nwin > (busy - 1) * per
    assert crossed and all(w % nW == 0 and w % per != 0 for w in crossed)                # first window of an image inside a range
    assert per >= 2 and (not backward or per_cu <= 2 or per >= 4)


def test_properties_are_not_vacuous():
    """is_ragged says no where one property fails, yes where all three hold"""
    assert walk_properties(64, 16, 16) == (0, 0, []) and not is_ragged(64, 16, 16)          # 4 each: exact, full, aligned
    assert walk_properties(45, 15, 45) == (0, 0, []) and not is_ragged(45, 15, 45)          # one window per workgroup
    assert walk_properties(45, 15, 10) == (0, 1, []) and not is_ragged(45, 15, 10)          # idle alone is not enough
    assert walk_properties(42, 21, 16) == (0, 2, []) and not is_ragged(42, 21, 16)
    assert walk_properties(42, 21, 10) == (2, 1, [21]) and is_ragged(42, 21, 10)            # 5 each, 9 busy, window 21 = 4 * 5 + 1
    assert walk_properties(40, 20, 16) == (1, 2, [20]) and is_ragged(40, 20, 16)
    assert all(H != W for _, _, H, W in CANDIDATES)
