"""Geometries for the window-attention fill tests (test_attention_fill_gpu.py, test_attention_fill_cpu.py).

The v2 kernels' grid is 256 * per_cu / (heads * L) window ranges per (head, band), per_cu being what the runtime reports for the compiled
kernel (fw_attn_chunks), so no fixed geometry keeps a ragged walk ragged under every fill.  choose_ragged() therefore picks the
geometry FROM the grid function: the smallest B x H x W (H != W, both >= 16 so that shift 4 is legal) at which
  (1) nwin leaves a remainder: the last busy workgroup walks fewer windows than the others,
  (2) at least one workgroup is idle (its range starts at or behind nwin),
  (3) an image boundary falls inside some workgroup's range (LFS: (a, b, c) re-read, dcoef flushed in mid-walk).
The CPU test proves that it finds one, of bounded size, for every per_cu from 1 to 8 and for the backward's walk floor."""

from helpers import attn2_chunks, attn_walk, walk_crossings

# kernel family -> (D, heads candidates, L, mode, lfs): the encoder's intra-band and inter-band forms and the decoder's LFS form
FAMILIES = {'attn2<28,0>': (28, (16, 8), 3, 0, 0), 'attn2x<28>': (28, (16, 8), 3, 1, 0), 'attn2<56,2>': (56, (16,), 1, 0, 2)}
MAX_NWIN = 135                                       # no chosen case is larger (asserted on the host for per_cu 1 .. 8)
BWD_MIN_WALK = 4                                     # csrc/fw_attn.hip: the backward's third workgroup per CU needs walks of 4 windows

CANDIDATES = sorted((B * h * w, B, 8 * h, 8 * w) for B in range(2, 10) for h in range(2, 10) for w in range(2, 10) if h != w)


def walk_properties(nwin, nW, chunks):
    """-> (remainder, idle workgroups, image boundaries inside a walk) of `chunks` ranges over nwin windows, nW per image"""
    per, busy, last, idle = attn_walk(nwin, chunks)
    return nwin % per, idle, walk_crossings(nwin, chunks, nW)


def is_ragged(nwin, nW, chunks):
    rem, idle, crossed = walk_properties(nwin, nW, chunks)
    return rem != 0 and idle >= 1 and len(crossed) > 0


def choose_ragged(grid, heads_candidates, max_nwin=None):
    """grid(nwin, heads) -> grid.x.  -> (heads, B, H, W) of the smallest candidate that is ragged under it AND launched at the
    kernel's full fill: grid.x is what an unbounded problem gets (256 * per_cu / (heads * L)), neither clamped to nwin nor held back
    by the backward's walk floor -- so the case runs the grid the occupancy query asked for, not the old one."""
    for heads in heads_candidates:
        full = grid(1 << 20, heads)
        for nwin, B, H, W in CANDIDATES:
            if nwin <= (max_nwin or MAX_NWIN) and grid(nwin, heads) == full and is_ragged(nwin, nwin // B, full):
                return heads, B, H, W
    raise AssertionError('no ragged geometry up to %d windows for this grid rule' % (max_nwin or MAX_NWIN))


def model_grid(L, per_cu, backward):
    """the launch rule of csrc/fw_attn.hip for a kernel of which a CU holds per_cu workgroups"""
    def grid(nwin, heads):
        chunks = attn2_chunks(nwin, heads, L, per_cu)
        if backward and per_cu > 2 and -(-nwin // chunks) < BWD_MIN_WALK:
            chunks = attn2_chunks(nwin, heads, L, 2)
        return chunks
    return grid
