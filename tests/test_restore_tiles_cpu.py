"""Host side of restoring images of any size (fwair/evaluate.py plan_tiles_ex, restore.py's flags) and the numpy restatement of
fw_restore_gather / fw_restore_blend the GPU tests compare with (tests/restore_cases.py), checked against numpy's own padding,
rotations and brute force.  No GPU."""
import sys

import numpy as np
import pytest

import data_oracle as D
import restore_cases as RC

T = RC.T


def test_reflection_rule_is_numpy_reflect_padding():
    """R continues np.pad(mode='reflect') to every pad width ('edge' at size 1): sizes 1 .. T + 3, pads up to 2 T"""
    for n in range(1, T + 4):
        a = np.arange(n) * 3 + 1
        for pad in range(0, 2 * T + 1):
            ref = np.pad(a, (pad, pad), mode='reflect' if n > 1 else 'edge')
            idx = RC.reflect(np.arange(-pad, n + pad), n)
            assert idx.min() >= 0 and idx.max() < n
            assert np.array_equal(a[idx], ref), (n, pad)


def test_mode_maps_are_the_reference_flips_and_rotations():
    """tile = x[preimage] is np.flipud(np.rot90(x, k)) in image_utils' order (flipud last), and the stated inverse undoes it"""
    x = np.random.RandomState(0).randn(T, T)
    seen = set()
    for mode in range(8):
        PY, PX = RC.preimage(mode, T)
        tile = x[PY, PX]
        ref = np.rot90(x, mode >> 1)
        ref = np.flipud(ref) if mode & 1 else ref
        assert np.array_equal(tile, ref), mode
        assert np.array_equal(tile, D.data_augmentation(x[:, :, None], mode)[:, :, 0]), mode
        assert np.array_equal(tile, RC.turn(x, mode)), mode
        OY, OX = RC.image(mode, T)
        assert np.array_equal(tile[OY, OX], x), mode                              # inverse after map
        assert np.array_equal(OY[PY, PX], np.mgrid[0:T, 0:T][0]) and np.array_equal(OX[PY, PX], np.mgrid[0:T, 0:T][1]), mode
        seen.add(tile.tobytes())
    assert len(seen) == 8, 'the eight turns of a generic tile differ'


@pytest.mark.parametrize('overlap', [0, 4, 5, 8])
def test_origins_against_brute_force(overlap):
    """sizes 1 .. 70 at T = 16: every pixel covered, by at most three tiles, no origin twice, every tile inside the padded image, and
    the tiles fw_restore_blend looks at for a pixel are exactly those that cover it"""
    from fwair.evaluate import tile_origins, tile_origins_ex
    stride = T - overlap
    for size in range(1, 71):
        o = tile_origins_ex(size, T, overlap, pad_small=True)
        assert o == RC.origins(size, T, overlap)
        P = max(size, T)
        assert len(set(o)) == len(o) and o == sorted(o) and o[0] == 0 and o[-1] == P - T
        assert o[:-1] == [a * stride for a in range(len(o) - 1)]
        if overlap == 0 and size >= T:
            assert o == tile_origins(size, T)
        for y in range(size):
            cover = [a for a, y0 in enumerate(o) if y0 <= y < y0 + T]
            assert 1 <= len(cover) <= 3, (size, y, cover)
            cand = RC.candidates(y, len(o), stride, T)
            assert cand == sorted(set(cand)) and len(cand) <= 3
            assert [a for a in cand if o[a] <= y < o[a] + T] == cover, (size, y)
        if size < T:
            with pytest.raises(AssertionError, match='invalid test image size'):
                tile_origins_ex(size, T, overlap)


def test_plan_tiles_ex_tables_and_chunks():
    from fwair.evaluate import plan_tiles, plan_tiles_ex
    big = [(17, 40), (50, 23), (16, 33), (16, 16), (70, 70)]
    # overlap 0, one mode: plan_tiles row for row
    for cap in (64, 25):
        t0, g0, c0 = plan_tiles(big, T, cap)
        t1, g1, c1 = plan_tiles_ex(big, T, cap, 0, 1, False)
        assert t1.dtype == np.int32 and g1.dtype == np.int64 and g1.shape == (len(big), 8)
        assert np.array_equal(t0, t1) and np.array_equal(g0, g1[:, :4]) and c0 == c1
        assert (g1[:, 4] == T).all() and (g1[:, 5] == 1).all() and (g1[:, 6:] == 0).all()
    sizes = RC.SIZES + [(70, 3)]
    for overlap in (0, 4, 5, 8):
        for nmodes in (1, 8):
            per = [len(RC.origins(h, T, overlap)) * len(RC.origins(w, T, overlap)) * nmodes for h, w in sizes]
            for cap in (sum(per), max(per), max(per) + 8):
                ttab, gtab, chunks = plan_tiles_ex(sizes, T, cap, overlap, nmodes, True)
                assert ttab.tolist() == [list(r) for r in RC.plan(sizes, T, overlap, nmodes)]
                assert chunks[0][0] == 0 and chunks[0][2] == 0 and chunks[-1][1] == len(sizes) and chunks[-1][3] == len(ttab)
                for (i0, i1, a, b), nxt in zip(chunks, chunks[1:] + [None]):
                    assert i1 > i0 and 0 < b - a <= cap and b - a == sum(per[i0:i1])          # whole images, within the buffer
                    if nxt is not None:
                        assert nxt[0] == i1 and nxt[2] == b
                        assert b - a + per[i1] > cap, 'a chunk closes only when the next image does not fit'
                    off = 0
                    for i in range(i0, i1):
                        h, w = sizes[i]
                        ny, nx = len(RC.origins(h, T, overlap)), len(RC.origins(w, T, overlap))
                        assert gtab[i].tolist() == [off, sum(per[i0:i]), ny, nx, T - overlap, nmodes, 0, 0]
                        first = a + int(gtab[i, 1])
                        for ai, y in enumerate(RC.origins(h, T, overlap)):                      # tile (a, b, m) = first + (a nx + b) nmodes + m
                            for bi, x in enumerate(RC.origins(w, T, overlap)):
                                for m in range(nmodes):
                                    assert ttab[first + (ai * nx + bi) * nmodes + m].tolist() == [i, y, x, m]
                        off += 3 * h * w
            with pytest.raises(ValueError, match='the tile buffer holds'):
                plan_tiles_ex(sizes, T, max(per) - 1, overlap, nmodes, True)
    with pytest.raises(AssertionError, match='invalid test image size'):
        plan_tiles_ex(sizes, T, 4096, 0, 1, False)


def test_eval_engine_refuses_an_overlap_beyond_half_a_tile():
    from fwair.evaluate import EvalEngine
    for bad in (-1, T // 2 + 1, T):
        with pytest.raises(ValueError, match='overlap'):
            EvalEngine(None, tile=T, overlap=bad)


def test_weights_positive_and_symmetric():
    for tile, ramps in ((T, range(1, T // 2 + 1)), (128, (1, 32, 64))):
        for ramp in ramps:
            w = RC.weights(tile, ramp)
            assert w.dtype == np.float32 and (w > 0).all() and w.max() == 1.0
            assert np.array_equal(w, w[::-1]), 'w1(i) = w1(T - 1 - i): the weight is the same in every mode'
            assert w[0] == np.float32(1.0) / np.float32(ramp) and (w[ramp - 1:tile - ramp + 1] == 1.0).all()
            if ramp == 1:
                assert (w == 1.0).all(), 'ramp 1 is the plain mean'


@pytest.mark.parametrize('overlap', RC.OVERLAPS)
@pytest.mark.parametrize('nmodes', [1, 8])
def test_restatement_restores_the_input_under_an_identity_network(overlap, nmodes):
    """gather, identity, blend in numpy: the image comes back within the bound for every size, which pins the restatement's own maps
    (a wrong inverse or a weight in the tile's frame would not return the image where it is reflected)"""
    imgs = RC.images(3, RC.SIZES)
    rows = RC.plan(RC.SIZES, T, overlap, nmodes)
    for i, (H, W) in enumerate(RC.SIZES):
        x = RC.unit(imgs[i])
        out, K, vmax = RC.restore(x, [r for r in rows if r[0] == i], H, W, T, max(overlap, 1), lambda t: t)
        assert K.min() >= nmodes and K.max() <= 9 * nmodes
        assert (np.abs(out - x) <= RC.blend_bound(K, vmax)).all()
        assert np.array_equal(vmax, x)


def test_restore_flags(monkeypatch):
    """restore.py: --tile_overlap, --self_ensemble, --keep_size, all off by default"""
    def parsed(extra):
        monkeypatch.setattr(sys, 'argv', ['restore.py', '--degradation_embedding_method', 'all_3_bands'] + extra)
        for name in ('restore', 'option'):
            sys.modules.pop(name, None)
        try:
            import restore
            return restore._ARGS, list(sys.argv)
        finally:
            for name in ('restore', 'option'):
                sys.modules.pop(name, None)

    a, argv = parsed([])
    assert (a.tile_overlap, a.self_ensemble, a.keep_size) == (0, False, False)
    a, argv = parsed(['--tile_overlap', '32', '--self_ensemble', '--keep_size', '--input', 'x.png', '--output', 'out'])
    assert (a.tile_overlap, a.self_ensemble, a.keep_size, a.input, a.output) == (32, True, True, 'x.png', 'out')
    assert argv[1:] == ['--degradation_embedding_method', 'all_3_bands'], 'the flags are taken off the command line option.py parses'


def test_load_u8_keeps_the_size_on_request(tmp_path):
    from PIL import Image
    from fwair.data import load_u8
    arr = np.random.RandomState(1).randint(0, 256, (37, 53, 3)).astype(np.uint8)
    Image.fromarray(arr).save(tmp_path / 'a.png')
    assert load_u8(str(tmp_path / 'a.png')).shape == (3, 32, 48)
    assert np.array_equal(load_u8(str(tmp_path / 'a.png'), crop=False), arr.transpose(2, 0, 1))
