"""Host side of the band statistics (fwair/spectrum.py): the ring tables against the reference's get_frequency_distribution (fixture
unit_band_stats.npz, tests/golden/make_golden_band_stats.py), the band partition, and restore.py's --band_report flag."""
import sys

import numpy as np
import pytest

import band_stats_cases as BC
from helpers import load


@pytest.mark.parametrize('h,w,size', BC.CASES)
def test_plot_rings_reproduce_the_reference(h, w, size):
    """ring_index('plot') and numpy's f64 FFT against the reference's own triple loop: 1e-12 relative, raw and normalised"""
    from fwair import spectrum as S
    g = load('unit_band_stats')
    ring = S.ring_index('plot', size, h, w)
    nb = int(1 / size)
    assert ring.dtype == np.uint8 and ring.shape == (h, w) and set(np.unique(ring)) <= set(range(nb)) | {255}
    assert len(S.ring_edges('plot', size, h, w)[0]) == nb
    raw = BC.band_sums(BC.images(h, w), ring, nb, 0)
    ref_raw, ref_norm = g[BC.key(h, w, size, False)].numpy(), g[BC.key(h, w, size, True)].numpy()
    assert ref_raw.shape == (BC.NIMG, nb)
    assert BC.rel_err(raw, ref_raw) <= 1e-12
    assert BC.rel_err(raw / raw.sum(1, keepdims=True), ref_norm) <= 1e-12


def test_plot_rings_leave_out_what_lies_beyond_half_the_width():
    from fwair import spectrum as S
    ring = S.ring_index('plot', 0.2, 40, 24)
    Y, X = np.ogrid[:40, :24]
    d = np.sqrt((X - 12) ** 2 + (Y - 20) ** 2)
    assert (ring[d > 12] == 255).all() and (ring[d <= 12] != 255).all()
    assert ring[20, 12] == 0 and ring[20, 0] == 4 and ring[20, 23] == 4          # d = 12 = diag: the last ring is closed


@pytest.mark.parametrize('h,w', [(33, 47), (320, 480)])
@pytest.mark.parametrize('nb', [1, 3, 5, 8])
def test_bands_cover_every_bin_exactly_once(h, w, nb):
    import torch
    from fwair import lfs, spectrum as S
    ring = S.ring_index('bands', 1.0 / nb, h, w)
    assert ring.shape == (h, w) and ring.max() == nb - 1 and ring.min() == 0
    masks = torch.stack(lfs.band_masks_shifted('frequency_decompose', 1.0 / nb, h, w)).numpy()
    assert masks.shape[0] == nb
    for b in range(nb):
        assert np.array_equal(ring == b, masks[b])
    assert sum(int((ring == b).sum()) for b in range(nb)) == h * w
    assert ring[h // 2, w // 2] == 0 and ring[0, 0] == nb - 1
    edges, rmax = S.ring_edges('bands', 1.0 / nb, h, w)
    assert len(edges) == nb and edges[0][0] == 0 and abs(edges[-1][1] - rmax) < 1e-6 * rmax


def test_empty_rings_give_exactly_zero():
    """8 x 8, size 0.1: diag = 4, rings 0.4 wide -- no bin has 0.4 <= d < 0.8 (ring 1), and others are empty too"""
    from fwair import spectrum as S
    ring = S.ring_index('plot', 0.1, 8, 8)
    empty = [b for b in range(10) if not (ring == b).any()]
    assert 1 in empty
    for power in (0, 1):
        s = BC.band_sums(BC.images(8, 8), ring, 10, power)
        assert (s[:, empty] == 0).all() and (np.delete(s, empty, 1) > 0).all()
        assert (BC.emulate_f32(BC.images(8, 8), ring, 10, power)[:, empty] == 0).all()


def test_a_bin_in_two_rings_is_an_error(monkeypatch):
    """rings that overlap (a linspace whose steps are smaller than the ring width) must not be counted twice silently"""
    from fwair import spectrum as S
    real = np.linspace
    monkeypatch.setattr(S.np, 'linspace', lambda a, b, n: real(a, b, n) * 0.9 + 0.1)
    with pytest.raises(ValueError, match='two rings'):
        S.ring_index('plot', 0.2, 16, 16)


def test_emulation_agrees_with_f64():
    """the f32 chain the GPU test derives its limit from is the DFT: 1e-5 of every band at a size with two tiles per axis"""
    from fwair import spectrum as S
    h, w = 65, 130
    ring = S.ring_index('plot', 0.2, h, w)
    x = BC.images(h, w)
    for power in (0, 1):
        assert BC.rel_err(BC.emulate_f32(x, ring, 5, power), BC.band_sums(x, ring, 5, power)) < 1e-5


def test_work_buffer_formula():
    from fwair import spectrum as S
    assert S.work_floats(1, 8, 8, 1) == 2 * 64 * 64 + 1
    assert S.work_floats(3, 321, 481, 5) == 3 * (2 * 384 * 256 + 6 * 4 * 5)           # 241 columns -> 256
    assert S.work_floats(1, 64, 126, 2) == 2 * 64 * 64 + 2 and S.work_floats(1, 64, 128, 2) == 2 * 64 * 128 + 2 * 2      # 64 / 65 columns
    assert S.panels_host(9).shape == (3, 64, 64) and S.panels_host(65).shape == (3, 128, 128)
    p = S.panels_host(9)
    assert (p[:, 9:, :] == 0).all() and (p[:, :, 9:] == 0).all() and p[0, 0, 0] == 1 and p[2, 1, 1] == -p[1, 1, 1]


def test_restore_parses_band_report(monkeypatch):
    """restore.py: --band_report N, 0 by default, taken off the command line option.py parses"""
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
    assert a.band_report == 0
    a, argv = parsed(['--band_report', '3'])
    assert a.band_report == 3
    assert argv[1:] == ['--degradation_embedding_method', 'all_3_bands']
