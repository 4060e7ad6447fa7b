"""Host side of the band split (fwair/spectrum.py: fw_band_split's tables and wrappers, BandSplit), debug_mode at 384 pixels,
restore.py's --band_images flag, and the f32 emulation the GPU test's bound rests on."""
import sys

import numpy as np
import pytest
import torch

import band_split_cases as SC
from helpers import make_opt


@pytest.mark.parametrize('h,w', SC.GOLDEN_SIZES)
def test_bands_1_ring_is_the_argmax_of_the_masks(h, w):
    from fwair import lfs, spectrum as S
    for size in (0.5, 1 / 3., 1.0):
        masks = torch.stack(lfs.band_masks_shifted('frequency_decompose_1', size, h, w))
        assert bool((masks.sum(0) == 1).all())
        ring = S.ring_index('bands_1', size, h, w)
        assert ring.dtype == np.uint8 and np.array_equal(ring, masks.to(torch.uint8).argmax(0).numpy())
        nb = masks.shape[0]
        assert len(S.ring_edges('bands_1', size, h, w)[0]) == nb == int(ring.max()) + 1
        assert ring[h // 2, w // 2] == 0 and int((ring == 0).sum()) == 1, 'band 0 is DC alone'
        table, n = S.ring_table('bands_1', size, h, w, 'cpu')
        assert n == nb and table[0, 0] == 0 and table.dtype == torch.uint8
    # the kinds that were there keep their results
    assert np.array_equal(S.ring_index('bands', 1 / 3., h, w),
                          torch.stack(lfs.band_masks_shifted('frequency_decompose', 1 / 3., h, w)).to(torch.uint8).argmax(0).numpy())


def test_work_buffer_formula():
    """include/fwair.h: nimg * Hp * Wh * 4 floats, in mode 0 plus 2 * min(nbands, 4) more planes"""
    from fwair import spectrum as S
    assert S.split_work_floats(1, 8, 8, 1, 0) == 64 * 64 * 6 and S.split_work_floats(1, 8, 8, 1, 1) == 64 * 64 * 4
    assert S.split_work_floats(3, 321, 481, 3, 0) == 3 * 384 * 256 * 10 and S.split_work_floats(3, 321, 481, 3, 2) == 3 * 384 * 256 * 4
    assert S.split_work_floats(2, 65, 130, 32, 0) == 2 * 128 * 128 * 12                       # 66 columns -> 128; at most 4 bands at a time
    assert S.split_work_floats(1, 64, 126, 2, 0) == 64 * 64 * 8 and S.split_work_floats(1, 64, 128, 2, 0) == 64 * 128 * 8
    from fwair.lib import parse_header
    sig = parse_header()['fw_band_split']
    assert len(sig) == 14 and [p for _, p in sig] == [False] + [True] * 7 + [False] * 5 + [True]


@pytest.mark.parametrize('h,w', [(320, 384), (100, 100), (24, 24)])
def test_band_split_constructs_where_frequency_decompose_raises(h, w):
    from fwair import spectrum as S
    from net.utils.frequency_decompose import FrequencyDecompose
    for kind, size, nb in (('frequency_decompose', 1 / 3., 3), ('frequency_decompose_1', 0.5, 2), ('frequency_decompose_dc', 0.5, None)):
        m = S.BandSplit(kind, size, h, w, inverse=True)
        assert not list(m.parameters()) and not list(m.buffers())
        if nb is not None:
            assert m.num_bands == nb
            with pytest.raises(NotImplementedError, match='HIP band decomposition handles square maps'):
                FrequencyDecompose(kind, size, h, w)
    with pytest.raises(NotImplementedError):
        S.BandSplit('frequency_decompose', 0.5, 7, 16)
    with pytest.raises(NotImplementedError):
        S.BandSplit('frequency_decompose', 0.5, 16, 1025)
    x = torch.zeros(1, 1, h, w, requires_grad=True)
    with pytest.raises(NotImplementedError, match='forward only'):
        S.BandSplit('frequency_decompose', 0.5, h, w)(x)


def test_airnet_constructs_at_384_with_debug_mode():
    from fwair import spectrum as S
    from net.model import AirNet
    from net.utils.frequency_decompose import FrequencyDecompose
    net = AirNet(make_opt('all3', batch_size=1, patch_size=384, debug_mode=True))
    sides = {}
    for m in net.modules():
        v = getattr(m, 'visual_decompose', None)
        if v is not None:
            sides.setdefault(type(v), set()).add((v.h, v.w))
    assert sides[S.BandSplit] == {(96, 96), (48, 48), (24, 24)} and sides[FrequencyDecompose] == {(384, 384), (192, 192)}
    plain = AirNet(make_opt('all3', batch_size=1, patch_size=384))
    assert list(plain.state_dict().keys()) == list(net.state_dict().keys())


def test_restore_parses_band_images(monkeypatch, capsys):
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

    a, _ = parsed([])
    assert a.band_images == 0
    a, argv = parsed(['--band_images', '3', '--input', 'x', '--output', 'y'])
    assert a.band_images == 3 and argv[1:] == ['--degradation_embedding_method', 'all_3_bands']
    a, _ = parsed(['--band_images', '2', '--save_imgs', 'True'])
    assert a.band_images == 2
    with pytest.raises(SystemExit):
        parsed(['--band_images', '3'])                                   # test sets without --save_imgs True
    assert '--save_imgs True' in capsys.readouterr().err


def _cases():
    return [(h, w, SC.NIMG, kind, size) for h, w in SC.SHAPES for kind, size in SC.RING_KINDS] + [SC.LARGEST + (1,) + SC.RING_KINDS[0]]


def test_emulated_chain_against_f64():
    """The kernel's four passes in f32 with its order of accumulation, at every shape of the GPU test and both ring kinds (and a ring
    without symmetry): the largest deviation from the f64 FFT, relative to the reference's maximum, must leave the 2e-5 of the GPU test
    a margin of 10 times."""
    worst = {}
    for h, w, n, kind, size in _cases():
        x = SC.maps(h, w, n)
        ring = SC.ring_unshifted(kind, size, h, w)
        nb = int(ring.max()) + 1
        e = SC.rel_max_err(SC.emulate_f32(x, ring, nb), SC.reference(x, ring, nb, 0))
        worst[(h, w)] = max(worst.get((h, w), 0.0), e)
    for h, w in ((33, 47), (40, 24)):
        x, ring = SC.maps(h, w, 2), SC.random_ring(h, w, 4, h * 7 + w)
        worst[(h, w, 'random ring')] = SC.rel_max_err(SC.emulate_f32(x, ring, 4), SC.reference(x, ring, 4, 0))
    print('f32 emulation against f64, relative to the maximum:', {k: f'{v:.2e}' for k, v in worst.items()})
    assert max(worst.values()) * 10 <= SC.TOL, max(worst.values())


def test_weights_are_the_symmetrised_ring():
    w = SC.weights(SC.random_ring(9, 8, 3, 1), 3)
    assert w.shape == (3, 9, 5) and set(np.unique(w)) <= {0.0, 0.5, 1.0, 2.0}
    ring = SC.ring_unshifted('bands', 1 / 3., 9, 8)
    w = SC.weights(ring, 3)                                              # a symmetric partition: c_v in the bin's own band
    assert np.array_equal(w.sum(0), np.tile(np.array([1, 2, 2, 2, 1], dtype=np.float32), (9, 1)))
