"""The Uformer encoder at 384 and 512 pixels, host side: construction, the sides FrequencyDecompose accepts, and the CPU oracle
against the goldens the REAL reference produced at those sizes (tests/golden/make_golden_uformer_sizes.py).
Limits: those of tests/test_oracle_golden.py (2e-5 rel-to-max for the band decomposition) and of
tests/test_oracle_model.py::test_256_eval_and_train_step (1e-4 on `restored`, 1e-3 dB on the PSNR)."""
import pytest
import torch

import airnet_oracle as O
from helpers import close, load, make_opt, rnd, schema, synth_batch


@pytest.mark.parametrize('S', [384, 512])
def test_airnet_constructs(S):
    from net.model import AirNet
    net = AirNet(make_opt('all3', batch_size=1, patch_size=S))
    fd = net.E.E.encoder_q.preprocess_decompose
    assert fd.h == S and fd.w == S and fd.type == 'frequency_decompose_1'
    assert net.E.E.encoder_k.preprocess_decompose.h == S


@pytest.mark.parametrize('h,w', [(320, 384), (576, 576), (100, 100)])
def test_frequency_decompose_rejects_other_sides(h, w):
    from net.utils.frequency_decompose import FrequencyDecompose
    with pytest.raises(NotImplementedError, match=r'power of two in \[8, 256\] or a multiple of 64 in \[192, 512\]'):
        FrequencyDecompose('frequency_decompose', 1 / 3., h, w)


@pytest.mark.parametrize('N', [8, 64, 128, 192, 256, 320, 384, 448, 512])
def test_frequency_decompose_accepts(N):
    from net.utils.frequency_decompose import FrequencyDecompose, _tiled_side
    assert FrequencyDecompose('frequency_decompose_1', 0.5, N, N).num_bands == 2
    assert _tiled_side(N) == (N in (192, 320, 384, 448, 512))            # 256 and below keep the kernels they had


@pytest.mark.parametrize('fixture', ['unit_freq_decompose_384', 'unit_freq_decompose_384_spectra'])
def test_oracle_frequency_decompose_384(fixture):
    g = load(fixture)
    n = 384
    x = rnd(f'fd{n}', (1, 2, n, n))                                          # the golden does not store it
    assert len(g) == (4 if fixture.endswith('384') else 6)
    for tag, ref in g.items():
        kind, size, inv = tag.split('|')
        inv = {'True': True, 'False': False}.get(inv, inv)
        out = O.frequency_decompose(x, kind, float(size), n, n, inv)
        close(out[:, :, :, ::4, ::4], ref, 2e-5, tag)


def test_oracle_model_384_eval():
    """airnet_forward in eval mode at 384 against the reference's classes built with img_size=384 (as test_oracle_model.py does at
    256).  The 512 forward is NOT repeated on the CPU: this 384 forward already takes most of a minute on a CPU and a
    512x512 one has 1.8x its tokens; the 512 golden is checked on the GPU (tests/test_uformer384_gpu.py), its inputs are pinned below."""
    g = load('model384_all3')
    st = O.fill_state_seeded(schema('all3'))
    st['E.E.queue'] = torch.nn.functional.normalize(O.seeded_tensor('E.E.queue', (3, 256, 3)) / 0.02, dim=1)   # K = 3 * batch_size
    opt = make_opt('all3', batch_size=1, patch_size=384)
    clean, q, k = synth_batch(1, 384, 'model384.')
    with torch.no_grad():
        out = O.airnet_forward(st, opt, q, q, False)
    close(out[:, :, ::3, ::3], g['restored_eval'], 1e-4, 'restored_eval (384)')
    assert abs(O.psnr(out, clean) - float(g['psnr_eval'])) < 1e-3
    assert abs(O.psnr(q, clean) - float(g['psnr_input'])) < 1e-3


def test_golden_512_inputs_and_keys():
    g = load('model512_all3')
    assert sorted(g) == ['psnr_eval', 'psnr_input', 'restored_eval']
    assert tuple(g['restored_eval'].shape) == (1, 3, 128, 128)
    clean, q, k = synth_batch(1, 512, 'model512.')
    assert abs(O.psnr(q, clean) - float(g['psnr_input'])) < 1e-3
    assert sorted(load('model384_all3')) == sorted(load('model256_all3'))
