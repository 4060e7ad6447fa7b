"""Host side of `--vit_band_grid tokens` (ViT band masks sized by the attention map, N x N, instead of dim_head x dim_head):
the spectral tables for n = 256 against the oracle's masks, the option, and the state_dict of the 256x256 model with `lamb`."""
import math
import sys

import pytest
import torch

import convnets_oracle as C
from helpers import make_opt, schema

VIT = dict(encoder_type='ViT', decoder_type='Uformer', encoder_dim=3, degradation_embedding_method=['None'], out_channels=3,
           batch_wise_decompose=False)


@pytest.mark.parametrize('ftype', ['2_bands', '3_bands', '5_bands', '16_bands', 'DC'])
def test_tables_at_256_equal_the_oracle_masks(ftype):
    from fwair import vit as V
    kind, nb = ('DC', 2) if ftype == 'DC' else ('bands', int(ftype.split('_')[0]))
    idx, panels = V._spectral_tables(kind, nb, 'cpu', n=256)
    masks = C.attn_band_masks(ftype, 256)
    assert idx.shape == (256, 256) and idx.dtype == torch.uint8 and masks.shape == (nb, 256, 256)
    assert bool(masks.sum(0).eq(1).all())
    for i in range(nb):
        assert torch.equal(idx == i, masks[i]), f'band {i}'
    k = torch.arange(256, dtype=torch.float64)
    ang = 2 * math.pi * torch.outer(k, k) / 256
    assert panels.shape == (2, 256, 256) and panels.dtype == torch.float32
    assert float((panels[0].double() - torch.cos(ang)).abs().max()) < 1e-7
    assert float((panels[1].double() - torch.sin(ang)).abs().max()) < 1e-7


def test_three_argument_call_is_unchanged():
    from fwair import vit as V
    idx, panels = V._spectral_tables('bands', 3, 'cpu')
    assert idx.shape == (64, 64) and panels.shape == (2, 64, 64)
    masks = C.attn_band_masks('3_bands', 64)
    for i in range(3):
        assert torch.equal(idx == i, masks[i])
    idx2, panels2 = V._spectral_tables('bands', 3, 'cpu', n=64)
    assert idx2 is idx and panels2 is panels


def test_option_vit_band_grid(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['x', '--degradation_embedding_method', 'all_3_bands'])
    sys.modules.pop('option', None)
    try:
        import option
        p = option.build_parser()
        assert p.parse_args([]).vit_band_grid == 'head_dim'
        assert p.parse_args(['--vit_band_grid', 'tokens']).vit_band_grid == 'tokens'
        with pytest.raises(SystemExit):
            p.parse_args(['--vit_band_grid', 'pixels'])
    finally:
        sys.modules.pop('option', None)


@pytest.mark.parametrize('ftype,nb', [('3_bands', 3), ('DC', 2)])
def test_state_dict_of_the_256_model_with_lamb(ftype, nb):
    from net.model import AirNet
    net = AirNet(make_opt('all3', batch_size=1, patch_size=256, frequency_decompose_type=ftype, vit_band_grid='tokens', **VIT))     # schema: K = 3
    mine = [(k, list(v.shape)) for k, v in net.state_dict().items()]
    ref = [(k, list(s)) for k, s, _ in schema('vit256_uformer')]
    lamb = [e for e in mine if e[0].endswith('.fn.lamb')]
    assert [e for e in mine if not e[0].endswith('.fn.lamb')] == ref
    assert len(lamb) == 24 and all(s == [nb, 1, 12] for _, s in lamb)              # 12 layers of the query and of the key encoder
    assert net.E.E.encoder_q.transformer.band_grid == 'tokens'
    with pytest.raises(ValueError):
        AirNet(make_opt('all3', patch_size=256, frequency_decompose_type=ftype, vit_band_grid='pixels', **VIT))
