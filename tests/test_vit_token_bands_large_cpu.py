"""Host side of `--vit_band_grid tokens` at 384x384 / 512x512 inputs (N = 576 / 1024 tokens): the spectral tables against the oracle's
masks (equal, transpose-symmetric -- the filter is self-adjoint, which the backward pass assumes -- and a partition of the grid), the
option parser, and the state_dict of the 384x384 model with `lamb`."""
import math
import sys

import pytest
import torch

import convnets_oracle as C
from helpers import make_opt, schema

VIT = dict(encoder_type='ViT', decoder_type='Uformer', encoder_dim=3, degradation_embedding_method=['None'], out_channels=3,
           batch_wise_decompose=False)


@pytest.mark.parametrize('ftype', ['DC', '3_bands', '5_bands'])
@pytest.mark.parametrize('n', [576, 1024])
def test_tables_equal_the_oracle_masks(n, ftype):
    from fwair import vit as V
    kind, nb = ('DC', 2) if ftype == 'DC' else ('bands', int(ftype.split('_')[0]))
    idx, panels = V._spectral_tables(kind, nb, 'cpu', n=n)
    masks = C.attn_band_masks(ftype, n)
    assert idx.shape == (n, n) and idx.dtype == torch.uint8 and masks.shape == (nb, n, n)
    assert bool(masks.sum(0).eq(1).all()), 'the masks do not partition the grid'
    assert int(idx.max()) == nb - 1
    for i in range(nb):
        assert torch.equal(idx == i, masks[i]), f'band {i}'
    assert torch.equal(idx, idx.t()), 'the band index is not transpose-symmetric'
    k = torch.arange(n, dtype=torch.float64)
    ang = 2 * math.pi * torch.outer(k, k) / n
    assert panels.shape == (2, n, n) and panels.dtype == torch.float32 and panels.is_contiguous()
    assert float((panels[0].double() - torch.cos(ang)).abs().max()) < 1e-7
    assert float((panels[1].double() - torch.sin(ang)).abs().max()) < 1e-7


@pytest.mark.parametrize('size,ftype', [(384, '3_bands'), (512, 'DC'), (512, '5_bands')])
def test_option_parser_takes_the_large_sides_with_tokens(monkeypatch, size, ftype):
    monkeypatch.setattr(sys, 'argv', ['x', '--degradation_embedding_method', 'all_3_bands'])
    sys.modules.pop('option', None)
    try:
        import option
        o = option.finalize(option.build_parser().parse_args(['--encoder_type', 'ViT', '--patch_size', str(size), '--frequency_decompose_type',
                                                              ftype, '--vit_band_grid', 'tokens']))
        assert (o.encoder_type, o.patch_size, o.frequency_decompose_type, o.vit_band_grid) == ('ViT', size, ftype, 'tokens')
    finally:
        sys.modules.pop('option', None)


@pytest.mark.parametrize('ftype,nb', [('3_bands', 3), ('DC', 2)])
def test_state_dict_of_the_384_model_with_lamb(ftype, nb):
    from net.model import AirNet
    net = AirNet(make_opt('all3', batch_size=1, patch_size=384, frequency_decompose_type=ftype, vit_band_grid='tokens', **VIT))
    mine = [(k, list(v.shape)) for k, v in net.state_dict().items()]
    ref = [(k, [1, 576, 768] if k.endswith('.pos_embedding') else list(s)) for k, s, _ in schema('vit256_uformer')]
    lamb = [e for e in mine if e[0].endswith('.fn.lamb')]
    assert [e for e in mine if not e[0].endswith('.fn.lamb')] == ref
    assert len(lamb) == 24 and all(s == [nb, 1, 12] for _, s in lamb)              # 12 layers of the query and of the key encoder
    assert net.E.E.encoder_q.transformer.band_grid == 'tokens'

