"""Image sides of the ViT encoder, without a GPU: construction at 384 / 512 (N = 576 / 1024 tokens), the sides that still raise,
and the CPU oracle's ViT restatement (oracle/convnets_oracle.py, generic in N) pinned at N = 576 against the golden of the reference
class constructed with image_size=384 (tests/golden/make_golden_vit_sizes.py)."""
import pytest
import torch

import airnet_oracle as O
import convnets_oracle as C
import dropout_hash as DH
from helpers import close, load, make_opt, rnd, schema

VIT = dict(encoder_type='ViT', decoder_type='Uformer', encoder_dim=3, degradation_embedding_method=['None'], out_channels=3,
           batch_wise_decompose=False)


@pytest.mark.parametrize('size,tokens', [(384, 576), (512, 1024)])
def test_airnet_with_vit_builds_at_larger_patches(size, tokens):
    from net.model import AirNet
    net = AirNet(make_opt('all3', patch_size=size, **VIT))
    for enc in (net.E.E.encoder_q, net.E.E.encoder_k):
        assert tuple(enc.pos_embedding.shape) == (1, tokens, 768)
        assert enc.image_height == enc.image_width == size


@pytest.mark.parametrize('size', [64, 192, 640])
def test_other_sides_still_raise(size):
    from fwair.vit import ViTEncoder
    with pytest.raises(NotImplementedError, match='128, 256, 384 and 512'):
        ViTEncoder(make_opt('all3', patch_size=size, **VIT))


def test_oracle_vit_encoder_384_with_dropout():
    """eval, and train mode with Dropout on (the hashed masks both sides draw), within 1e-4 of the reference's outputs"""
    g = load('model_vit384_encoder')
    pre = 'E.E.encoder_q.'
    sch = [(k, [1, 576, 768] if k.endswith('.pos_embedding') else s, d) for k, s, d in schema('vit256_uformer')]
    st = {k[len(pre):]: v for k, v in O.fill_state_seeded(sch).items() if k.startswith(pre)}
    assert tuple(st['pos_embedding'].shape) == (1, 576, 768)
    opt = make_opt('all3', encoder_type='ViT', encoder_dim=3)
    x = rnd('vit384.x', (2, 3, 384, 384), 0.5)
    with torch.no_grad():
        fea, out, inter = C.vit_encoder(st, '', opt, x, False)
        close(fea, g['fea_eval'], 1e-4, 'fea (eval)')
        close(out[0], g['out_eval'], 1e-4, 'out (eval)')
        close(inter[:, :, ::4, ::4], g['inter_eval'], 1e-4, 'inter (eval)')
        fea, out, inter = C.vit_encoder(st, '', opt, x, True, {}, drop=(int(g['drop_seed']), DH.site_base(pre), 0.1))
        close(out[0], g['out_train'], 1e-4, 'out (train, Dropout on)')
        close(inter[:, :, ::4, ::4], g['inter_train'], 1e-4, 'inter (train, Dropout on)')
