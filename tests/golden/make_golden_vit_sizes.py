"""Golden vectors of the ViT encoder at 384x384 (N = 576 tokens) -- runs ONLY where the reference checkout exists, like
make_golden.py, whose helpers it imports unchanged (name-seeded weights, hashed Dropout masks patched into the imported reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vit_sizes.py

  model_vit384_encoder.npz   the reference's ViTEncoder(opt, image_size=384): eval outputs, TRAIN-mode outputs with every Dropout at
                             p = 0.1, `inter` at every 4th pixel, gradient norms, the small gradient tensors, drop_seed
                             (the keys of model_vit256_encoder.npz)
  model_vit384_uformer.npz   ViT(384) + plain Uformer decoder (img_size=384), eval: `restored` at every 3rd pixel, and the PSNR

schema.json is not touched: the state dict is that of `vit256_uformer` with pos_embedding [1, 576, 768] (tests derive it).
A fixture is data (expected outputs); no reference source text is stored."""
import numpy as np
import torch

import make_golden as MG
from make_golden import O, RD, AirNet, opt, rnd, save, seed_module, set_opt, synth_batch

SIZE = 384


def gen_vit384():
    from net import encoder_ViT as RV
    import net.model as RM
    set_opt(encoder_type='ViT', decoder_type='Uformer', encoder_dim=3, batch_size=2, degradation_embedding_method=['None'],
            frequency_decompose_type='none', out_channels=3, batch_wise_decompose=False)
    keep_fwd = torch.nn.Dropout.forward
    try:
        MG.patch_dropout(MG.DROP_SEED)
        pre = 'E.E.encoder_q.'
        enc = seed_module(RV.ViTEncoder(opt, image_size=SIZE), pre)
        assert tuple(enc.pos_embedding.shape) == (1, (SIZE // 16) ** 2, 768)
        MG.assign_vit_sites(enc, pre)
        x = rnd('vit384.x', (2, 3, SIZE, SIZE), 0.5)
        save('model_vit384_encoder', drop_seed=np.int64(MG.DROP_SEED), **MG.vit_encoder_arrays(enc, x, 'vit384.', 4))
        keep = RM.ViTEncoder, RM.UformerDecoder
        RM.ViTEncoder = lambda o: RV.ViTEncoder(o, image_size=SIZE)
        RM.UformerDecoder = lambda o: RD.UformerDecoder(o, img_size=SIZE)
        try:
            set_opt(batch_size=1)
            net = seed_module(AirNet(opt), '')
        finally:
            RM.ViTEncoder, RM.UformerDecoder = keep
        for pq, pk in zip(net.E.E.encoder_q.parameters(), net.E.E.encoder_k.parameters()):
            pk.data.copy_(pq.data)
        clean, q, k = synth_batch(1, SIZE, 'model384.')
        net.eval()
        with torch.no_grad():
            restored = net(x_query=q, x_key=q)
        save('model_vit384_uformer', restored_eval=restored[:, :, ::3, ::3], psnr_eval=O.psnr(restored, clean))
    finally:
        torch.nn.Dropout.forward = keep_fwd
        set_opt(encoder_type='Uformer', decoder_type='Uformer', encoder_dim=256, degradation_embedding_method=['all_3_bands'], batch_size=2)


if __name__ == '__main__':
    gen_vit384()
