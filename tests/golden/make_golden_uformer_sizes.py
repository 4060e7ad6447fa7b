"""Golden vectors of the Uformer encoder + Uformer decoder at 384x384 and 512x512 -- runs ONLY where the reference checkout exists,
like make_golden.py, whose helpers it imports unchanged (name-seeded weights and inputs, DropPath neutralised).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_uformer_sizes.py [unit] [model384] [model512]

  unit_freq_decompose_384.npz  the reference FrequencyDecompose at 384 on rnd('fd384', (1, 2, 384, 384)): the four kinds of
                               make_golden.gen_unit, inverse=True, every 4th pixel ([..., ::4, ::4] of the two map axes).
                               x is NOT stored: a test rebuilds it from the seed name.
  unit_freq_decompose_384_spectra.npz  the same kinds with inverse False / 'visual', every 4th bin -- a file of its own so that
                               each fixture stays below 1 MiB
  model384_all3.npz            the keys of model256_all3.npz from the reference classes with img_size=384, B = 1, all_3_bands / L = 3 /
                               freq; restored_eval / restored_train at every 3rd pixel
  model512_all3.npz            eval only, img_size=512: restored_eval at every 4th pixel, psnr_eval, psnr_input

schema.json is not touched: no parameter's shape depends on the image size (tests derive it from `all3`).
A fixture is data (expected outputs); no reference source text is stored."""
import time

import numpy as np
import torch

import make_golden as MG
from make_golden import O, RD, RE, AirNet, FrequencyDecompose, grads_of, opt, rnd, save, seed_module, set_opt, synth_batch


def gen_unit384():
    n = 384
    x = rnd(f'fd{n}', (1, 2, n, n))
    out, spectra = {}, {}
    for kind, size in (('frequency_decompose', 1 / 3.), ('frequency_decompose_1', 0.5),
                       ('frequency_decompose_dc', 0.5), ('frequency_decompose', 1.0)):
        for inv in (True, False, 'visual'):
            if kind == 'frequency_decompose_dc' and inv is not True:
                continue
            y = FrequencyDecompose(kind, size, n, n, inverse=inv)(x)
            if torch.is_complex(y):
                y = torch.view_as_real(y)
            (out if inv is True else spectra)[f'{kind}|{size:.4f}|{inv}'] = y[:, :, :, ::4, ::4]      # [nb, B, C, h, w(, 2)]
    save(f'unit_freq_decompose_{n}', **out)
    save(f'unit_freq_decompose_{n}_spectra', **spectra)


def _net(size):
    import net.model as RM
    set_opt(batch_size=1, degradation_embedding_method=['all_3_bands'], L=3, encoder_msa_type='freq')
    keep = RM.UformerEncoder, RM.UformerDecoder
    RM.UformerEncoder = lambda o: RE.UformerEncoder(o, img_size=size)
    RM.UformerDecoder = lambda o: RD.UformerDecoder(o, img_size=size)
    try:
        net = seed_module(AirNet(opt), '')
    finally:
        RM.UformerEncoder, RM.UformerDecoder = keep
    for pq, pk in zip(net.E.E.encoder_q.parameters(), net.E.E.encoder_k.parameters()):
        pk.data.copy_(pq.data)
    return net


def gen_model384():
    t0 = time.time()
    net = _net(384)
    clean, q, k = synth_batch(1, 384, 'model384.')
    net.eval()
    with torch.no_grad():
        restored_eval = net(x_query=q, x_key=q)
    arrs = {'restored_eval': restored_eval[:, :, ::3, ::3], 'psnr_eval': O.psnr(restored_eval, clean), 'psnr_input': O.psnr(q, clean)}
    net.train()
    restored, logits, labels = net(x_query=q, x_key=k)
    CE = torch.nn.CrossEntropyLoss()
    contrast = sum(CE(logits[i], labels[i]) for i in range(opt.L)) / opt.L
    l1 = torch.nn.L1Loss()(restored, clean)
    loss = l1 + opt.contrast_loss_weight * contrast
    g = grads_of(net, loss)
    names = sorted(g.keys())
    arrs.update({'restored_train': restored[:, :, ::3, ::3], 'logits': torch.stack(logits, 0), 'loss': loss, 'l1': l1, 'contrast': contrast,
                 'grad_names': np.array(names), 'grad_norms': np.array([g[n].norm().item() for n in names]),
                 'queue_after': net.E.E.queue, 'queue_ptr_after': net.E.E.queue_ptr})
    for n in ('R.R.output_proj.proj.0.weight', 'R.R.input_proj.proj.0.weight', 'E.E.encoder_q.uformer.input_proj.proj.0.weight',
              'R.R.bottleneck_0.blocks.1.attn.relative_position_bias_table'):
        arrs['g.' + n] = g[n]
    save('model384_all3', **arrs)
    print('model384 done in %.1fs' % (time.time() - t0))


def gen_model512():
    t0 = time.time()
    net = _net(512)
    clean, q, k = synth_batch(1, 512, 'model512.')
    net.eval()
    with torch.no_grad():
        restored_eval = net(x_query=q, x_key=q)
    save('model512_all3', restored_eval=restored_eval[:, :, ::4, ::4], psnr_eval=O.psnr(restored_eval, clean), psnr_input=O.psnr(q, clean))
    print('model512 done in %.1fs' % (time.time() - t0))


if __name__ == '__main__':
    what = MG._ARGV or ['unit', 'model384', 'model512']          # make_golden keeps the command line; the shim rewrites sys.argv
    with torch.enable_grad():
        if 'unit' in what:
            gen_unit384()
        if 'model384' in what:
            gen_model384()
        if 'model512' in what:
            gen_model512()
