"""Golden vectors of the model at the decoder widths --embed_dim 32 and 64 (the default, 56, is what make_golden.py covers) -- runs
ONLY where the reference checkout exists, like make_golden.py, whose helpers it imports unchanged (name-seeded weights and inputs,
DropPath neutralised).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_widths.py

  schema_widths.json     the state-dict schema of the reference AirNet built with embed_dim 32 / 64 (encoder_embed_dim stays 28).  Its
                         keys, their order and their dtypes are those of schema.json's `all3` (asserted here), so only what the width
                         changes is stored: {"keys": "schema.json:all3", "32": [shape, ...], "64": [shape, ...]}, one shape per key
                         in state-dict order.  schema.json is not touched.
  model_all3_w32.npz     the keys of model_all3_modulator.npz without the table entries, at 128x128, B = 1, all_3_bands / L = 3 / freq,
  model_all3_w64.npz     every pixel stored; inputs synth_batch(1, 128, 'w32.') / synth_batch(1, 128, 'w64.').

A fixture is data (expected outputs); no reference source text is stored."""
import json
import os
import time

import numpy as np
import torch

from make_golden import HERE, O, AirNet, grads_of, opt, save, schema_of, seed_module, set_opt, synth_batch

WIDTHS = (32, 64)
G_NAMES = ('R.R.output_proj.proj.0.weight', 'R.R.input_proj.proj.0.weight', 'E.E.encoder_q.uformer.input_proj.proj.0.weight',
           'R.R.bottleneck_0.blocks.1.attn.relative_position_bias_table')


def gen_width(E):
    t0 = time.time()
    set_opt(batch_size=1, degradation_embedding_method=['all_3_bands'], L=3, encoder_msa_type='freq', learnable_modulator=False,
            embed_dim=E)
    net = seed_module(AirNet(opt), '')
    for pq, pk in zip(net.E.E.encoder_q.parameters(), net.E.E.encoder_k.parameters()):
        pk.data.copy_(pq.data)
    schema = schema_of(net)
    nparam = sum(p.numel() for p in net.R.parameters())
    clean, q, k = synth_batch(1, 128, f'w{E}.')
    net.eval()
    with torch.no_grad():
        restored_eval = net(x_query=q, x_key=q)
    arrs = {'restored_eval': restored_eval, 'psnr_eval': O.psnr(restored_eval, clean), 'psnr_input': O.psnr(q, clean)}
    net.train()
    restored, logits, labels = net(x_query=q, x_key=k)
    CE = torch.nn.CrossEntropyLoss()
    contrast = sum(CE(logits[i], labels[i]) for i in range(opt.L)) / opt.L
    l1 = torch.nn.L1Loss()(restored, clean)
    loss = l1 + opt.contrast_loss_weight * contrast
    g = grads_of(net, loss)
    names = sorted(g.keys())
    arrs.update({'restored_train': restored, 'logits': torch.stack(logits, 0), 'loss': loss, 'l1': l1, 'contrast': contrast,
                 'grad_names': np.array(names), 'grad_norms': np.array([g[n].norm().item() for n in names]),
                 'queue_after': net.E.E.queue, 'queue_ptr_after': net.E.E.queue_ptr})
    for n in G_NAMES:
        arrs['g.' + n] = g[n]
    save(f'model_all3_w{E}', **arrs)
    print('embed_dim %d: %.1f M decoder parameters, done in %.1fs' % (E, nparam / 1e6, time.time() - t0))
    return schema


if __name__ == '__main__':
    with torch.enable_grad():
        schemas = {str(E): gen_width(E) for E in WIDTHS}
    with open(os.path.join(HERE, 'schema.json')) as f:
        base = json.load(f)['all3']
    out = {'keys': 'schema.json:all3'}
    for E, schema in schemas.items():
        assert [(k, d) for k, _, d in schema] == [(k, d) for k, _, d in base], 'keys / dtypes differ from schema.json all3'
        out[E] = [shape for _, shape, _ in schema]
    with open(os.path.join(HERE, 'schema_widths.json'), 'w') as f:
        f.write('{' + ',\n'.join(json.dumps(k) + ': ' + json.dumps(v, separators=(',', ':')) for k, v in out.items()) + '}\n')
