"""Golden vectors of the model with the decoder's learnable window modulator (--learnable_modulator True) -- runs ONLY where the
reference checkout exists, like make_golden.py, whose helpers it imports unchanged (name-seeded weights and inputs, DropPath
neutralised).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_modulator.py

  schema_modulator.json     state-dict schema (key, shape, dtype) of the reference AirNet built with the flag: schema.json's `all3`
                            plus the 20 `R.R.decoderlayer_{3,2,1,0}.blocks.<i>.modulator.weight` tables.  schema.json is not touched.
  model_all3_modulator.npz  the keys of model384_all3.npz at 128x128, B = 1, all_3_bands / L = 3 / freq, every pixel stored;
                            g.<name> of three modulator tables (decoderlayer_0 blocks 0 and 1 -- the un-shifted and the shifted
                            block of the widest map -- and decoderlayer_2 block 1); restored_eval_zero_mod: the eval output with
                            every table zeroed (what a port that ignores the flag computes).

seed_module fills every floating tensor at the 0.02 scale of the name-seeded RNG; a table that small moves the output by 6.9e-4 of
its maximum only, too close to the 1e-4 limit of the model tests to show an omitted table.  nn.Embedding initialises N(0, 1), so
every `*.modulator.weight` is re-seeded at unit variance: seeded_tensor(name, shape) / 0.02 (MOD_SCALE below; tests repeat it).
A fixture is data (expected outputs); no reference source text is stored."""
import json
import os
import time

import numpy as np
import torch

from make_golden import HERE, O, AirNet, grads_of, opt, save, schema_of, seed_module, set_opt, synth_batch

G_TABLES = ('R.R.decoderlayer_0.blocks.0.modulator.weight', 'R.R.decoderlayer_0.blocks.1.modulator.weight',
            'R.R.decoderlayer_2.blocks.1.modulator.weight')


def gen_modulator():
    t0 = time.time()
    set_opt(batch_size=1, degradation_embedding_method=['all_3_bands'], L=3, encoder_msa_type='freq', learnable_modulator=True)
    net = seed_module(AirNet(opt), '')
    tables = {}
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith('.modulator.weight'):
                p.copy_(O.seeded_tensor(name, tuple(p.shape)) / 0.02)
                tables[name] = p
    assert len(tables) == 20, len(tables)
    for pq, pk in zip(net.E.E.encoder_q.parameters(), net.E.E.encoder_k.parameters()):
        pk.data.copy_(pq.data)
    with open(os.path.join(HERE, 'schema_modulator.json'), 'w') as f:
        json.dump(schema_of(net), f)
    clean, q, k = synth_batch(1, 128, 'modulator.')
    net.eval()
    with torch.no_grad():
        restored_eval = net(x_query=q, x_key=q)
        kept = {n: p.detach().clone() for n, p in tables.items()}
        for p in tables.values():
            p.zero_()
        restored_zero = net(x_query=q, x_key=q)
        for n, p in tables.items():
            p.copy_(kept[n])
    arrs = {'restored_eval': restored_eval, 'restored_eval_zero_mod': restored_zero, 'psnr_eval': O.psnr(restored_eval, clean),
            'psnr_input': O.psnr(q, clean)}
    net.train()
    restored, logits, labels = net(x_query=q, x_key=k)
    CE = torch.nn.CrossEntropyLoss()
    contrast = sum(CE(logits[i], labels[i]) for i in range(opt.L)) / opt.L
    l1 = torch.nn.L1Loss()(restored, clean)
    loss = l1 + opt.contrast_loss_weight * contrast
    g = grads_of(net, loss)
    names = sorted(g.keys())
    assert all(n in g for n in tables)
    arrs.update({'restored_train': restored, 'logits': torch.stack(logits, 0), 'loss': loss, 'l1': l1, 'contrast': contrast,
                 'grad_names': np.array(names), 'grad_norms': np.array([g[n].norm().item() for n in names]),
                 'queue_after': net.E.E.queue, 'queue_ptr_after': net.E.E.queue_ptr})
    for n in ('R.R.output_proj.proj.0.weight', 'R.R.input_proj.proj.0.weight', 'E.E.encoder_q.uformer.input_proj.proj.0.weight',
              'R.R.bottleneck_0.blocks.1.attn.relative_position_bias_table') + G_TABLES:
        arrs['g.' + n] = g[n]
    save('model_all3_modulator', **arrs)
    sep = float((restored_eval - restored_zero).abs().max() / restored_eval.abs().max())
    mod_norms = [g[n].norm().item() for n in tables]
    print('max|restored_eval - restored_eval_zero_mod| / max|restored_eval| = %.3e' % sep)
    print('modulator gradient norms %.3e .. %.3e; largest norm of the model %.3e' % (min(mod_norms), max(mod_norms), max(arrs['grad_norms'])))
    print('modulator done in %.1fs' % (time.time() - t0))


if __name__ == '__main__':
    with torch.enable_grad():
        gen_modulator()
