#!/usr/bin/env python3
"""Time to evaluate one test set (test.py:36-84) two ways, one process, one net (BASELINE configs[1], bf16): 68 synthetic images of
321 x 481 (cropped to 320 x 480 by crop_img), Gaussian noise sigma 25.
  (a) per image, as train_ddp.py:evaluate_tasks does without --data_root: upload, fwair.evaluate.tiled_restore (eager forward over the
      image's tiles), psnr and ssim with a host sync each;
  (b) fwair.evaluate.EvalEngine.run on the resident uint8 images: chunks of tiles, HIP-graph replay at a fixed batch, metrics on the device.
Each is the median of 5 repeats after one warm-up, torch.cuda.synchronize() around each repeat.  Prints one JSON line
(the record kept as profiles/r05_eval_rate.json).
  (c) `--restore`: EvalEngine with overlap=32, and with overlap=32, ensemble=True (fw_restore_gather / fw_restore_blend), next to (b):
      seconds, tiles and seconds per tile of each, and the summed time of the gather and blend launches as a share of the arm
      (the record kept as profiles/r12_restore_rate.json)."""
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
from fwair import augment as A              # noqa: E402
from fwair import evaluate as EV            # noqa: E402
from fwair.data import crop_img            # noqa: E402
from net.model import AirNet                # noqa: E402

dev = 'cuda'
opt = types.SimpleNamespace(L=3, encoder_dim=256, encoder_embed_dim=28, embed_dim=56, batch_size=16, patch_size=128,
                            degradation_embedding_method=['all_3_bands'], encoder_msa_type='freq', contrast_loss_weight=0.6,
                            encoder_type='Uformer', decoder_type='Uformer', debug_mode=False, frequency_decompose_type='none',
                            learnable_modulator=False, compute_dtype='bf16', de_type=['denoising_25'] * 16)
torch.manual_seed(0)
net = AirNet(opt).to(dev).eval()
rng = np.random.default_rng(68)
host = []
for _ in range(68):                                      # smooth content + grain, HWC like a decoded file, cropped as load_u8 crops
    yy, xx = np.mgrid[0:321, 0:481].astype(np.float32)
    ph = rng.uniform(0, 6.28, 3)
    img = np.stack([127 + 90 * np.sin(xx / (7 + c) + yy / (11 + 2 * c) + ph[c]) + rng.standard_normal((321, 481)) * 12 for c in range(3)], -1)
    host.append(np.ascontiguousarray(crop_img(np.clip(img, 0, 255).astype(np.uint8), 16).transpose(2, 0, 1)))
assert host[0].shape == (3, 320, 480)
n_tiles = sum(len(EV.tile_origins(h.shape[1], 128)) * len(EV.tile_origins(h.shape[2], 128)) for h in host)


def per_image():
    """The parent's way: one image at a time (train_ddp.py:evaluate_tasks)."""
    g = torch.Generator(device='cpu').manual_seed(4321)
    vals, svals = [], []
    with torch.no_grad():
        for h in host:
            cu8 = torch.from_numpy(h).to(dev)
            clean = cu8.float().div_(255.0)[None]
            deg = A.add_noise(cu8, 25, g).float().div_(255.0)
            rest = EV.tiled_restore(net, deg[None], 128)
            vals.append(EV.psnr(rest, clean)); svals.append(EV.ssim(rest, clean))
    return sum(vals) / len(vals), sum(svals) / len(svals)


resident = [torch.from_numpy(h).to(dev) for h in host]
engine = EV.EvalEngine(net, tile=128, tile_batch=64, use_graph=True)


def batched():
    p, s = engine.run(resident, sigma=25, seed=0)
    return float(p.mean()), float(s.mean())


def timed(fn):
    fn()                                                 # warm-up (graph capture, lazily built tables)
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts, out


def restore_arm(overlap, ensemble):
    """Arm (c): EvalEngine with overlapping tiles / the x8 self-ensemble (fw_restore_gather / fw_restore_blend).  -> seconds, tiles,
    seconds per tile, and the summed time of the gather and blend launches of the chunks (hipEvent pairs around each, one run on its
    own after the timed repeats) as a share of the arm."""
    eng = EV.EvalEngine(net, tile=128, tile_batch=64, use_graph=True, overlap=overlap, ensemble=ensemble)

    def run():
        p, s = eng.run(resident, sigma=25, seed=0)
        return float(p.mean()), float(s.mean())

    t, ts, (p, s) = timed(run)
    (plan,) = eng._plans.values()
    tiles = int(plan['ttab'].shape[0])
    pairs, real = [], EV.call

    def timed_call(name, *args):
        if name in ('fw_restore_gather', 'fw_restore_blend'):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            real(name, *args)
            b.record()
            pairs.append((name, a, b))
        else:
            real(name, *args)

    EV.call = timed_call
    try:
        run()
    finally:
        EV.call = real
    torch.cuda.synchronize()
    ms = {n: sum(a.elapsed_time(b) for m, a, b in pairs if m == n) for n in ('fw_restore_gather', 'fw_restore_blend')}
    return {'overlap': overlap, 'ensemble': ensemble, 'seconds': round(t, 4), 'repeats_s': [round(x, 4) for x in ts], 'tiles': tiles,
            'seconds_per_tile': round(t / tiles, 6), 'chunks': len(plan['chunks']), 'engine_graph': bool(eng.use_graph),
            'gather_ms': round(ms['fw_restore_gather'], 3), 'blend_ms': round(ms['fw_restore_blend'], 3),
            'gather_blend_share': round((ms['fw_restore_gather'] + ms['fw_restore_blend']) * 1e-3 / t, 5), 'psnr_ssim': [round(p, 3), round(s, 4)]}


if '--restore' in sys.argv[1:]:
    # the record kept as profiles/r12_restore_rate.json: arm (b) next to arm (c) at overlap 32, without and with the ensemble
    tb, tbs, (pb, sb) = timed(batched)
    print(json.dumps({'metric': 'seconds to evaluate one test set: 68 images of 320 x 480, sigma 25, bf16, tiles of 128',
                      'eval_engine': {'seconds': round(tb, 4), 'repeats_s': [round(t, 4) for t in tbs], 'tiles': n_tiles,
                                      'seconds_per_tile': round(tb / n_tiles, 6), 'psnr_ssim': [round(pb, 3), round(sb, 4)]},
                      'restore_overlap32': restore_arm(32, False), 'restore_overlap32_ensemble': restore_arm(32, True), 'tile_batch': 64,
                      'note': 'median of 5 repeats after one warm-up, synchronised around each repeat; gather_ms / blend_ms: hipEvent pairs '
                              'around the launches of one further run; untrained weights'}))
    sys.exit(0)

ta, tas, (pa, sa) = timed(per_image)
tb, tbs, (pb, sb) = timed(batched)
print(json.dumps({'metric': 'seconds to evaluate one test set: 68 images of 320 x 480, sigma 25, bf16, tiles of 128', 'tiles': n_tiles,
                  'per_image_s': round(ta, 4), 'eval_engine_s': round(tb, 4), 'ratio_per_image_over_engine': round(ta / tb, 3),
                  'per_image_repeats_s': [round(t, 4) for t in tas], 'eval_engine_repeats_s': [round(t, 4) for t in tbs],
                  'engine_graph': bool(engine.use_graph), 'tile_batch': 64,
                  'psnr_ssim_per_image': [round(pa, 3), round(sa, 4)], 'psnr_ssim_engine': [round(pb, 3), round(sb, 4)],
                  'note': 'median of 5 repeats after one warm-up, synchronised around each repeat; untrained weights (the two noise '
                          'draws differ: host generator vs in-kernel counter-based), so the PSNR / SSIM pairs agree only roughly'}))
