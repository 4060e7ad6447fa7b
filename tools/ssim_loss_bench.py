#!/usr/bin/env python3
"""Cost of the SSIM loss term (--ssim_loss_weight; csrc/fw_loss.hip) -- bench.py runs with the term off, so this tool measures it.
  kernels  fw_ssim11_loss (value + gradient accumulated into da, as the training step calls it) next to fw_l1_loss on the same images, at
           16 x 3 x 128 x 128 (the step's loss input) and 1 x 3 x 512 x 512: device events around ~20 ms of back-to-back calls, median
           (min, max) of 9 windows after a warm-up, the two kernels alternating window by window.  Bytes are those the algorithm must
           move (a, b in, da out; the SSIM call reads da as well).
  step     one training step at bench.py's default configuration (bf16, batch 16, 128 x 128, HIP-graph replay) with the term off and with
           weight 0.2: each measurement in a fresh child process (20 warm-up steps, then 9 windows of 20 steps between device events),
           the two settings alternating, `--rounds` children each.
  parent   with `--parent DIR` (a built checkout of the parent commit): `bench.py --gpus 1 --steps 100 --warmup 20` of DIR and of this
           tree, alternating, `--rounds` runs each -- the term-off step against the commit before.
    python tools/ssim_loss_bench.py [--parent DIR] [--rounds 3] [out.json]      (profiles/r21_ssim_loss.json is one run of it)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
BATCH, SIDE, WEIGHT = 16, 128, 0.2
SHAPES = [(16, 3, 128, 128), (1, 3, 512, 512)]


def window(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # us per call


def measure(fns, reps=9, window_us=20e3, min_calls=5):
    """fns: {name: callable}; windows alternate between them.  -> {name: (median us, min us, max us)}"""
    import torch
    calls = {}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(min_calls, int(window_us / window(fn, min_calls)))
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(window(fn, calls[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def entry(us, nbytes):
    return dict(us=round(us[0], 2), us_min_max=[round(us[1], 2), round(us[2], 2)], bytes=int(nbytes),
                tbytes_per_s=round(nbytes / (us[0] * 1e-6) / 1e12, 3))


def kernels():
    import torch
    from fwair.lib import call
    dev = torch.device('cuda')
    out = []
    for n, C, H, W in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        b = torch.rand(n, C, H, W, device=dev, generator=g)
        a = (b + 0.1 * torch.randn(n, C, H, W, device=dev, generator=g)).contiguous()
        da = torch.zeros_like(a)
        loss = torch.zeros(2, device=dev)
        N = a.numel()
        res = measure({'l1': lambda: call('fw_l1_loss', a, b, da, N, 1.0, loss[0:1]),
                       'ssim': lambda: call('fw_ssim11_loss', a, b, da, n, C, H, W, -WEIGHT, 1, loss[1:2])})
        tiles = n * C * ((H + 31) // 32) * ((W + 31) // 32)
        r = dict(shape=[n, C, H, W], workgroups=tiles, fw_l1_loss=entry(res['l1'], 3 * N * 4), fw_ssim11_loss=entry(res['ssim'], 4 * N * 4))
        r['ssim_over_l1'] = round(res['ssim'][0] / res['l1'][0], 2)
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def child_step(weight):
    """bench.py's default engine (bf16, batch 16, 128 x 128, graph replay) with the given SSIM weight -> one JSON line of window times."""
    import torch
    from fwair import engine as E
    from fwair.synthetic import synth_batch
    from net.model import AirNet
    dev = torch.device('cuda')
    torch.manual_seed(1234)
    opt = types.SimpleNamespace(L=3, encoder_dim=256, encoder_embed_dim=28, embed_dim=56, batch_size=BATCH, patch_size=SIDE,
                                degradation_embedding_method=['all_3_bands'], encoder_msa_type='freq', contrast_loss_weight=0.6,
                                encoder_type='Uformer', decoder_type='Uformer', debug_mode=False, frequency_decompose_type='none',
                                learnable_modulator=False, compute_dtype='bf16')
    net = AirNet(opt).to(dev).train()
    eng = E.TrainEngine(net, lr=2e-4, contrast_loss_weight=0.6, use_graph=True, ssim_loss_weight=weight)
    clean, xq, xk = synth_batch(BATCH, SIDE, 25, 1234, dev)
    for _ in range(20):
        out = eng.step(xq, xk, clean)
    torch.cuda.synchronize()
    t = [window(lambda: eng.step(xq, xk, clean), 20) / 1e3 for _ in range(9)]          # ms per step
    print(json.dumps(dict(weight=weight, ms=round(statistics.median(t), 3), ms_min_max=[round(min(t), 3), round(max(t), 3)],
                          loss=[round(float(v), 6) for v in out], ssim=None if eng.ssim is None else round(float(eng.ssim), 6))), flush=True)


def last_json(text):
    for line in reversed(text.splitlines()):
        if line.startswith('{'):
            return json.loads(line)
    raise RuntimeError('no JSON line in:\n' + text[-2000:])


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), runs=[round(x, 3) for x in v])


def whole_step(rounds):
    runs = {0.0: [], WEIGHT: []}
    last = {}
    for _ in range(rounds):
        for w in runs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(w)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f'child (weight {w}) failed with {r.returncode}:\n' + r.stderr[-3000:])
            last[w] = last_json(r.stdout)
            runs[w].append(last[w]['ms'])
            print(json.dumps(last[w]), flush=True)
    off, on = spread(runs[0.0]), spread(runs[WEIGHT])
    r = dict(batch=BATCH, side=SIDE, dtype='bfloat16', mode='graph replay, a fresh process per measurement, settings alternating',
             weight=WEIGHT, flag_off_ms=off, flag_on_ms=on, on_minus_off_ms=round(on['median'] - off['median'], 3),
             window_min_max_of_last_runs={'off': last[0.0]['ms_min_max'], 'on': last[WEIGHT]['ms_min_max']},
             loss_on=last[WEIGHT]['loss'], ssim_on=last[WEIGHT]['ssim'], loss_off=last[0.0]['loss'])
    print(json.dumps(r), flush=True)
    return r


def against_parent(parent, rounds):
    runs = {'parent': [], 'this': []}
    for _ in range(rounds):
        for k, root in (('parent', parent), ('this', ROOT)):
            r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '100', '--warmup', '20'], cwd=root,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f'bench.py of {k} failed with {r.returncode}:\n' + r.stderr[-3000:])
            runs[k].append(last_json(r.stdout)['ms_per_step'])
            print(json.dumps({k: runs[k][-1]}), flush=True)
    r = dict(cmd='bench.py --gpus 1 --steps 100 --warmup 20', parent_ms=spread(runs['parent']), this_flag_off_ms=spread(runs['this']))
    r['this_minus_parent_ms'] = round(r['this_flag_off_ms']['median'] - r['parent_ms']['median'], 3)
    print(json.dumps(r), flush=True)
    return r


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit: compare bench.py of both')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('out', nargs='?')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('ssim_loss_bench: no GPU -- a time is measured on the device or not at all')
    if args.child is not None:
        child_step(args.child)
        sys.exit(0)
    record = dict(device=torch.cuda.get_device_name(0))
    # the children and bench.py runs first, while this process has not opened the device for work of its own
    record['step'] = whole_step(args.rounds)
    if args.parent:
        record['parent'] = against_parent(os.path.abspath(args.parent), args.rounds)
    record['kernels'] = kernels()
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
