#!/usr/bin/env python3
"""Cost of the decoder width (--embed_dim 32 / 56 / 64; head_dim of the decoder's window attention = embed_dim, csrc/fw_attn.hip) --
bench.py pins the width at 56, so this tool measures the other two next to it.  One whole training step (bf16, batch 16, 128 x 128,
all_3_bands) per width, the three engines alive in one process: first eager (one launch after the other from the host, as
tools/modulator_bench.py times its step), then replayed from the engine's captured graph (what train_ddp.py and bench.py run).  Device
events around ~400 ms of back-to-back steps, median (min, max) of 7 windows after a warm-up, the widths alternating window by window.
First measurements: nothing is gated on them.
    python tools/width_bench.py [out.json]          (the `widths_*` entries of profiles/r13_decoder_widths.json are one run of it)"""
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
from fwair import functional as Fn  # noqa: E402
from fwair.synthetic import synth_batch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('width_bench: no GPU -- a time is measured on the device or not at all')
dev = torch.device('cuda')
BATCH, SIDE = 16, 128
WIDTHS = (32, 56, 64)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # us per call


def measure(fns, reps=7, window_us=400e3, min_calls=3):
    """fns: {name: callable}; windows alternate between them.  -> {name: (median us, min us, max us)}"""
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


def whole_step(graph):
    from fwair import engine as E
    from net.model import AirNet
    clean, xq, xk = synth_batch(BATCH, SIDE, 25, 1234, dev)
    engines, params = {}, {}
    for width in WIDTHS:
        torch.manual_seed(1234)
        opt = types.SimpleNamespace(L=3, encoder_dim=256, encoder_embed_dim=28, embed_dim=width, batch_size=BATCH, patch_size=SIDE,
                                    degradation_embedding_method=['all_3_bands'], encoder_msa_type='freq', contrast_loss_weight=0.6,
                                    encoder_type='Uformer', decoder_type='Uformer', debug_mode=False, frequency_decompose_type='none',
                                    learnable_modulator=False, compute_dtype='bf16')
        net = AirNet(opt).to(dev).train()
        params[width] = sum(p.numel() for p in net.R.parameters())
        engines[width] = E.TrainEngine(net, lr=2e-4, contrast_loss_weight=0.6, use_graph=graph)
    try:
        res = measure({w: (lambda e=engines[w]: (e.step if graph else e.step_eager)(xq, xk, clean)) for w in WIDTHS})
    finally:
        Fn.config.direct_grads = False
    r = dict(batch=BATCH, side=SIDE, dtype='bfloat16', mode=('graph replay' if graph else 'eager step') + ', one engine per width alive in one process')
    for w in WIDTHS:
        r[f'w{w}'] = dict(decoder_params_m=round(params[w] / 1e6, 1), step_ms=round(res[w][0] / 1e3, 3),
                          step_ms_min_max=[round(v / 1e3, 3) for v in res[w][1:]])
    r['w32_over_w56'] = round(res[32][0] / res[56][0], 3)
    r['w64_over_w56'] = round(res[64][0] / res[56][0], 3)
    print(json.dumps(r), flush=True)
    return r


if __name__ == '__main__':
    record = dict(device=torch.cuda.get_device_name(0), widths_eager=whole_step(False), widths_graph=whole_step(True))
    print(json.dumps(record))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as f:
            json.dump(record, f, indent=1)
