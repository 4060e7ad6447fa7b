#!/usr/bin/env python3
"""Time the ViT global attention at N = 256 (the register kernel: the yardstick), 576 and 1024 tokens (the streaming forward and the
backward body with a run-time tile count): us per forward and per backward launch group, bf16, Dropout p = 0.1, at B * heads = 48 and
192, with the MFMA rate counted as 4 N^2 64 FLOPs per (image, head) forward (Q K^T and P V) and 10 N^2 64 backward (five products),
and us / (B heads N^2) of every size relative to N = 256 in the same session.  Device events around `reps` calls after a warm-up of
every shape; each figure is the median of `rounds` such windows.   python tools/gattn_stream_bench.py [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
from fwair import vit as V  # noqa: E402

dev, dtype, heads = torch.device('cuda'), torch.bfloat16, 12
PEAK_BF16 = 2.5e15                                                # dense bf16 MFMA, MI355X (specification)


def timeit(fn, reps=50, rounds=5):
    for _ in range(5):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return statistics.median(out), (max(out) - min(out)) / statistics.median(out)


rows, base = [], {}
for B in (4, 16):
    for N in (256, 576, 1024):
        maps = B * heads
        qkv = (torch.randn(B * N, 3 * heads * 64, device=dev) * 0.8).to(dtype).requires_grad_(True)
        dout = (torch.randn(B * N, heads * 64, device=dev) * 0.5).to(dtype)
        meta = (B, N, heads, 0.1, 7, None)
        fwd = lambda: V.GlobalAttnFn.apply(qkv, None, meta)
        with torch.no_grad():
            tf, sf = timeit(fwd)

        def both():
            qkv.grad = None
            fwd().backward(dout)
        tfb, sb = timeit(both)
        tb = tfb - tf
        r = dict(N=N, maps=maps, kernel='register' if N == 256 else 'stream', fwd_us=round(tf, 1), bwd_us=round(tb, 1),
                 fwd_spread=round(sf, 3), fwd_bwd_spread=round(sb, 3),
                 fwd_tflops=round(4.0 * N * N * 64 * maps / (tf * 1e-6) / 1e12, 1),
                 bwd_tflops=round(10.0 * N * N * 64 * maps / (tb * 1e-6) / 1e12, 1))
        r['fwd_ps_per_score'] = round(tf * 1e6 / (maps * N * N), 3)       # us / (B heads N^2), in picoseconds
        r['bwd_ps_per_score'] = round(tb * 1e6 / (maps * N * N), 3)
        if N == 256:
            base[maps] = r
        r['fwd_per_score_vs_256'] = round(r['fwd_ps_per_score'] / base[maps]['fwd_ps_per_score'], 3)
        r['bwd_per_score_vs_256'] = round(r['bwd_ps_per_score'] / base[maps]['bwd_ps_per_score'], 3)
        rows.append(r)
        print(r, flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), dtype='bf16', heads=heads, drop_p=0.1, bf16_mfma_peak_tflops=PEAK_BF16 / 1e12,
                       flops='4 N^2 64 per (image, head) forward, 10 N^2 64 backward', rows=rows), f, indent=1)
