#!/usr/bin/env python3
"""Time the ViT global attention at N = 256 tokens with and without the band re-weighting on the N x N grid (`--vit_band_grid tokens`):
us per forward / backward launch group for lamb = None, 'DC' (affine form) and '3_bands' (row / column / output DFT passes), bf16,
at B * heads = 48 and 192, and the f32-MFMA rate of the filter (0.40 GFLOP per map forward: 2 + 4 + 4 + 2 real 256^3 products;
backward 0.60: one more row pass and half a column pass for the spectrum of P).   python tools/gattn_bands_bench.py [out.json]
`--tokens 576` / `--tokens 1024` (384x384 / 512x512 inputs) time the tiled passes behind the same entry pair (fw_gattn_bands_fwd / bwd) the same way, at
B * heads = 24 and 96 / 12 and 48 maps, with 12 N^3 (forward) and 18 N^3 (backward) multiply-adds per map."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
from fwair import vit as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('out', nargs='?')
ap.add_argument('--tokens', type=int, default=256, choices=[256, 576, 1024])
args = ap.parse_args()
dev, dtype, N, heads = torch.device('cuda'), torch.bfloat16, args.tokens, 12
PEAK = 157.3e12
BATCHES = {256: (4, 16), 576: (2, 8), 1024: (1, 4)}[N]
FWD_FLOP, BWD_FLOP = (0.4027e9, 0.6040e9) if N == 256 else (24.0 * N ** 3, 36.0 * N ** 3)


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


rows = []
for B in BATCHES:
    qkv = (torch.randn(B * N, 3 * heads * 64, device=dev) * 0.8).to(dtype).requires_grad_(True)
    dout = (torch.randn(B * N, heads * 64, device=dev) * 0.5).to(dtype)
    base = {}
    for kind in ('none', 'DC', '3_bands'):
        nb = {'none': 0, 'DC': 2, '3_bands': 3}[kind]
        lamb = torch.nn.Parameter(torch.randn(nb, 1, heads, device=dev) * 0.3) if nb else None
        spec = V._spectral_tables('bands', 3, dev, n=N) if kind == '3_bands' else None
        meta = (B, N, heads, 0.1, 7, spec)
        fwd = lambda: V.GlobalAttnFn.apply(qkv, lamb, meta)
        with torch.no_grad():
            tf = timeit(fwd)

        def both():
            qkv.grad = None
            fwd().backward(dout)
        tb = timeit(both) - tf
        r = dict(kind=kind, maps=B * heads, fwd_us=round(tf, 1), bwd_us=round(tb, 1))
        if kind == 'none':
            base = r
        else:
            r['fwd_vs_none'] = round(tf / base['fwd_us'], 3)
            r['bwd_vs_none'] = round(tb / base['bwd_us'], 3)
        if kind == '3_bands':                                    # the filter's share: time over the lamb = None kernels, exact-f32 MFMA FLOPs
            maps = B * heads
            r['filter_fwd_tflops'] = round(FWD_FLOP * maps / ((tf - base['fwd_us']) * 1e-6) / 1e12, 1)
            r['filter_bwd_tflops'] = round(BWD_FLOP * maps / ((tb - base['bwd_us']) * 1e-6) / 1e12, 1)
            r['f32_mfma_peak_tflops'] = PEAK / 1e12
        rows.append(r)
        print(r)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), dtype='bf16', N=N, drop_p=0.1, rows=rows), f, indent=1)
