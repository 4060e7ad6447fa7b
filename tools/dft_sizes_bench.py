#!/usr/bin/env python3
"""Time the band decomposition on the tiled f32-MFMA passes (csrc/fw_dft.hip) at N = 256, 384, 512 and nimg = 48 maps:
  decompose      the whole `frequency_decompose_1`, size 0.5 (3 bands: DC as the mean, one masked inverse, the last by subtraction):
                 2 + 4 + 4 + 2 real N^3 products = 24 N^3 FLOP per map
  spectrum_pairs the spectrum + `frequency_decompose`, size 1/3, mode 1 ((re, im) pairs of the masked spectrum): 2 + 4 products
                 = 12 N^3 FLOP per map, plus one element-wise pass
and, at N = 256 only, the same two on the existing kernels (fw_dft2_fwd + fw_dft2_bands + fw_band_residual), which this file's
subject does not touch.  Device events around ~50 ms of back-to-back calls, median of 9 such windows after a warm-up; at 256 the
two paths alternate window by window.  `peak_share` = FLOP / time over the f32-MFMA peak (157.3 TFLOP/s): the passes are bound
by that rate, not by bytes (24 N^3 FLOP against ~64 N^2 bytes per map).      python tools/dft_sizes_bench.py [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
from fwair import lfs  # noqa: E402
from fwair.lib import call  # noqa: E402
from net.utils.frequency_decompose import _dft_panels  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('dft_sizes_bench: no GPU -- a time is measured on the device or not at all')
dev = torch.device('cuda')
PEAK = 157.3e12
NIMG = 48


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # us per call


def measure(fns, reps=9, window_us=50e3):
    """fns: {name: callable}; windows of ~50 ms alternate between them.  -> {name: (median us, min us, max us)}"""
    calls = {}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(5, int(window_us / window(fn, 5)))
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(window(fn, calls[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def masks(kind, size, N):
    m = torch.stack(lfs.band_masks_shifted(kind, size, N, N)).float()
    return torch.fft.ifftshift(m, dim=(-2, -1)).contiguous().to(dev)


rows = []
for N in (256, 384, 512):
    n = NIMG
    x = torch.randn(n, N, N, device=dev)
    pn = _dft_panels(N, dev)
    m1, m3 = masks('frequency_decompose_1', 0.5, N), masks('frequency_decompose', 1 / 3., N)
    nb1, nb3 = m1.shape[0], m3.shape[0]
    out = torch.empty(nb1, n, N, N, device=dev)
    pairs = torch.empty(nb3, n, N, N, 2, device=dev)
    fr, fi = torch.empty(n, N, N, device=dev), torch.empty(n, N, N, device=dev)
    work = torch.empty((2 + 2 * nb1) * n * N * N, device=dev)

    def tiled_decompose():
        call('fw_dft2t_decompose', x, m1, pn, work, out, n, N, nb1, 1)

    def tiled_pairs():
        call('fw_dft2t_fwd', x, pn, work, fr, fi, n, N)
        call('fw_dft2t_bands', fr, fi, m3, None, None, pairs, n, N, nb3, 1)

    jobs = {'decompose': {'tiled': tiled_decompose}, 'spectrum_pairs': {'tiled': tiled_pairs}}
    if N == 256:
        out0, pairs0 = torch.empty_like(out), torch.empty_like(pairs)

        def old_decompose():
            call('fw_dft2_fwd', x, fr, fi, n, N)
            call('fw_dft2_bands', fr, fi, m1, out0, n, N, nb1 - 1, 0)
            call('fw_band_residual', x, out0, n, N, nb1)

        def old_pairs():
            call('fw_dft2_fwd', x, fr, fi, n, N)
            call('fw_dft2_bands', fr, fi, m3, pairs0, n, N, nb3, 1)

        jobs['decompose']['existing'] = old_decompose
        jobs['spectrum_pairs']['existing'] = old_pairs
    for job, fns in jobs.items():
        flop = (24 if job == 'decompose' else 12) * float(N) ** 3 * n
        res = measure(fns)
        r = dict(job=job, N=N, nimg=n, tiled_us=round(res['tiled'][0], 1), tiled_us_min_max=[round(res['tiled'][1], 1), round(res['tiled'][2], 1)],
                 tiled_tflops=round(flop / (res['tiled'][0] * 1e-6) / 1e12, 1), peak_share=round(flop / (res['tiled'][0] * 1e-6) / PEAK, 3))
        if 'existing' in res:
            r.update(existing_us=round(res['existing'][0], 1), existing_us_min_max=[round(res['existing'][1], 1), round(res['existing'][2], 1)],
                     existing_over_tiled=round(res['existing'][0] / res['tiled'][0], 2))
            a, b = (out, out0) if job == 'decompose' else (pairs, pairs0)
            r['max_diff_rel_to_max'] = float((a - b).abs().max() / b.abs().max())      # same inputs, both paths (f32 sums reordered)
        rows.append(r)
        print(r, flush=True)

res = dict(device=torch.cuda.get_device_name(0), peak_f32_mfma_tflops=PEAK / 1e12, rows=rows)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, indent=1)
