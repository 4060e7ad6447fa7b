#!/usr/bin/env python3
"""Time the band statistics (csrc/fw_spec.hip: fw_band_stats, five 'plot' rings) at 128x128, 320x480, 321x481, 512x512 and 1024x1024
with nimg = 1 and 68 maps and power = 0 and 1, against the same result from the FFT library on the same device:
  kernel     one fw_band_stats call: row pass, column pass with the band reduction in its epilogue, fold -- half the spectrum of
             a real map, so H W^2 + 2 H^2 W real multiply-adds per map on the f32 MFMA (more where H or W / 2 + 1 is no multiple of
             64: the tile grid is padded), no spectrum written
  yardstick  torch.fft.fft2(x).abs() (squared for power 1), then the masked sum as one product [n, H W] x [H W, bands]
Device events around ~50 ms of back-to-back calls, median of 9 such windows after a warm-up, the two paths alternating window by
window.  `us_per_image` = time of a call / nimg; `mfma_share` = the multiply-adds the maps need (unpadded) over the f32-MFMA peak
(157.3 TFLOP/s) -- what the padding and the epilogue cost shows there.      python tools/band_stats_bench.py [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
from fwair import spectrum as S  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('band_stats_bench: no GPU -- a time is measured on the device or not at all')
dev = torch.device('cuda')
PEAK = 157.3e12
SIZES = [(128, 128), (320, 480), (321, 481), (512, 512), (1024, 1024)]
NB = 5


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


rows = []
for h, w in SIZES:
    ring, nb = S.ring_table('plot', 1.0 / NB, h, w, dev)
    onehot = torch.stack([(ring == b) for b in range(nb)]).float().view(nb, h * w).t().contiguous()     # [H W, bands], un-shifted
    ph, pw = S.panels(h, dev), S.panels(w, dev)
    for n in (1, 68):
        x = torch.rand(n, h, w, device=dev) * 255
        out = torch.empty(n, nb, dtype=torch.float64, device=dev)
        work = torch.empty(S.work_floats(n, h, w, nb), device=dev)
        for power in (0, 1):
            def kernel():
                S.call('fw_band_stats', 0, x, None, ring, ph, pw, work, out, n, h, w, nb, power)

            def yardstick():
                m = torch.fft.fft2(x).abs()
                if power:
                    m = m * m
                return m.view(n, h * w) @ onehot

            res = measure({'kernel': kernel, 'yardstick': yardstick})
            kernel()
            ref = yardstick().double()
            macs = (1.0 * h * w * w + 2.0 * h * h * w) * n
            r = dict(H=h, W=w, nimg=n, power=power,
                     kernel_us_per_image=round(res['kernel'][0] / n, 2), kernel_us_min_max=[round(v / n, 2) for v in res['kernel'][1:]],
                     yardstick_us_per_image=round(res['yardstick'][0] / n, 2),
                     yardstick_us_min_max=[round(v / n, 2) for v in res['yardstick'][1:]],
                     yardstick_over_kernel=round(res['yardstick'][0] / res['kernel'][0], 2),
                     mfma_share=round(2 * macs / (res['kernel'][0] * 1e-6) / PEAK, 3),
                     max_band_diff_rel=float(((out - ref).abs() / ref.abs()).max()))       # both are f32 chains: not a reference check
            rows.append(r)
            print(r, flush=True)

res = dict(device=torch.cuda.get_device_name(0), peak_f32_mfma_tflops=PEAK / 1e12, bands=NB, rows=rows)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, indent=1)
