#!/usr/bin/env python3
"""Time the band images (fwair.spectrum.band_images, N = 3 bands: csrc/fw_spec.hip fw_band_split, mode 0) at 96x96, 321x481,
320x480 with 68 maps, 512x512 and 1024x1024, against the same result from the FFT library on the same device:
  kernel     one band_images call: row pass, forward column pass (the half spectrum, written once), the inverse column pass of
             the three bands in one launch and their inverse row pass -- with Wq = W / 2 + 1 columns, H W Wq 2 + H^2 Wq 4 real
             multiply-adds forward and 3 (H^2 Wq 4 + H W Wq 2) inverse per map on the f32 MFMA (more where H or Wq is no multiple of
             64: the tile grid is padded); the call allocates its work buffer and output as a user's call does
  yardstick  F = torch.fft.fft2(x), then torch.fft.ifft2(F * mask_b).real for the three bands, stacked
Device events around ~50 ms of back-to-back calls, median of 9 such windows after a warm-up, the two paths alternating window by
window.  `us_per_image` = time of a call / nimg; `mfma_share` = the multiply-adds the maps need (unpadded) over the f32-MFMA peak
(157.3 TFLOP/s).      python tools/band_split_bench.py [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
from fwair import spectrum as S  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('band_split_bench: no GPU -- a time is measured on the device or not at all')
dev = torch.device('cuda')
PEAK = 157.3e12
SIZES = [(96, 96, 1), (321, 481, 1), (320, 480, 68), (512, 512, 1), (1024, 1024, 1)]
NB = 3


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
for h, w, n in SIZES:
    ring, nb = S.ring_table('bands', 1.0 / NB, h, w, dev)
    masks = torch.stack([(ring == b) for b in range(nb)]).float()                 # [bands, H, W], un-shifted
    x = torch.rand(n, h, w, device=dev)

    def kernel():
        return S.band_images(x, NB)

    def yardstick():
        F = torch.fft.fft2(x)
        return torch.stack([torch.fft.ifft2(F * masks[b]).real for b in range(nb)])

    res = measure({'kernel': kernel, 'yardstick': yardstick})
    out, ref = kernel(), yardstick()
    wq = w // 2 + 1
    macs = (2.0 * h * w * wq + 4.0 * h * h * wq) * (1 + nb) * n
    r = dict(H=h, W=w, nimg=n, bands=nb,
             kernel_us_per_image=round(res['kernel'][0] / n, 2), kernel_us_min_max=[round(v / n, 2) for v in res['kernel'][1:]],
             yardstick_us_per_image=round(res['yardstick'][0] / n, 2),
             yardstick_us_min_max=[round(v / n, 2) for v in res['yardstick'][1:]],
             yardstick_over_kernel=round(res['yardstick'][0] / res['kernel'][0], 2),
             mfma_share=round(2 * macs / (res['kernel'][0] * 1e-6) / PEAK, 3),
             max_diff_rel_to_max=float((out - ref).abs().max() / ref.abs().max()))       # both are f32 chains: not a reference check
    rows.append(r)
    print(r, flush=True)

res = dict(device=torch.cuda.get_device_name(0), peak_f32_mfma_tflops=PEAK / 1e12, bands=NB, rows=rows)
print(json.dumps(res))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, indent=1)
