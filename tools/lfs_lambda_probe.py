#!/usr/bin/env python3
"""Do the lambda-head kernels wait for their scattered parameters?  fw_lfs_lambda and fw_lfs_lambda_bwd at the bench geometry
(44 blocks, B = 16, C = 448, two bands), timed alone between events with the L2 flushed before every call, once with the 704
parameter / gradient tensors packed into one 4 MB buffer and once spread evenly over a 1 GiB buffer.

    python tools/lfs_lambda_probe.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
import torch                                  # noqa: E402
from fwair.lib import call                    # noqa: E402

DEV = 'cuda'
B, C, nb1 = 16, 448, 2
heads_list = [1] * 4 + [2] * 8 + [4] * 8 + [8] * 8 + [16] * 8 + [8] * 4 + [4] * 4     # 44 blocks
nblk = len(heads_list)
flush = torch.empty(256 << 20, dtype=torch.float32, device=DEV)


def tables(buf, gbuf, scatter):
    ptab, gtab = [], []
    n = buf.numel()
    o, k, ntens = 0, 0, nblk * 2 * 8
    for h in heads_list:
        for band in range(2):
            for shp in [(C,), (C,), (h, C), (h,), (h, h), (h,), (h, h), (h,)]:
                sz = 1
                for s in shp:
                    sz *= s
                if scatter:
                    o = (k * (n // ntens)) // 4 * 4
                ptab.append(buf.data_ptr() + 4 * o); gtab.append(gbuf.data_ptr() + 4 * o)
                o += (sz + 3) // 4 * 4
                k += 1
    return torch.tensor(ptab, dtype=torch.int64, device=DEV), torch.tensor(gtab, dtype=torch.int64, device=DEV)


def run(name, buf, gbuf, scatter):
    ptab, gtab = tables(buf, gbuf, scatter)
    heads = torch.tensor(heads_list, dtype=torch.int32, device=DEV)
    offs = [0]
    for h in heads_list:
        offs.append(offs[-1] + B * h * 3)
    coef_off = torch.tensor(offs[:-1], dtype=torch.int64, device=DEV)
    coef = torch.zeros(offs[-1], device=DEV); dcoef = torch.randn(offs[-1], device=DEV)
    save = torch.zeros(nblk, 2, B, 16, 3, device=DEV)
    xbar = torch.randn(nb1 * B, C, device=DEV); dxbar = torch.zeros_like(xbar)
    tf, tb = [], []
    for it in range(12):
        for which in (0, 1):
            flush.fill_(1.0)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            if which == 0:
                call('fw_lfs_lambda', xbar, ptab, heads, coef_off, coef, save, nblk, B, C, nb1)
            else:
                call('fw_lfs_lambda_bwd', xbar, ptab, gtab, heads, coef_off, dcoef, save, dxbar, nblk, B, C, nb1)
            e.record()
            torch.cuda.synchronize()
            (tf if which == 0 else tb).append(s.elapsed_time(e) * 1e3)
    tf, tb = sorted(tf[2:]), sorted(tb[2:])
    print(f'{name}: lambda median {tf[len(tf) // 2]:.1f} us (min {tf[0]:.1f}), lambda_bwd median {tb[len(tb) // 2]:.1f} us (min {tb[0]:.1f})', flush=True)


small = torch.randn(1 << 20, device=DEV) * 0.1
gsmall = torch.zeros(1 << 20, device=DEV)
big = torch.randn(256 << 20, device=DEV) * 0.1
gbig = torch.zeros(256 << 20, device=DEV)
run('packed   ', small, gsmall, False)
run('scattered', big, gbig, True)
run('packed   ', small, gsmall, False)
run('scattered', big, gbig, True)
