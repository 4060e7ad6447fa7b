#!/usr/bin/env python3
"""Tall-skinny GEMM shapes of the C <= 112 stages (gemm_stream_kernel): time per launch on cold operands (8 sets in a captured graph),
TB/s of algorithmic bytes, and a SHA-256 of the first set's output (seeded operands: two builds that compute the same thing print
the same hashes).

  --pkg DIR     the package tree whose libfwair_hip.so is measured (default: this checkout's); e.g. a build of the parent commit
  --json FILE   also write the rows as JSON, labelled --label

The switch that skips the epilogue's stores (FW_GEMM_BIG_DBG=1: what is left is loads + MFMA) is compiled into this kernel only
with -DFW_STREAM_DBG (HIPCC flags in build.sh); such a build sends every launch through the kernel's generic loop."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--pkg', default=os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
ap.add_argument('--json', default=None)
ap.add_argument('--label', default='')
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg))
from fwair import ops  # noqa: E402

dev, bf = 'cuda', torch.bfloat16
SHAPES = [(786432, 88, 28, 'plain'), (786432, 112, 28, 'plain'), (786432, 28, 112, 'res'), (262144, 168, 56, 'plain'), (262144, 224, 56, 'plain'),
          (262144, 56, 224, 'res'), (262144, 448, 112, 'plain'), (262144, 336, 112, 'plain'), (196608, 224, 56, 'plain'),
          (786432, 28, 88, 'dplain'), (786432, 28, 112, 'dgelu_in'), (262144, 112, 448, 'dgelu'), (262144, 56, 224, 'dgelu')]


def ld8(n):
    return (n + 7) // 8 * 8


def run(M, N, K, kind, reps=8):
    torch.manual_seed(M + 1000 * N + K)
    sets, outs = [], []
    for _ in range(reps):
        if kind in ('plain', 'res'):
            x = (torch.randn(M, ld8(K), device=dev) * 0.5).to(bf)[:, :K]
            w = (torch.randn(N, ld8(K), device=dev) * 0.05).to(bf)[:, :K]
            b = torch.randn(N, device=dev)
            if kind == 'res':
                res = torch.randn(M, N, device=dev)
                y = torch.empty(M, N, device=dev)
                sets.append(lambda x=x, w=w, b=b, y=y, res=res: ops.gemm(x, w, M, N, K, out=y, bias=b, residual=res))
                outs.append(y)
            else:
                y = torch.empty(M, ld8(N), device=dev, dtype=bf)[:, :N]
                sets.append(lambda x=x, w=w, b=b, y=y: ops.gemm(x, w, M, N, K, out=y, bias=b))
                outs.append(y)
        else:
            dy = (torch.randn(M, ld8(K), device=dev) * 0.5).to(bf)[:, :K]
            w = (torch.randn(K, ld8(N), device=dev) * 0.05).to(bf)[:, :N]
            out = torch.empty(M, ld8(N), device=dev, dtype=bf)[:, :N]
            aux = torch.randn(M, ld8(N), device=dev).to(bf)[:, :N] if kind.startswith('dgelu') else None
            sets.append(lambda dy=dy, w=w, out=out, aux=aux: ops.gemm(dy, w, M, N, K, w_trans=True, out=out, act=2 if aux is not None else 0, aux=aux))
            outs.append(out)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for f in sets:
            f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for f in sets:
                f()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        for _ in range(3):
            g.replay()
        e1.record(side)
        torch.cuda.synchronize()
    digest = hashlib.sha256(outs[0].contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
    return e0.elapsed_time(e1) * 1e-3 / (3 * reps), digest


if __name__ == '__main__':
    tot, rows = 0.0, []
    for M, N, K, kind in SHAPES:
        t, digest = run(M, N, K, kind)
        tot += t
        by = M * K * 2 + (M * N * 4 * 2 if kind == 'res' else M * N * 2) + (M * N * 2 if kind.startswith('dgelu') else 0)
        print(f'{kind:9s} M={M:7d} N={N:4d} K={K:4d}  {t * 1e6:8.1f} us  {by / t / 1e12:5.2f} TB/s  {digest[:16]}', flush=True)
        rows.append({'kind': kind, 'M': M, 'N': N, 'K': K, 'us': round(t * 1e6, 2), 'tb_per_s': round(by / t / 1e12, 3), 'sha256': digest})
    print(f'sum {tot * 1e6:.1f} us')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'label': args.label, 'sum_us': round(tot * 1e6, 1), 'shapes': rows}, f, indent=1)
