#!/usr/bin/env python3
"""LayerNorm backward at the model's shapes: microseconds per launch on cold operands (every repetition has its own buffers; all
repetitions run inside one captured graph, timed over replays), for dy given as bf16 and as a split-K slab of sk = 2, 3, 16 slices.

  bf16      fw_layernorm_bwd2 on a bf16 dy                                           (one launch)
  chain     fw_slab_reduce -> fw_cast_rows -> fw_layernorm_bwd2, timed as a chain    (three launches: what ops.dgrad + LN cost before)
  slab      fw_layernorm_bwd_slab on the unfolded slab                               (one launch; skipped if the library lacks the entry)

Every figure is measured --repeats times (the spread of a build against itself) and goes with a SHA-256 of dx and of twin of the
first repetition: seeded operands, so chain and slab -- and two builds that compute the same thing -- print the same hashes.

  --pkg DIR     the package tree whose libfwair_hip.so is measured (default: this checkout's); e.g. a build of the parent commit
  --json FILE   merge the rows into FILE under --label (two runs, parent and change, share one file)
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEEP = [(1024, 896), (4096, 896), (3072, 448), (4096, 448), (16384, 448), (12288, 224), (16384, 224), (65536, 224)]
CONTROLS = [(262144, 56), (786432, 28)]
SKS = (2, 3, 16)
dev, bf = 'cuda', torch.bfloat16


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def make_set(L, rows, C, mode, sk):
    """One repetition's buffers and the closure that launches it."""
    call, lib = L.call, L.lib()
    x = torch.randn(rows, C, device=dev)
    gamma = torch.randn(C, device=dev)
    mean = x.mean(1).contiguous()
    rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    dres = torch.randn(rows, C, device=dev)
    dx = torch.empty(rows, C, device=dev)
    twin = torch.empty(rows, C, device=dev, dtype=bf)
    nblk = lib.fw_layernorm_bwd_blocks(rows, C)
    partial = torch.empty(nblk, 2 * C, device=dev)
    S = (rows * C + 3) // 4 * 4
    if mode == 'bf16':
        dy = (torch.randn(rows, C, device=dev) * 0.5).to(bf)
    else:
        slab = torch.randn(sk, S, device=dev) * 0.5
        dy = torch.empty(rows, C, device=dev, dtype=bf)
        tmp = torch.empty(rows, C, device=dev)

    def bwd2():
        call('fw_layernorm_bwd2', 1, dy, C, x, C, gamma, mean, rstd, dres, C, dx, C, None, None, partial, rows, C, twin, C, None, 1)

    def chain():
        call('fw_slab_reduce', slab, sk, rows * C, S, tmp, 0, None, 0, 0)
        call('fw_cast_rows', 1, tmp, C, dy, C, rows, C, None, 1)
        bwd2()

    def fused():
        call('fw_layernorm_bwd_slab', 1, None, 0, slab, sk, S, x, C, gamma, mean, rstd, dres, C, dx, C, None, None, partial, rows, C,
             twin, C, None, 1)

    return {'bf16': bwd2, 'chain': chain, 'slab': fused}[mode], dx, twin


def measure(L, rows, C, mode, sk=0, repeats=3):
    """-> ([us per launch or chain, one per repeat], sha256 of dx, sha256 of twin)"""
    torch.manual_seed(rows + 1000 * C + sk)
    per = rows * C * (16 + 4 * sk)
    reps = max(8, min(32, (1 << 29) // per + 1))               # at least 512 MB of distinct operands between two uses of a buffer
    sets = [make_set(L, rows, C, mode, sk) for _ in range(reps)]
    side = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(side):
        for f, _, _ in sets:
            f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for f, _, _ in sets:
                f()
        g.replay()
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(3):
                g.replay()
            e1.record(side)
            torch.cuda.synchronize()
            out.append(round(e0.elapsed_time(e1) * 1e3 / (3 * reps), 2))
    return out, _sha(sets[0][1]), _sha(sets[0][2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pkg', default=os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
    ap.add_argument('--json', default=None)
    ap.add_argument('--label', default='change')
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from fwair import lib as L  # noqa: E402
    has_slab = 'fw_layernorm_bwd_slab' in L.protos()
    rows_out = []
    for rows, C in DEEP + CONTROLS:
        configs = [('bf16', 0)] + [(m, sk) for sk in SKS for m in (('chain', 'slab') if has_slab else ('chain',))]
        for mode, sk in configs:
            us, hdx, htw = measure(L, rows, C, mode, sk, args.repeats)
            by = rows * C * (16 + (4 * sk - 2 if mode == 'slab' else 0))
            print(f'rows={rows:7d} C={C:4d} {mode:5s} sk={sk:2d}  {min(us):8.2f} .. {max(us):8.2f} us  {by / min(us) / 1e6:5.2f} TB/s  '
                  f'dx {hdx[:12]} twin {htw[:12]}', flush=True)
            rows_out.append({'rows': rows, 'C': C, 'control': (rows, C) in CONTROLS, 'mode': mode, 'sk': sk, 'us': us,
                             'sha256_dx': hdx, 'sha256_twin': htw})
    if args.json:
        doc = json.load(open(args.json)) if os.path.exists(args.json) else {}
        doc[args.label] = rows_out
        with open(args.json, 'w') as f:
            json.dump(doc, f, indent=1)


if __name__ == '__main__':
    main()
