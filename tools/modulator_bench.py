#!/usr/bin/env python3
"""Cost of the decoder's learnable window modulator (--learnable_modulator; csrc/fw_norm.hip) -- bench.py pins the flag off, so this
tool measures it.  At the four decoder shapes of a batch of 16 at 128 x 128 (rows x C = 262144 x 112, 65536 x 224, 16384 x 448,
4096 x 896) and in both compute types:
  fwd   fw_layernorm_fwd against fw_layernorm_mod_fwd on the same x: the same bytes plus the L2-resident table
  bwd   fw_modulator_bwd (its fold included) against fw_layernorm_bwd (its fold included) on the same dy: the latter moves more
        bytes and is the project's tuned stream over the same rows -- compare bytes / s
and one whole eager training step (bf16, batch 16, 128 x 128) with the flag on and off, both engines alive in one process.
Device events around ~20 ms of back-to-back calls, median (min, max) of 9 windows after a warm-up, the two sides of a comparison
alternating window by window.  Bytes are those the algorithm must move, computed from the shapes below.
    python tools/modulator_bench.py [out.json]          (profiles/r11_modulator.json is one run of it)"""
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'))
from fwair import functional as Fn  # noqa: E402
from fwair.lib import call, dt, lib  # noqa: E402
from fwair.synthetic import synth_batch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('modulator_bench: no GPU -- a time is measured on the device or not at all')
dev = torch.device('cuda')
BATCH, SIDE = 16, 128
SHAPES = [(SIDE >> i, 112 << i) for i in range(4)]            # (H = W, C) of decoderlayer_0 .. decoderlayer_3


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # us per call


def measure(fns, reps=9, window_us=20e3, min_calls=5):
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


def entry(us, nbytes):
    return dict(us=round(us[0], 2), us_min_max=[round(us[1], 2), round(us[2], 2)], bytes=int(nbytes),
                tbytes_per_s=round(nbytes / (us[0] * 1e-6) / 1e12, 3))


def kernels():
    out = []
    for side, C in SHAPES:
        rows = BATCH * side * side
        x = torch.randn(rows, C, device=dev)
        g, b, table = torch.randn(C, device=dev), torch.randn(C, device=dev), torch.randn(64, C, device=dev)
        mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        dx = torch.empty(rows, C, device=dev)
        dg, db, dmod = torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(64, C, device=dev)
        nblk, nz = lib().fw_layernorm_bwd_blocks(rows, C), lib().fw_modulator_bwd_blocks(rows, C)
        p_ln = torch.empty(nblk, 2 * C, device=dev)
        p_mod = torch.empty(nz, 64 * C, device=dev)
        for dtype in (torch.float32, torch.bfloat16):
            es = 4 if dtype == torch.float32 else 2
            y = torch.empty(rows, C, dtype=dtype, device=dev)
            dy = torch.randn(rows, C, device=dev).to(dtype)
            fwd = measure({
                'plain': lambda: call('fw_layernorm_fwd', dt(dtype), x, C, g, b, y, C, mean, rstd, rows, C, 1e-5),
                'mod': lambda: call('fw_layernorm_mod_fwd', dt(dtype), x, C, g, b, table, y, C, mean, rstd, rows, C, side, side, 4, 1e-5)})
            bwd = measure({
                'ln': lambda: call('fw_layernorm_bwd', dt(dtype), dy, C, x, C, g, mean, rstd, None, 0, dx, C, dg, db, p_ln, rows, C),
                'mod': lambda: call('fw_modulator_bwd', dt(dtype), dy, C, dmod, p_mod, rows, C, side, side, 4)})
            stream = rows * C * (4 + es) + rows * 8                              # x in, y out, mean and rstd out
            ln_b = rows * C * (es + 4 + 4) + rows * 8 + 2 * nblk * 2 * C * 4 + 4 * C * 4   # dy, x in; dx out; statistics; partials out and back in
            mod_b = rows * C * es + 2 * nz * 64 * C * 4 + 2 * 64 * C * 4                 # dy in; slices out and back in; dmod read-modify-write
            r = dict(rows=rows, C=C, dtype=str(dtype).replace('torch.', ''), ln_blocks=nblk, mod_slices=nz,
                     fwd_plain=entry(fwd['plain'], stream), fwd_mod=entry(fwd['mod'], stream + 64 * C * 4),
                     bwd_layernorm=entry(bwd['ln'], ln_b), bwd_modulator=entry(bwd['mod'], mod_b))
            r['fwd_mod_over_plain'] = round(fwd['mod'][0] / fwd['plain'][0], 3)
            r['bwd_rate_mod_over_layernorm'] = round(r['bwd_modulator']['tbytes_per_s'] / r['bwd_layernorm']['tbytes_per_s'], 3)
            out.append(r)
            print(json.dumps(r), flush=True)
    return out


def whole_step():
    from fwair import engine as E
    from net.model import AirNet
    clean, xq, xk = synth_batch(BATCH, SIDE, 25, 1234, dev)
    engines = {}
    for flag in (False, True):
        torch.manual_seed(1234)
        opt = types.SimpleNamespace(L=3, encoder_dim=256, encoder_embed_dim=28, embed_dim=56, batch_size=BATCH, patch_size=SIDE,
                                    degradation_embedding_method=['all_3_bands'], encoder_msa_type='freq', contrast_loss_weight=0.6,
                                    encoder_type='Uformer', decoder_type='Uformer', debug_mode=False, frequency_decompose_type='none',
                                    learnable_modulator=flag, compute_dtype='bf16')
        net = AirNet(opt).to(dev).train()
        engines[flag] = E.TrainEngine(net, lr=2e-4, contrast_loss_weight=0.6, use_graph=False)
    try:
        res = measure({'off': lambda: engines[False].step_eager(xq, xk, clean), 'on': lambda: engines[True].step_eager(xq, xk, clean)},
                      reps=7, window_us=400e3, min_calls=3)
    finally:
        Fn.config.direct_grads = False
    r = dict(batch=BATCH, side=SIDE, dtype='bfloat16', mode='eager step, one engine per flag alive in one process',
             flag_off_ms=round(res['off'][0] / 1e3, 3), flag_off_ms_min_max=[round(v / 1e3, 3) for v in res['off'][1:]],
             flag_on_ms=round(res['on'][0] / 1e3, 3), flag_on_ms_min_max=[round(v / 1e3, 3) for v in res['on'][1:]])
    r['on_minus_off_ms'] = round(r['flag_on_ms'] - r['flag_off_ms'], 3)
    print(json.dumps(r), flush=True)
    return r


if __name__ == '__main__':
    record = dict(device=torch.cuda.get_device_name(0), kernels=kernels(), step=whole_step())
    print(json.dumps(record))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as f:
            json.dump(record, f, indent=1)
