"""What tests/test_modulator_cpu.py and tests/test_modulator_gpu.py share: the shapes, the unit-variance tables, the window position
of a token row (the index formula of include/fwair.h), the torch restatement of the reference's window add, and the wrong
expectations the kernel tests must tell from the right one."""
import json
import os

import torch

import airnet_oracle as O
from helpers import GOLDEN, U32, UBF

B = 2
GEOS = [(16, 24), (24, 16)]                   # H != W tells a swapped axis apart
SHIFTS = [0, 4]
WIDTHS = [28, 112, 224, 448, 896]             # the four decoder widths and one narrow row
INDEX_CASES = [(16, 24, 0), (16, 24, 4), (24, 16, 4)]
MIN_REJECTED = 0.99


def schema_modulator():
    with open(os.path.join(GOLDEN, 'schema_modulator.json')) as f:
        return [tuple(e) for e in json.load(f)]


def unit_table(name, C):
    """a [64, C] table of unit variance from the name-seeded RNG (nn.Embedding initialises N(0, 1); seeded_tensor scales by 0.02)"""
    return O.seeded_tensor(name, (64, C)) / 0.02


def reseed_tables(st):
    """every `*.modulator.weight` of a seeded state at unit variance, as tests/golden/make_golden_modulator.py sets them -> names"""
    names = [k for k in st if k.endswith('.modulator.weight')]
    for k in names:
        st[k] = O.seeded_tensor(k, tuple(st[k].shape)) / 0.02
    return names


def window_pos(Bn, H, W, s):
    """p(r) of every row r of a [Bn*H*W, C] stream: yy = (r / W) % H, xx = r % W, p = ((yy - s) mod 8) * 8 + ((xx - s) mod 8)"""
    r = torch.arange(Bn * H * W)
    yy, xx = (r // W) % H, r % W
    return ((yy - s) % 8) * 8 + ((xx - s) % 8)


def window_add(y, table, Bn, H, W, s):
    """decoder_Uformer.py:675-691 and back, restated: roll by -s, 8x8 window partition, + table on the 64 tokens of every window,
    window reverse, roll by +s.  y: [Bn*H*W, C], table: [64, C] -> [Bn*H*W, C]"""
    C = y.shape[1]
    t = torch.roll(y.view(Bn, H, W, C), shifts=(-s, -s), dims=(1, 2))
    win = t.view(Bn, H // 8, 8, W // 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64, C)           # window_partition
    win = win + table.unsqueeze(0)
    t = win.view(Bn, H // 8, W // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(Bn, H, W, C)         # window_reverse
    return torch.roll(t, shifts=(s, s), dims=(1, 2)).reshape(Bn * H * W, C)


def wrong_positions(Bn, H, W, s):
    """-> {name: p'(r)}: the positions three wrong kernels would read the table at.  `shift0` exists only where s = 4."""
    p = window_pos(Bn, H, W, s)
    out = {'hw_exchanged': window_pos(Bn, W, H, s), 'transposed': (p % 8) * 8 + p // 8}
    if s:
        out['shift0'] = window_pos(Bn, H, W, 0)
    return out


def fwd_bound(y0, m, dtype):
    """|y - (y0 + m)| <= 2 * 2^-24 (|y0| + |m|): two f32 roundings (what a differently contracted fma can cost), plus for a bf16
    output its rounding 2^-8 |y0 + m|.  y0, m: f64"""
    tol = 2 * U32 * (y0.abs() + m.abs())
    if dtype == torch.bfloat16:
        tol = tol + UBF * (y0 + m).abs()
    return tol
