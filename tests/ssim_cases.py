"""Cases, seeded inputs and a torch-CPU restatement of the Gaussian-window SSIM (fw_ssim11_loss; the reference's
utils/pytorch_ssim/__init__.py:19-43), shared by tests/golden/make_ssim_golden.py and the CPU and GPU tests of the SSIM loss.

The restatement is differentiable (plain torch ops on conv2d).  `maps` / `closed_form_grad` evaluate the gradient the kernel implements
from the five filtered maps, without autograd."""
import math

import numpy as np
import torch
import torch.nn.functional as F

TILE = 32                      # fw_loss.hip SS_T: a workgroup's tile; seams lie at multiples of it
C1, C2 = 0.01 ** 2, 0.03 ** 2

# name, (n, C, H, W), seed, kind
CASES = [
    ('window_over_image', (1, 3, 8, 8), 11, 'noise'),           # every tap of every pixel meets the padding
    ('one_dim_under_window', (1, 1, 9, 70), 12, 'noise'),       # H under the window, a ragged width over three tiles
    ('planes_nonsquare', (2, 3, 24, 40), 13, 'noise'),          # plane and image indexing, under one tile in H
    ('odd_unaligned', (2, 3, 33, 17), 14, 'noise'),             # odd sizes, unaligned rows: the element-wise store
    ('seams_partial_tile', (1, 3, 72, 40), 15, 'noise'),        # tile seams, a partial last tile
    ('seams_both_odd', (1, 1, 65, 67), 16, 'noise'),            # seams in both directions, last tiles 1 and 3 pixels wide, W % 4 != 0
    ('training_shape', (1, 3, 128, 128), 17, 'noise'),
    ('smooth_ramp', (1, 3, 48, 48), 18, 'smooth'),              # E[x^2] - mu^2 cancels, C2 decides
]


def inputs(shape, seed, kind):
    """-> (a, b) f32: b the clean image, a the restoration.  'noise': b uniform in [0, 1], a = b + 0.1 * normal.  'smooth': a ramp of
    contrast 0.05 around 0.5 (over x and y, shifted per plane), a = b + 0.01 * normal."""
    rs = np.random.RandomState(seed)
    n, C, H, W = shape
    if kind == 'noise':
        b = rs.uniform(size=shape)
        a = b + 0.1 * rs.standard_normal(shape)
    else:
        y = np.arange(H, dtype=np.float64)[:, None] / H
        x = np.arange(W, dtype=np.float64)[None, :] / W
        p = np.arange(n * C, dtype=np.float64).reshape(n, C, 1, 1)
        b = 0.5 + 0.05 * (0.6 * x + 0.4 * y - 0.5) + 0.01 * p
        a = b + 0.01 * rs.standard_normal(shape)
    return torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b.astype(np.float32))


def taps():
    """The normalised 11-tap Gaussian, sigma 1.5, as f32 (each exponential rounded to f32, divided by their f32 sum)."""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return g / g.sum()


def window(dtype):
    """The 11 x 11 window: outer product of the f32 taps formed in f32, then cast."""
    g = taps()
    return torch.outer(g, g).to(dtype)


def _conv(x, w):
    C = x.shape[1]
    return F.conv2d(x, w.expand(C, 1, 11, 11), padding=5, groups=C)


def maps(a, b):
    """-> mu_a, mu_b, E_aa, E_bb, E_ab, zero padding 5"""
    w = window(a.dtype)
    return _conv(a, w), _conv(b, w), _conv(a * a, w), _conv(b * b, w), _conv(a * b, w)


def ssim_map(a, b):
    ma, mb, eaa, ebb, eab = maps(a, b)
    saa, sbb, sab = eaa - ma * ma, ebb - mb * mb, eab - ma * mb
    return ((2 * ma * mb + C1) * (2 * sab + C2)) / ((ma * ma + mb * mb + C1) * (saa + sbb + C2))


def ssim(a, b):
    """mean SSIM of two [n, C, H, W] tensors, differentiable."""
    return ssim_map(a, b).mean()


def closed_form_grad(a, b):
    """d mean(S) / d a from the five maps: (conv(G_mu) + 2 a conv(G_aa) + b conv(G_ab)) / N (the window is its own adjoint)."""
    ma, mb, eaa, ebb, eab = maps(a, b)
    saa, sbb, sab = eaa - ma * ma, ebb - mb * mb, eab - ma * mb
    A1, A2 = 2 * ma * mb + C1, 2 * sab + C2
    B1, B2 = ma * ma + mb * mb + C1, saa + sbb + C2
    S = A1 * A2 / (B1 * B2)
    Gaa = -S / B2
    Gab = 2 * A1 / (B1 * B2)
    Gmu = 2 * mb * (A2 - A1) / (B1 * B2) - 2 * ma * S / B1 + 2 * ma * S / B2
    w = window(a.dtype)
    return (_conv(Gmu, w) + 2 * a * _conv(Gaa, w) + b * _conv(Gab, w)) / a.numel()


def workgroups(shape):
    n, C, H, W = shape
    return n * C * (-(-H // TILE)) * (-(-W // TILE))
