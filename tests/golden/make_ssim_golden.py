"""Fixture generator of the SSIM loss -- runs ONLY where the reference exists (oracle/refshim.py: REFERENCE_ROOT).

Imports the reference's utils/pytorch_ssim and, for every case of tests/ssim_cases.py, runs `ssim(a, b)` with autograd on the seeded
f32-valued inputs -- once in f64 (the expected value and gradient) and once in f32 (how far the reference's own f32 run is from that:
the scale of the kernel test's tolerance).  Stores tests/golden/unit_ssim11.npz: per case the seed, the shape, the f64 value and
gradient and the two deviations.  Inputs are regenerated from the seed, never stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ssim_golden.py

A fixture is data (expected outputs); no reference source text is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import refshim                     # noqa: E402
import ssim_cases as SC            # noqa: E402

sys.path.insert(0, refshim.REFERENCE_ROOT)
from utils import pytorch_ssim     # noqa: E402

torch.set_num_threads(8)


def run(a, b, dtype):
    a = a.to(dtype).requires_grad_(True)
    v = pytorch_ssim.ssim(a, b.to(dtype))
    g, = torch.autograd.grad(v, a)
    return v.detach(), g


def main():
    out = {}
    for name, shape, seed, kind in SC.CASES:
        a, b = SC.inputs(shape, seed, kind)
        v64, g64 = run(a, b, torch.float64)
        v32, g32 = run(a, b, torch.float32)
        out[name + '.seed'] = np.asarray(seed)
        out[name + '.shape'] = np.asarray(shape)
        out[name + '.value'] = v64.numpy()
        out[name + '.grad'] = g64.numpy()
        out[name + '.f32_value_dev'] = np.asarray(abs(float(v32.double() - v64)))
        out[name + '.f32_grad_dev'] = np.asarray(float((g32.double() - g64).abs().max()))
        print(f'{name:22s} {str(shape):18s} SSIM {float(v64):.12f}  max|grad| {float(g64.abs().max()):.3e}  reference f32 run: '
              f'value off by {float(out[name + ".f32_value_dev"]):.2e}, gradient by {float(out[name + ".f32_grad_dev"]):.2e}')
    path = os.path.join(HERE, 'unit_ssim11.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
