"""What tests/golden/make_spec_bits.py and tests/test_spec_bits_gpu.py share: the cases whose output BYTES are pinned (fixture
spec_bits.json, SHA-256 per case) for the entries built on the shared tile-contraction chunk (DftChunk, csrc/fw_common.h), whose order of
accumulation is a contract -- fw_band_stats, fw_band_split (csrc/fw_spec.hip) and fw_dft2t_fwd / fw_dft2t_bands /
fw_dft2t_decompose (csrc/fw_dft.hip) -- and, group gattn_bands, for the attention-map band filter's entry pair fw_gattn_bands_fwd / bwd
(csrc/fw_gattn.hip) where its bytes do not depend on the tiled passes' order of accumulation (see gattn_bands()).

Every input comes from numpy.random.RandomState's uniform and integer draws (and band_split_cases.random_ring, integer draws of a
seeded torch generator): no libm call of the host takes part, so the inputs are the same bytes wherever the test runs.  That goes
for the panels too: they are seeded uniform values in the padded [3][Np][Np] layout (zero outside n x n), three INDEPENDENT planes,
not cos / sin / -sin -- a digest then also tells a swapped sin / -sin plane from a negated product, which real panels cannot.
The shapes are the smallest at which each path differs: 8 x 8; 9 x 8 (an odd side, the per-element loads and stores); 63 x 65 (Wp = 128
while Wh = 64); 65 x 130 (two tiles each way, 2 v == W present)."""
import hashlib
import os
import subprocess
import zlib

import numpy as np
import torch

import band_split_cases as SC
from fwair import spectrum as S
from fwair.lib import call

DEV = 'cuda'
SHAPES = [(8, 8), (9, 8), (63, 65), (65, 130)]
GROUPS = ['band_stats', 'band_split', 'dft2t', 'gattn_bands']
STATS_NIMG, STATS_NB = 3, 5
SPLIT_NIMG, SPLIT_NBANDS = 2, (1, 2, 3, 4, 5)           # every spec_coli_kernel<NB>; 5 bands: a second group with b0 = 4
DFT_N, DFT_NIMG, DFT_NB = 192, 2, 3
GATTN_B, GATTN_HEADS, GATTN_NB, GATTN_P, GATTN_SEED, GATTN_SITE = 1, 2, 3, 0.1, 777, 41


def toolchain():
    """The version lines of `hipcc --version` (HIP and clang; not where it is installed) of the compiler build.sh uses: the digests
    hold for one compiler.  A hipcc that cannot be run is an error, not another version: the library under test was built with it."""
    r = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--version'], capture_output=True, text=True, timeout=60, check=True)
    return '\n'.join(ln.strip() for ln in r.stdout.splitlines() if 'version' in ln)


def _rs(tag):
    return np.random.RandomState(zlib.crc32(tag.encode()) & 0x7fffffff)


def uniform(tag, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy((lo + (hi - lo) * _rs(tag).random_sample(shape)).astype(np.float32))


def u8(tag, shape):
    return torch.from_numpy(_rs(tag).randint(0, 256, shape).astype(np.uint8))


def rand_panels(n, padded=True):
    """f32 [3][Np][Np]: seeded uniform values in [-1, 1) for i, j < n, zero elsewhere"""
    np_ = S.padded(n) if padded else n
    p = torch.zeros(3, np_, np_)
    p[:, :n, :n] = uniform(f'specbits.panels.{n}', (3, n, n))
    return p.to(DEV)


def sources(h, w, n):
    """-> {source kind: (src, clean)} device tensors: f32 maps, u8 maps, restored f32 beyond [0, 1] with its u8 ground truth"""
    q = u8(f'specbits.u8.{h}x{w}', (n, h, w)).to(DEV)
    return {0: (uniform(f'specbits.f32.{h}x{w}', (n, h, w), 0.0, 1.0).to(DEV), None), 1: (q, None),
            2: (uniform(f'specbits.restored.{h}x{w}', (n, h, w), -0.1, 1.1).to(DEV), q)}


def sha(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)                                                 # numpy has no bf16: the same bytes
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def band_stats():
    out = {}
    for h, w in SHAPES:
        ring = torch.from_numpy(SC.random_ring(h, w, STATS_NB, 11 * h + w)).to(DEV)
        ph, pw = rand_panels(h), rand_panels(w)
        for kind, (src, clean) in sources(h, w, STATS_NIMG).items():
            for power in (0, 1):
                res = torch.zeros((STATS_NIMG, STATS_NB), dtype=torch.float64, device=DEV)
                work = torch.zeros(S.work_floats(STATS_NIMG, h, w, STATS_NB), device=DEV)
                call('fw_band_stats', kind, src, clean, ring, ph, pw, work, res, STATS_NIMG, h, w, STATS_NB, power)
                out[f'{h}x{w}|kind{kind}|power{power}'] = sha(res)
    return out


def band_split():
    out = {}
    for h, w in SHAPES:
        ph, pw = rand_panels(h), rand_panels(w)
        srcs = sources(h, w, SPLIT_NIMG)
        for kind in ((0, 2) if (h, w) == (9, 8) else (0,)):
            src, clean = srcs[kind]
            for nb in SPLIT_NBANDS:
                ring = torch.from_numpy(SC.random_ring(h, w, nb, 13 * h + w + nb)).to(DEV)
                for mode in (0, 1, 2):
                    res = torch.zeros((nb, SPLIT_NIMG, h, w, 2) if mode == 1 else (nb, SPLIT_NIMG, h, w), device=DEV)
                    work = torch.zeros(S.split_work_floats(SPLIT_NIMG, h, w, nb, mode), device=DEV)
                    call('fw_band_split', kind, src, clean, ring, ph, pw, work, res, SPLIT_NIMG, h, w, nb, mode)
                    out[f'{h}x{w}|kind{kind}|bands{nb}|mode{mode}'] = sha(res)
    return out


def dft2t():
    N, n, nb = DFT_N, DFT_NIMG, DFT_NB
    out = {}
    x = uniform('specbits.dft.x', (n, N, N)).to(DEV)
    pn = rand_panels(N, padded=False)
    ring = torch.from_numpy(SC.random_ring(N, N, nb, 192)).to(DEV)
    ring = torch.where(ring >= nb, torch.zeros_like(ring), ring)                # a partition, as fw_dft2t_decompose asks
    mask = torch.stack([ring == b for b in range(nb)]).float().contiguous()
    fr, fi = torch.zeros(n, N, N, device=DEV), torch.zeros(n, N, N, device=DEV)
    call('fw_dft2t_fwd', x, pn, torch.zeros(2 * n * N * N, device=DEV), fr, fi, n, N)
    out['fwd|re'], out['fwd|im'] = sha(fr), sha(fi)
    for mode in (0, 1, 2):
        res = torch.zeros((nb, n, N, N, 2) if mode == 1 else (nb, n, N, N), device=DEV)
        call('fw_dft2t_bands', fr, fi, mask, pn, torch.zeros(2 * nb * n * N * N, device=DEV), res, n, N, nb, mode)
        out[f'bands|mode{mode}'] = sha(res)
    for bits in (0, 1):                                                         # 1: band 0 written as the DC value, no transform
        res = torch.zeros(nb, n, N, N, device=DEV)
        call('fw_dft2t_decompose', x, mask, pn, torch.zeros((2 + 2 * nb) * n * N * N, device=DEV), res, n, N, nb, bits)
        out[f'decompose|dc_bits{bits}'] = sha(res)
    return out


def gattn_bands():
    """out and dqkv of vit.GlobalAttnFn with '<n>_bands' on the N x N map (dlamb is summed with f32 atomics across workgroups: its
    bytes are not reproducible, it stays under the tolerance tests).
      N = 256, lamb != 0: a seeded symmetric band table and seeded uniform [2][256][256] panels -- the 256 kernels, the entry pair,
        the argument filling, the row-dot kernel.
      N = 576 (the smallest tiled N; nine tiles a side), lamb = 0, the tables of _spectral_tables: the filter adds +-0 to a map of
        non-negative probabilities and to G, whose dropped entries are +0, so out and dqkv depend neither on the panels nor on the
        order of accumulation of the tiled passes -- the probabilities, apply, rows, row-dot and dQ / dK / dV kernels and the
        plumbing of the tiled path."""
    from fwair import functional as Fn
    from fwair import vit as V
    B, heads, p, nb = GATTN_B, GATTN_HEADS, GATTN_P, GATTN_NB
    out = {}
    for N in (256, 576):
        if N == 256:
            r = _rs('specbits.gattn.bidx').randint(0, nb, (N, N)).astype(np.uint8)
            bidx = torch.from_numpy(np.triu(r) + np.triu(r, 1).T)
            assert bool((bidx == bidx.t()).all()) and int(bidx.max()) < nb
            spec = (bidx.to(DEV), uniform('specbits.gattn.panels', (2, N, N)).to(DEV))
            lamb0 = uniform('specbits.gattn.lamb', (nb, 1, heads), -0.5, 0.5)
        else:
            spec = V._spectral_tables('bands', nb, torch.device(DEV), n=N)
            lamb0 = torch.zeros(nb, 1, heads)
        for name, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
            qkv = uniform(f'specbits.gattn.qkv.{N}', (B * N, 3 * heads * 64)).to(dtype).to(DEV).requires_grad_(True)
            dout = uniform(f'specbits.gattn.dout.{N}', (B * N, heads * 64), -0.5, 0.5).to(dtype).to(DEV)
            lamb = torch.nn.Parameter(lamb0.to(DEV))
            direct = Fn.config.direct_grads
            Fn.config.direct_grads = False
            Fn.set_dropout_seed(GATTN_SEED, DEV, frozen=True)
            try:
                res = V.GlobalAttnFn.apply(qkv, lamb, (B, N, heads, p, GATTN_SITE, spec))
                res.backward(dout)
                torch.cuda.synchronize()
            finally:
                Fn.set_dropout_seed(1, DEV, frozen=False)
                Fn.config.direct_grads = direct
            assert bool(torch.isfinite(lamb.grad).all())
            out[f'N{N}|{name}|out'], out[f'N{N}|{name}|dqkv'] = sha(res), sha(qkv.grad)
    return out


def digests(group):
    res = {'band_stats': band_stats, 'band_split': band_split, 'dft2t': dft2t, 'gattn_bands': gattn_bands}[group]()
    torch.cuda.synchronize()
    return res
