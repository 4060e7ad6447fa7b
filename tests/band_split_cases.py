"""What tests/golden/make_golden_band_split.py, tests/test_band_split_cpu.py and tests/test_band_split_gpu.py share: the cases of the
fixture unit_band_split.npz, the shapes of the GPU test, their seeded inputs (not stored), the f64 reference of fw_band_split and the f32
emulation of its four-pass chain."""
import numpy as np
import torch

from helpers import rnd

# the fixture: reference FrequencyDecompose on rnd(...) of shape (1, 2, h, w); the two largest sizes are stored at every STRIDE-th pixel
GOLDEN_SIZES = [(9, 8), (24, 40), (33, 47), (63, 65), (65, 130), (96, 96)]
GOLDEN_KINDS = [('frequency_decompose', 1 / 3.), ('frequency_decompose_1', 0.5), ('frequency_decompose', 1.0)]
GOLDEN_INVERSE = [True, False, 'visual']
STRIDE = {(65, 130): 3, (96, 96): 3}

# the GPU test's shapes: the smallest, one odd side each way, h != w both ways, both sides odd with W % 4 != 0, either side of a
# 64-tile, W / 2 + 1 = 66 in a second half-spectrum tile, two tiles per axis, an extreme pitch / grid, the debug sides, a BSD68 image
SHAPES = [(8, 8), (9, 8), (8, 9), (24, 40), (40, 24), (33, 47), (63, 65), (65, 130), (100, 100), (8, 1024), (1024, 8), (96, 96), (48, 48),
          (24, 24), (321, 481)]
LARGEST = (1024, 1024)                       # nimg 1, mode 0, one ring kind
RING_KINDS = [('bands', 1 / 3.), ('bands_1', 0.5)]          # three bands each
NIMG = 3
TOL = 2e-5                                   # relative to the reference's maximum: the project's limit for the band decomposition


def key(h, w, kind, size, inverse):
    return f'{h}x{w}|{kind}|{size:.4f}|{inverse}'


def golden_input(h, w):
    return rnd(f'bandsplit.{h}x{w}', (1, 2, h, w))


def maps(h, w, n=NIMG, tag='bandsplit'):
    """f64 numpy [n][h][w] of f32 values: unit normal plus a mean of 0.5 (DC stands out as it does in an image)"""
    return (0.5 + rnd(f'{tag}.maps.{h}x{w}', (n, h, w))).float().double().numpy()


def ring_unshifted(kind, size, h, w):
    from fwair import spectrum as S
    return np.ascontiguousarray(np.fft.ifftshift(S.ring_index(kind, size, h, w)))


def random_ring(h, w, nbands, seed):
    """a table without any symmetry: band indices 0 .. nbands - 1, and 255 / 40 for `in no band` (un-shifted coordinates)"""
    g = torch.Generator().manual_seed(seed)
    ring = torch.randint(0, nbands + 2, (h, w), generator=g).to(torch.uint8)
    ring[ring == nbands] = 255
    ring[ring == nbands + 1] = 40
    return ring.numpy()


def reference(x, ring, nbands, mode):
    """f64 reference of fw_band_split: x numpy [n][h][w], ring u8 [h][w] un-shifted -> [nbands][n][h][w] (mode 1: [..., 2])"""
    F = np.fft.fft2(x.astype(np.float64))
    out = []
    for b in range(nbands):
        Fb = F * (ring == b)
        if mode == 0:
            out.append(np.fft.ifft2(Fb).real)
        elif mode == 1:
            out.append(np.stack([Fb.real, Fb.imag], -1))
        else:
            out.append(np.abs(np.fft.fftshift(Fb, axes=(-2, -1))))
    return np.stack(out)


def weights(ring, nbands):
    """f32 [nbands][h][w / 2 + 1]: what the inverse column pass multiplies the half spectrum with -- c_v / 2 ([ring[u][v] == b] +
    [ring[(h - u) % h][(w - v) % w] == b]), c_v = 1 for v = 0 and 2 v = w, 2 otherwise: 0, 1/2, 1 or 2"""
    h, w = ring.shape
    wh = w // 2 + 1
    mirror = np.roll(ring[::-1, ::-1], (1, 1), (0, 1))                   # mirror[u][v] = ring[(h - u) % h][(w - v) % w]
    v = np.arange(wh)
    cv = np.where((v == 0) | (2 * v == w), 0.5, 1.0).astype(np.float32)
    return np.stack([cv * ((ring[:, :wh] == b).astype(np.float32) + (mirror[:, :wh] == b).astype(np.float32)) for b in range(nbands)])


def _mm2_f32(a, pa, b, pb):
    """(a [.., m, K] @ pa [K, n]) + (b @ pb) in f32 with the kernel's order: the accumulator takes four k of the first product, then
    the same four k of the second, in order (band_stats_cases._mm_f32 for two interleaved products)"""
    acc = torch.zeros(a.shape[:-1] + (pa.shape[1],), dtype=torch.float32)
    for k in range(0, a.shape[-1], 4):
        acc = (acc + a[..., k:k + 4] @ pa[k:k + 4]) + b[..., k:k + 4] @ pb[k:k + 4]
    return acc


def emulate_f32(x, ring, nbands):
    """Mode 0 of the kernel's chain on the host: f32 panels, f32 products accumulated four k at a time in order -- row pass (columns
    v <= w / 2 only), forward column pass, per band the weighted inverse column pass (weights(): the half-spectrum doubling and the
    1/2 of the symmetrised ring; the products are exact) and the inverse row pass, scaled by the f32 value of 1 / (h w).
    x numpy [n][h][w], ring u8 [h][w] un-shifted -> f32 numpy [nbands][n][h][w]"""
    from band_stats_cases import _mm_f32
    from fwair import spectrum as S
    n, h, w = x.shape
    wh = w // 2 + 1
    ph, pw = torch.from_numpy(S.panels_host(h))[:, :h, :h], torch.from_numpy(S.panels_host(w))[:, :w, :w]
    xf = torch.from_numpy(x.astype(np.float32))
    tr, ti = _mm_f32(xf, pw[0][:, :wh]).transpose(1, 2), _mm_f32(xf, pw[2][:, :wh]).transpose(1, 2)          # T^t[v][y]
    fr, fi = _mm2_f32(tr, ph[0], ti, ph[1]), _mm2_f32(tr, ph[2], ti, ph[0])                                  # F^t[v][u]
    wt = torch.from_numpy(weights(ring, nbands)).transpose(1, 2)                                             # [nb][v][u]
    scale = np.float32(1.0) / (np.float32(h) * np.float32(w))
    out = []
    for b in range(nbands):
        br, bi = wt[b] * fr, wt[b] * fi
        gr, gi = _mm2_f32(br, ph[0], bi, ph[2]).transpose(1, 2), _mm2_f32(br, ph[1], bi, ph[0]).transpose(1, 2)      # G[y][v]
        out.append((_mm2_f32(gr, pw[0][:wh], gi, pw[2][:wh]) * scale).numpy())
    return np.stack(out)


def rel_max_err(got, ref):
    """helpers.close's figure: the largest deviation relative to the reference's largest magnitude"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-12))
