"""What tests/golden/make_golden_band_stats.py, tests/test_band_stats_cpu.py and tests/test_band_stats_gpu.py share: the cases of the
fixture unit_band_stats.npz, their seeded inputs (not stored), the f64 reference of fw_band_stats and the f32 emulation of its chain."""
import numpy as np
import torch

from helpers import rnd

# (h, w, size) of get_frequency_distribution: the smallest maps, odd sides, h != w both ways, sides beside a multiple of 64 (63 / 65),
# more than one 64-tile per axis (65 x 130, 100 x 100), 2 to 10 rings
CASES = [(8, 8, 0.2), (9, 8, 1 / 3), (16, 16, 0.5), (24, 40, 0.2), (40, 24, 0.2), (33, 47, 0.25), (50, 36, 0.1), (63, 65, 0.2),
         (65, 130, 0.2), (100, 100, 0.2)]
NIMG = 3


def key(h, w, size, norm):
    return f'{h}x{w}|{size:.6f}|{"norm" if norm else "raw"}'


def images(h, w, n=NIMG, tag='bandstats'):
    """f64 numpy [n][h][w]: whole grey levels 0..255 around 128 (so a u8 copy holds the same values and no ring's sum is near zero)"""
    x = 128.0 + rnd(f'{tag}.{h}x{w}', (n, h, w), 40.0).double()
    return x.round().clamp(0, 255).numpy()


def band_sums(x, ring_shifted, nbands, power):
    """f64 reference of fw_band_stats: x numpy [n][h][w], ring in fftshift-ed coordinates -> [n][nbands]"""
    mag = np.abs(np.fft.fftshift(np.fft.fft2(x.astype(np.float64)), axes=(-2, -1)))
    if power:
        mag = mag * mag
    return np.stack([(mag * (ring_shifted == b)).sum((-2, -1)) for b in range(nbands)], -1)


def _mm_f32(a, b):
    """a [.., m, K] @ b [K, n] in f32 with the kernel's order of accumulation: the accumulator takes the K terms four at a time, in
    order (one v_mfma_f32_16x16x4_f32 per step), so its error is that of a K / 4-step sequential sum whatever the host's BLAS does
    with a long dot product"""
    acc = torch.zeros(a.shape[:-1] + (b.shape[1],), dtype=torch.float32)
    for k in range(0, a.shape[-1], 4):
        acc = acc + a[..., k:k + 4] @ b[k:k + 4]
    return acc


def emulate_f32(x, ring_shifted, nbands, power):
    """The kernel's chain on the host: f32 panels, f32 products accumulated in the kernel's order (row pass, then column pass, real
    and imaginary parts as separate real products; the column pass adds the real and the imaginary input's term alternately), f32
    magnitudes, one f32 partial sum per 64 x 64 tile of the spectrum (u from 64 i, v from 64 j) and band, the fold of the partials in
    double.  x numpy [n][h][w] -> [n][nbands] f64"""
    from fwair import spectrum as S
    n, h, w = x.shape
    ph, pw = torch.from_numpy(S.panels_host(h))[:, :h, :h], torch.from_numpy(S.panels_host(w))[:, :w, :w]
    xf = torch.from_numpy(x.astype(np.float32))
    tr, ti = _mm_f32(xf, pw[0]).transpose(1, 2), _mm_f32(xf, pw[2]).transpose(1, 2)          # T^t[v][y]
    fr = torch.zeros(n, w, h, dtype=torch.float32)                                           # F^t[v][u] = sum_y T^t[v][y] W_H[y][u]
    fi = torch.zeros(n, w, h, dtype=torch.float32)
    for k in range(0, h, 4):
        fr = (fr + tr[..., k:k + 4] @ ph[0, k:k + 4]) + ti[..., k:k + 4] @ ph[1, k:k + 4]
        fi = (fi + tr[..., k:k + 4] @ ph[2, k:k + 4]) + ti[..., k:k + 4] @ ph[0, k:k + 4]
    e = (fr * fr + fi * fi).transpose(1, 2)
    mag = e if power else torch.sqrt(e)
    ring = torch.from_numpy(np.ascontiguousarray(np.fft.ifftshift(ring_shifted)))
    hp, wp = (h + 63) // 64 * 64, (w + 63) // 64 * 64
    out = []
    for b in range(nbands):
        m = torch.zeros(n, hp, wp, dtype=torch.float32)
        m[:, :h, :w] = mag * (ring == b)
        part = m.view(n, hp // 64, 64, wp // 64, 64).sum((2, 4))                              # f32, one per tile
        out.append(part.double().sum((1, 2)).numpy())
    return np.stack(out, -1)


def rel_err(got, ref):
    """largest per-band relative error (bands whose reference is exactly 0 must be exactly 0)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    zero = ref == 0
    assert (got[zero] == 0).all(), 'an empty band is not exactly 0'
    return float((np.abs(got - ref)[~zero] / np.abs(ref[~zero])).max()) if (~zero).any() else 0.0
