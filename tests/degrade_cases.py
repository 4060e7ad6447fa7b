"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the degradations that fw_train_batch_synth makes inside the launch (csrc/fw_data.hip;
records and tables: fwair/augment.py) and of its crop / flip / rotation map.  Integers throughout, so the device must agree bit for bit.
The tables RAY / HAZE_T are read from fwair.augment (they are data, built there in float64); the hash is oracle/dropout_hash.py's."""
import numpy as np

import dropout_hash as DH
from fwair import augment as A

RAY, HAZE_T = A.RAY, A.HAZE_T


def site_key(seed, site):
    return int(DH.site_key(seed, site))


def pixel_hash(H, W, key):
    """h[qy][qx] = hash32((qy W + qx) ^ key): one value per pixel, the same for the three channels."""
    idx = np.arange(H * W, dtype=np.uint64)
    return DH._hash32((idx & DH.M32) ^ np.uint64(key)).astype(np.int64).reshape(H, W)


def blur(clean, a, n):
    """n taps (odd) along angle index a, clamped at the image border: (2 sum + n) // (2 n)."""
    assert n % 2 == 1 and 1 <= n <= 25
    _, H, W = clean.shape
    yy, xx = np.mgrid[0:H, 0:W]
    img = clean.astype(np.int64)
    total = np.zeros_like(img)
    for t in range(n):
        s = t - (n - 1) // 2
        dy, dx = (int(np.sign(s)) * int(v) for v in RAY[a][abs(s)])
        total += img[:, np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]
    return ((2 * total + n) // (2 * n)).astype(np.uint8)


def rain_layer(H, W, a, L, density16, key):
    """-> (m, seeds): m[y][x] = max over t < L of A(q) (L - t) at q = (y, x) - RAY[a][t], q inside the image and a seed; 0 without one."""
    h = pixel_hash(H, W, key)
    seeds = (h & 0xFFFF) < density16
    amp = np.where(seeds, 128 + ((h >> 16) & 127), 0)
    m = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(L):
        qy, qx = yy - int(RAY[a][t][0]), xx - int(RAY[a][t][1])
        ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
        v = np.where(ok, amp[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], 0) * (L - t)
        m = np.maximum(m, v)
    return m, seeds


def rain(clean, a, L, density16, s8, key):
    assert 1 <= L <= 32
    m, _ = rain_layer(clean.shape[1], clean.shape[2], a, L, density16, key)
    return np.minimum(255, clean.astype(np.int64) + (m * s8 // (256 * L))[None]).astype(np.uint8)


def haze(clean, j, a8):
    _, H, W = clean.shape
    k = np.arange(H, dtype=np.int64) * 255 // (H - 1) if H > 1 else np.zeros(H, np.int64)
    T = HAZE_T[j].astype(np.int64)[k][None, :, None]
    return ((clean.astype(np.int64) * T + a8 * (65535 - T) + 32767) // 65535).astype(np.uint8)


def degrade_image(clean, rec, seed, site):
    """The full degraded image of one record [8] (code 1..3), as slot `site - batch site` of a batch sees it."""
    code, p1, p2, p3, p4 = (int(v) for v in rec[:5])
    if code == 1:
        return rain(clean, p1, p2, p3, p4, site_key(seed, site))
    if code == 2:
        return haze(clean, p1, p2)
    assert code == 3
    return blur(clean, p1, p2)


def mode_preimage(mode, S):
    """(py, px)[oy][ox]: where output pixel (oy, ox) of a crop turned by `mode` comes from in the unturned crop (k = mode >> 1 quarter
    turns counter-clockwise, then flipud when mode is odd)."""
    oy, ox = np.mgrid[0:S, 0:S]
    k, ii, jj = mode >> 1, (S - 1 - oy if mode & 1 else oy), ox
    if k == 0:
        return ii, jj
    if k == 1:
        return jj, S - 1 - ii
    if k == 2:
        return S - 1 - ii, S - 1 - jj
    return S - 1 - jj, ii


def view(img, ry, rx, rm, S):
    """One view of a [3][H][W] uint8 image from its raw draws -> f32 [3][S][S] (ToTensor)."""
    _, H, W = img.shape
    y0, x0, mode = int(ry) % (H - S + 1), int(rx) % (W - S + 1), 1 + int(rm) % 7
    py, px = mode_preimage(mode, S)
    return img[:, y0 + py, x0 + px].astype(np.float32) / np.float32(255.0)


def noisy_image(clean, sigma, seed, site):
    """Code 0 without a degraded image: the f64 evaluation of the kernel's counter-based draw (oracle/data_oracle.py's rule)."""
    import data_oracle as D
    z = D.hashed_normal(seed, site, clean.size).reshape(clean.shape)
    return np.clip(clean + z * sigma, 0, 255).astype(np.uint8)


def train_batch(images, degraded, sigma, rnd, params, seed, site, S):
    """-> (d1, d2, c1, c2) f32 [B][3][S][S] and the list of full degraded images the slots were cut from."""
    outs, full = [[], [], [], []], []
    for b, clean in enumerate(images):
        if 1 <= int(params[b][0]) <= 3:
            deg = degrade_image(clean, params[b], seed, site + b)
        elif degraded[b] is not None:
            deg = degraded[b]
        elif sigma[b] > 0:
            deg = noisy_image(clean, sigma[b], seed, site + b)
        else:
            deg = clean
        full.append(deg)
        for v in range(2):
            r = rnd[b][3 * v:3 * v + 3]
            outs[v].append(view(deg, *r, S))
            outs[2 + v].append(view(clean, *r, S))
    return tuple(np.stack(o, 0) for o in outs), full


def images(seed, sizes):
    """Smooth colour images with some texture and a wide value range (dark and near-white regions, so rain both adds and saturates)."""
    rs = np.random.RandomState(seed)
    out = []
    for (h, w) in sizes:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        img = np.stack([135 + 125 * np.sin(xx / (5 + c) + yy / (9 + 2 * c)) + rs.randn(h, w) * 10 for c in range(3)])
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out
