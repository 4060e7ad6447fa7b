"""What tests/test_restore_tiles_cpu.py and tests/test_restore_tiles_gpu.py share: the numpy restatement of fw_restore_gather /
fw_restore_blend (include/fwair.h) -- tile origins, the reflection rule R, the eight mode maps, the ramp weights, the blend evaluated
in f64 from the f32 weights -- and the bound of the kernel's deviation from it."""
import numpy as np

T = 16                                        # the tile of the stub-network tests
OVERLAPS = [0, 5, 8]                          # none, one that is no multiple of 4 (one pixel per thread), the largest (T / 2)
SIZES = [(5, 7), (1, 16), (16, 16), (17, 40), (50, 23), (16, 33)]      # smaller than the tile, a single row, exact, odd, H > W
# every width, and so every offset in the packed buffer, a multiple of 4: at overlaps 0 and 8 fw_restore_blend takes four x per thread
ALIGNED = [(16, 16), (17, 40), (1, 16), (20, 24), (7, 8)]
U32 = 2.0 ** -24


def origins(size, tile, overlap):
    """range(0, P - T, T - overlap) + [P - T], P = max(size, T)"""
    P = max(size, tile)
    return list(range(0, P - tile, tile - overlap)) + [P - tile]


def reflect(y, n):
    """R(y, n) for an integer array y: whole-sample reflection without edge repeat, continued periodically; 0 at n = 1"""
    y = np.asarray(y, dtype=np.int64)
    if n == 1:
        return np.zeros_like(y)
    p = 2 * n - 2
    m = ((y % p) + p) % p
    return np.where(m < n, m, p - m)


def preimage(mode, tile):
    """-> (PY, PX) int arrays [T, T]: tile element (oy, ox) comes from (PY[oy, ox], PX[oy, ox]) of the unturned tile"""
    oy, ox = np.mgrid[0:tile, 0:tile]
    k = mode >> 1
    ii = tile - 1 - oy if mode & 1 else oy
    jj = ox
    return [(ii, jj), (jj, tile - 1 - ii), (tile - 1 - ii, tile - 1 - jj), (tile - 1 - jj, ii)][k]


def image(mode, tile):
    """-> (OY, OX) int arrays [T, T]: the turned tile holds unturned (py, px) at (OY[py, px], OX[py, px]); the stated inverse"""
    py, px = np.mgrid[0:tile, 0:tile]
    k = mode >> 1
    ii, jj = [(py, px), (tile - 1 - px, py), (tile - 1 - py, tile - 1 - px), (px, tile - 1 - py)][k]
    return (tile - 1 - ii if mode & 1 else ii), jj


def turn(x, mode):
    """utils/image_utils.py:133-175 on the last two axes: rot90 by mode // 2, then flipud when mode is odd"""
    out = np.rot90(x, mode >> 1, axes=(-2, -1))
    return np.flip(out, -2) if mode & 1 else out


def weights(tile, ramp):
    """w1(i) = (float)min(i + 1, T - i, ramp) / (float)ramp as f32"""
    i = np.arange(tile)
    return (np.minimum(np.minimum(i + 1, tile - i), ramp).astype(np.float32) / np.float32(ramp)).astype(np.float32)


def plan(sizes, tile, overlap, nmodes):
    """-> rows [(image, y0, x0, mode)], image after image, positions rows major, the modes of a position next to each other"""
    return [(i, y, x, m) for i, (H, W) in enumerate(sizes) for y in origins(H, tile, overlap) for x in origins(W, tile, overlap)
            for m in range(nmodes)]


def candidates(y, n, stride, tile):
    """the tiles of an axis the blend looks at for coordinate y: regular a with a stride <= y < a stride + T and a <= n - 2, then n - 1"""
    return [a for a in range(n - 1) if a * stride <= y < a * stride + tile] + [n - 1]


def gather(src, y0, x0, mode, tile):
    """src [3, H, W] (any dtype) -> [3, T, T]: src[c][R(y0 + py)][R(x0 + px)] at the preimage (py, px) of every (oy, ox)"""
    PY, PX = preimage(mode, tile)
    return src[:, reflect(y0 + PY, src.shape[1]), reflect(x0 + PX, src.shape[2])]


def unit(u8):
    """uint8 -> f32 in [0, 1] as ToTensor divides: correctly rounded"""
    return (u8.astype(np.float32) / np.float32(255.0)).astype(np.float32)


def blend(rest, rows, H, W, tile, ramp):
    """rest [n, 3, T, T] (f32 values), rows: the n tiles of ONE image -> (out f64 [3, H, W], K int [H, W], vmax f64 [3, H, W]):
    sum(w v) / sum(w) in f64 with the f32 weights, the number of terms, and the largest |v| among them"""
    w1 = weights(tile, ramp)
    w = (w1[:, None] * w1[None, :]).astype(np.float32).astype(np.float64)            # the product rounded once in f32
    num, den = np.zeros((3, H, W)), np.zeros((H, W))
    K, vmax = np.zeros((H, W), dtype=np.int64), np.zeros((3, H, W))
    for t, (_, y0, x0, mode) in enumerate(rows):
        OY, OX = image(mode, tile)
        u = rest[t].astype(np.float64)[:, OY, OX]                                     # the turn undone: u[c][py][px]
        ya, yb, xa, xb = max(y0, 0), min(y0 + tile, H), max(x0, 0), min(x0 + tile, W)
        if ya >= yb or xa >= xb:
            continue
        uu, ww = u[:, ya - y0:yb - y0, xa - x0:xb - x0], w[ya - y0:yb - y0, xa - x0:xb - x0]
        num[:, ya:yb, xa:xb] += ww * uu
        den[ya:yb, xa:xb] += ww
        K[ya:yb, xa:xb] += 1
        vmax[:, ya:yb, xa:xb] = np.maximum(vmax[:, ya:yb, xa:xb], np.abs(uu))
    return num / den, K, vmax


def blend_bound(K, vmax):
    """|kernel - blend| <= (2 K + 4) 2^-24 max|v|: one rounding per product w v, K - 1 in the sum of the products and K - 1 in the sum
    of the weights, one for the division -- 2 K relative to sum(w |v|) / sum(w) <= max|v| -- and 4 for the second-order terms, the
    rounding of the reference's own f64 arithmetic and the comparison"""
    return (2 * K[None] + 4) * U32 * vmax


def restore(src_f32, rows, H, W, tile, ramp, net):
    """the whole path for one image: gather every tile from src_f32 [3, H, W], net(tile [3, T, T]) -> f32 tile, blend"""
    rest = np.stack([net(gather(src_f32, y0, x0, m, tile)) for _, y0, x0, m in rows]).astype(np.float32)
    return blend(rest, rows, H, W, tile, ramp)


def images(seed, sizes):
    """the generator of tests/test_folder_eval_gpu.py:_images"""
    rs = np.random.RandomState(seed)
    out = []
    for (h, w) in sizes:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        img = np.stack([127 + 90 * np.sin(xx / (7 + c) + yy / (11 + 2 * c)) + rs.randn(h, w) * 12 for c in range(3)])
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def noisy(imgs, seed, sigma=25):
    rs = np.random.RandomState(seed)
    return [np.clip(i + rs.randn(*i.shape) * sigma, 0, 255).astype(np.uint8) for i in imgs]
