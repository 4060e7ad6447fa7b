"""The helper kernels on the step's serial path, at the ownerships their rebuilt forms use (csrc/fw_heads.hip: LFS lambda heads;
csrc/fw_elem.hip: the LDS-tiled fw_permute3, fw_im2col4 / fw_col2im4 by (token, ky) runs).

LFS: against the oracle's per-block lambda head exactly as test_ops_gpu.test_lfs_lambda_heads does, with its tolerances (5e-5 on
coef, 2e-4 on gradients, both relative to the largest reference value), every accumulated buffer pre-filled with non-zero values so
that a kernel that stores instead of adding fails.  The pre-fill holds multiples of 2^-6 below 1/8, so subtracting it again costs at
most one rounding of 2^-27, far below the tolerance.
fw_permute3: bit-exact against the host statement, guards and gap words included, on both sides of the dispatch.
fw_im2col4 / fw_col2im4: bit-exact against a restatement by indexing; zero taps are +0."""
import numpy as np
import pytest
import torch

import airnet_oracle as O
from helpers import SENTINEL, assert_bits, assert_guarded, close, guarded, guarded_like

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32
NAMES = ['mlp_head.%d.0.weight', 'mlp_head.%d.0.bias', 'mlp_head.%d.1.weight', 'mlp_head.%d.1.bias',
         'mlp.%d.0.weight', 'mlp.%d.0.bias', 'mlp.%d.2.weight', 'mlp.%d.2.bias']


def call(*a):
    from fwair.lib import call as _c
    return _c(*a)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=gen(seed + sum(shape)), dtype=F32) * scale


def prefill(*shape, seed):
    """non-zero multiples of 2^-6 in [-1/8, 1/8]"""
    v = torch.randint(1, 9, shape, generator=gen(seed)).float() / 64
    return v * (torch.randint(0, 2, shape, generator=gen(seed + 1)).float() * 2 - 1)


def lam_to_coef(lam, nb):
    if nb == 3:
        l1, l2 = lam[:, 0], lam[:, 1]
        return torch.stack([1 + l2, -l2 / 64, l1 - l2], -1)
    l1 = lam[:, 0]
    return torch.stack([1 + l1, -l1 / 64, torch.zeros_like(l1)], -1)


# ------------------------------------------------------------------------------------------------ LFS lambda heads
LFS_CASES = {'bench_ownership': (16, 3, 64, 448, [1, 2, 4, 8, 16, 16]),      # B, nb, NT, C, heads: the timed step's geometry, 6 blocks
             'tails': (1, 2, 9, 100, [3]),                                     # C no multiple of 64, NT no multiple of the waves
             'model_256': (2, 3, 256, 448, [1, 2, 16])}                        # NT = 256: the 256 x 256 model


@pytest.mark.parametrize('case', list(LFS_CASES))
def test_lfs_heads_accumulate(case):
    B, nb, NT, C, heads_list = LFS_CASES[case]
    nb1, nblk = nb - 1, len(heads_list)
    inter = rnd(nb1 * B, NT, C).requires_grad_(True)
    states = []
    for bi, h in enumerate(heads_list):
        st = {}
        for band in range(1, nb):
            shapes = [(C,), (C,), (h, C), (h,), (h, h), (h,), (h, h), (h,)]
            for n, shp in zip(NAMES, shapes):
                t = rnd(*shp, seed=bi * 100 + band * 10 + len(st)) * (0.3 if len(shp) > 1 else 0.2)
                if n.endswith('0.weight') and len(shp) == 1:
                    t = t + 1
                st[n % band] = t.requires_grad_(True)
        states.append(st)
    lam_ref = [torch.stack([O.lfs_lambda(st, '', i, inter.view(nb1, B, NT, C)[i - 1])[:, 0] for i in range(1, nb)], 1) for st in states]

    xbar, stats = torch.empty(nb1 * B, C, device=DEV), torch.empty(nb1 * B, NT, 2, device=DEV)
    idev = inter.detach().to(DEV)
    call('fw_lfs_xbar', idev, xbar, stats, nb1, B, NT, C, 1e-5)
    ptab, gtab, keep = [], [], []
    for bi, st in enumerate(states):
        for band in (1, 2):
            for j, n in enumerate(NAMES):
                if band < nb:
                    p = st[n % band].detach().to(DEV).contiguous()
                    g0 = prefill(*p.shape, seed=1000 + bi * 32 + band * 8 + j)
                    g = g0.to(DEV)
                    keep.append((st[n % band], g0, g, f'block {bi} band {band} {n % band}', p))     # p: kept alive for ptab
                    ptab.append(p.data_ptr()); gtab.append(g.data_ptr())
                else:
                    ptab.append(0); gtab.append(0)
    ptab = torch.tensor(ptab, dtype=torch.int64, device=DEV)
    gtab = torch.tensor(gtab, dtype=torch.int64, device=DEV)
    heads = torch.tensor(heads_list, dtype=torch.int32, device=DEV)
    offs = np.cumsum([0] + [B * h * 3 for h in heads_list])
    coef_off = torch.tensor(offs[:-1], dtype=torch.int64, device=DEV)
    cbuf, coef = guarded(int(offs[-1]), F32, DEV)
    save = torch.zeros(nblk, 2, B, 16, 3, device=DEV)
    call('fw_lfs_lambda', xbar, ptab, heads, coef_off, coef, save, nblk, B, C, nb1)
    torch.cuda.synchronize()
    assert_guarded(cbuf, coef, 0, 'guards of coef')
    dcoef_host = []
    for bi, h in enumerate(heads_list):
        c = coef[offs[bi]:offs[bi + 1]].view(B, h, 3).cpu()
        close(c, lam_to_coef(lam_ref[bi], nb), 5e-5, f'{case}: coef block {bi}')
        dcoef_host.append(rnd(B, h, 3, seed=50 + bi))
    loss = sum((lam_to_coef(l, nb) * d).sum() for l, d in zip(lam_ref, dcoef_host))
    loss.backward()
    dcoef = torch.cat([d.reshape(-1) for d in dcoef_host]).to(DEV)
    dxbar0 = prefill(nb1 * B, C, seed=7)
    dxbar = dxbar0.to(DEV)
    call('fw_lfs_lambda_bwd', xbar, ptab, gtab, heads, coef_off, dcoef, save, dxbar, nblk, B, C, nb1)
    torch.cuda.synchronize()
    for ref_p, g0, g, what, _ in keep:
        close(g.cpu() - g0, ref_p.grad, 2e-4, f'{case}: what was added to the gradient of {what}')
    # dinter: the kernel adds the LayerNorm backward of the dxbar it is GIVEN; the autograd reference belongs to what lambda_bwd added
    dx_added = (dxbar.cpu() - dxbar0).to(DEV)
    dinter0 = prefill(nb1 * B, NT, C, seed=9)
    dbuf, dinter = guarded_like(dinter0.reshape(-1), DEV)
    call('fw_lfs_xbar_bwd', idev, stats, dx_added, dinter, nb1, B, NT, C)
    torch.cuda.synchronize()
    close(dinter.cpu().view(nb1 * B, NT, C) - dinter0, inter.grad, 2e-4, f'{case}: what was added to dinter')
    assert_guarded(dbuf, dinter, 0, 'guards of dinter')


# ------------------------------------------------------------------------------------------------ fw_permute3
def permuted(src, dims, strides, base):
    """host statement of out[a*s0 + b*s1 + c*s2] = src[a][b][c] into a copy of `base` (1-D)"""
    a, b, c = torch.meshgrid(*(torch.arange(d) for d in dims), indexing='ij')
    idx = (a * strides[0] + b * strides[1] + c * strides[2]).reshape(-1)
    assert idx.unique().numel() == idx.numel() and int(idx.min()) >= 0 and int(idx.max()) < base.numel()
    out = base.clone()
    out[idx] = src.reshape(-1).to(base.dtype)
    return out, idx


# dims, strides, offset of the base pointer in the destination
PERMUTES = {'tile_borders': ((130, 16, 36), (576, 1, 16), 0),               # crosses tile borders in both directions
            'upsample_grad': ((4, 28, 56), (1, 4, 112), 0),                  # the k2s2 transposed-convolution gradient layout
            'no_tile_divides': ((3, 5, 67), (1, 3, 15), 0),
            'gaps': ((5, 7, 3), (50, 6, 2), 0),                              # a destination with gaps: the element-wise kernel
            'negative': ((6, 4, 9), (1, 54, -6), 48)}                        # negative stride, base moved so that indices stay >= 0


def edge_values(n, seed):
    x = torch.randn(n, generator=gen(seed)) * 3
    edge = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, 2.0 ** -100, -3.0e38])
    x[:min(n, edge.numel())] = edge[:n]
    return x


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('pair', [(F32, F32), (F32, BF), (BF, F32)])
@pytest.mark.parametrize('shape', list(PERMUTES))
def test_permute3_forms(shape, pair, accumulate):
    dims, strides, off = PERMUTES[shape]
    tin, tout = pair
    n = dims[0] * dims[1] * dims[2]
    a, b, c = torch.meshgrid(*(torch.arange(d) for d in dims), indexing='ij')
    rel = a * strides[0] + b * strides[1] + c * strides[2]
    assert int(rel.min()) == -off
    span = int(rel.max()) + off + 1
    x = edge_values(n, 70).to(tin)
    base = torch.randn(span, generator=gen(71)).to(tout) if accumulate else torch.full((span,), SENTINEL, dtype=tout)
    _, src = guarded_like(x, DEV)
    dbuf, dst = guarded_like(base, DEV)
    call('fw_permute3', int(tin == BF), int(tout == BF), src, dst[off:], *dims, *strides, accumulate)
    torch.cuda.synchronize()
    idx = (rel + off).reshape(-1)
    assert idx.unique().numel() == n
    want = base.float().clone()
    want[idx] = x.float().reshape(-1) + base.float()[idx] if accumulate else x.float().reshape(-1)   # one f32 sum, then the output's rounding
    if off == 0:
        w2, _ = permuted(x.float(), dims, strides, base.float())
        assert accumulate or bool((w2 == want).all())
    assert_guarded(dbuf, want.to(tout), 0, f'permute3 {shape} {tin}->{tout} accumulate={accumulate}: values, gap words and guards')


# ------------------------------------------------------------------------------------------------ fw_im2col4 / fw_col2im4
CONV_SHAPES = [(2, 8, 24, 28), (1, 16, 8, 56)]                               # B, H, W, C


def col_index(B, H, W):
    """for col row (b, oy, ox) and tap (ky, kx): the input token it reads and whether it lies inside the image"""
    b, oy, ox, ky, kx = torch.meshgrid(torch.arange(B), torch.arange(H // 2), torch.arange(W // 2), torch.arange(4), torch.arange(4),
                                       indexing='ij')
    iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
    inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    tok = (b * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1)
    return tok.reshape(-1), inside.reshape(-1)


@pytest.mark.parametrize('pad', [0, 4])
@pytest.mark.parametrize('dtype', [BF, F32])
@pytest.mark.parametrize('shape', CONV_SHAPES)
def test_im2col4_exact(shape, dtype, pad):
    B, H, W, C = shape
    ldx, ntok = C + pad, B * H * W
    x = edge_values(ntok * C, 31).view(ntok, C)
    xp = torch.full((ntok, ldx), float('nan'))
    xp[:, :C] = x
    tok, inside = col_index(B, H, W)
    want = x[tok].clone()
    want[~inside] = 0.0                                                      # +0
    want = want.to(dtype).reshape(-1)
    cbuf, col = guarded(want.numel(), dtype, DEV)
    call('fw_im2col4', int(dtype == BF), xp.to(DEV), ldx, col, B, H, W, C)
    torch.cuda.synchronize()
    assert_guarded(cbuf, want, 0, f'im2col4 {shape} {dtype} ldx={ldx}')
    z = col.cpu().view(-1, C)[~inside]
    assert z.numel() > 0 and bool((z.view(torch.int16 if dtype == BF else torch.int32) == 0).all()), 'border taps are exactly +0'


@pytest.mark.parametrize('with_dres', [False, True])
@pytest.mark.parametrize('pad', [0, 4])
@pytest.mark.parametrize('dtype', [BF, F32])
@pytest.mark.parametrize('shape', CONV_SHAPES)
def test_col2im4_exact(shape, dtype, pad, with_dres):
    B, H, W, C = shape
    ldd, ntok = C + pad, B * H * W
    nrow = B * (H // 2) * (W // 2)
    dcol = (torch.randn(nrow * 16, C, generator=gen(41)) * 2).to(dtype)
    dres = torch.randn(ntok, C, generator=gen(42))
    dres[0, :4] = -0.0                                                      # token 0 has ONE tap, (ky, kx) = (1, 1) of col row 0: with -0 there
    dcol[5, :4] = -0.0                                                      # too the sum stays -0 only if the absent taps are skipped, not added as +0
    tok, inside = col_index(B, H, W)
    # dx[token] = dres, then its taps in (ky, kx) ascending order, each one f32 addition
    want = dres.clone() if with_dres else torch.zeros(ntok, C)
    vals = dcol.float()
    taps = torch.arange(16).repeat(nrow)
    for t in range(16):                                                      # ky * 4 + kx ascending; a token meets each tap at most once
        sel = inside & (taps == t)
        want[tok[sel]] = want[tok[sel]] + vals[sel]
    full = torch.full((ntok, ldd), SENTINEL)
    full[:, :C] = want
    dbuf, dx = guarded(ntok * ldd, F32, DEV)
    rp = torch.full((ntok, ldd), float('nan'))
    rp[:, :C] = dres
    call('fw_col2im4', int(dtype == BF), dcol.to(DEV), dx, ldd, rp.to(DEV) if with_dres else None, ldd if with_dres else 0, B, H, W, C)
    torch.cuda.synchronize()
    assert_guarded(dbuf, full.reshape(-1), 0, f'col2im4 {shape} {dtype} lddx={ldd} dres={with_dres}')
