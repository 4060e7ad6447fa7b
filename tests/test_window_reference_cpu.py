"""The window-attention reference of the GPU tests (test_ops_gpu.ref_window_attention) is pinned to the reference model's goldens at
square sizes only.  Here it is compared, at H != W, with a second statement of the same operation that shares none of its pieces:
explicit loops over images, windows, heads and tokens, the cyclic roll as index arithmetic, the relative-position bias looked up
coordinate by coordinate, and the shift mask from the nine-region label image (regions [0, H-8), [H-8, H-shift), [H-shift, H) per axis;
-100 between tokens of different regions), as decoder_Uformer.py:634-651 builds it.  float64, no frequency selection; limit 1e-12."""
import pytest
import torch

from test_ops_gpu import ref_window_attention, rnd

WIN = 8


def region(p, size, shift):
    return 0 if p < size - WIN else (1 if p < size - shift else 2)


def naive_window_attention(qkv, C, B, H, W, heads, L, mode, shift, tables):
    """qkv: [L*B*H*W, 3C] (q | k | v), image index = band * B + b.  tables: [L*L, 225, heads].  -> [L*B*H*W, C]"""
    D = C // heads
    x = qkv.view(L, B, H, W, 3, heads, D)
    out = torch.zeros(L, B, H, W, heads, D, dtype=qkv.dtype)
    # pixel of token t of window (wy, wx) in the UNROLLED image: rolling by -shift moves pixel p + shift to position p
    def pix(wy, wx, t):
        return (wy * WIN + t // WIN + shift) % H, (wx * WIN + t % WIN + shift) % W
    # label of a position of the ROLLED image
    def label(wy, wx, t):
        return 3 * region(wy * WIN + t // WIN, H, shift) + region(wx * WIN + t % WIN, W, shift)
    bias = torch.zeros(L * L, heads, 64, 64, dtype=qkv.dtype)
    for i in range(64):
        for j in range(64):
            bias[:, :, i, j] = tables[:, (i // WIN - j // WIN + WIN - 1) * (2 * WIN - 1) + (i % WIN - j % WIN + WIN - 1), :]
    for wy in range(H // WIN):
        for wx in range(W // WIN):
            ys = torch.tensor([pix(wy, wx, t)[0] for t in range(64)])
            xs = torch.tensor([pix(wy, wx, t)[1] for t in range(64)])
            mask = torch.zeros(64, 64, dtype=qkv.dtype)
            if shift:
                lab = [label(wy, wx, t) for t in range(64)]
                for i in range(64):
                    for j in range(64):
                        if lab[i] != lab[j]:
                            mask[i, j] = -100.0
            for b in range(B):
                for lq in range(L):
                    keys = [lq] if mode == 0 else [lk for lk in range(L) if lk != lq]
                    for h in range(heads):
                        qw = x[lq, b, ys, xs, 0, h] * D ** -0.5                        # [64, D]
                        s = torch.cat([qw @ x[lk, b, ys, xs, 1, h].t() + bias[lq * L + lk, h] + mask for lk in keys], 1)
                        p = torch.exp(s - s.max(1, keepdim=True).values)
                        p = p / p.sum(1, keepdim=True)
                        out[lq, b, ys, xs, h] = p @ torch.cat([x[lk, b, ys, xs, 2, h] for lk in keys], 0)
    return out.reshape(L * B * H * W, C)


@pytest.mark.parametrize('L,mode', [(1, 0), (3, 1)])
@pytest.mark.parametrize('H,W', [(16, 24), (24, 16)])
def test_window_reference_at_rectangles(H, W, L, mode):
    B, heads, shift = 2, 2, 4
    C = 28 * heads
    qkv = rnd(L * B * H * W, 3 * C).double()
    tables = (rnd(L * L, 225, heads, seed=1) * 0.5).double()
    ref = ref_window_attention(qkv, C, B, H, W, heads, L, mode, shift, tables)
    naive = naive_window_attention(qkv, C, B, H, W, heads, L, mode, shift, tables)
    err = (ref - naive).abs().max().item()
    print(f'{H}x{W} L={L} mode={mode}: max abs difference {err:.3e}')
    assert err < 1e-12
