"""The five 3-channel edge convolutions (fw_inproj_fwd / fw_inproj_bwd / fw_outproj_fwd / fw_outproj_bwd) in their tile form against
torch.nn.functional.conv2d and its autograd in f32 (on the device for the benchmark shapes and the ragged shape, see ref_device).

Error measure and limits are those of test_ops_gpu.py::test_in_out_proj (maximum absolute error over the reference's maximum):
forward results 2e-5, every gradient 1e-4.  Shapes: the two the benchmark runs (decoder B = 16, 128 x 128, C = 56; encoder bands
B = 48, 128 x 128, C = 28 in rows of 32 floats), one whose H and W are not multiples of the 8 x 32 pixel tile with C not a multiple
of 8, and -- fw_inproj_bwd alone takes any C -- one with C not a multiple of 4.  The weight gradients run twice into a pre-filled
buffer: they accumulate, they do not overwrite.

The LeakyReLU derivative is taken from the sign of `out`; the backward calls get the REFERENCE's forward result as `out`, so an
element within rounding of zero cannot pick a different slope on the two sides."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
#            B   H    W    C   row stride
SHAPES = [(16, 128, 128, 56, 56),
          (48, 128, 128, 28, 32),
          (2, 19, 45, 20, 20)]
IDS = ['bench_decoder', 'bench_encoder_ld32', 'ragged_c20']


def call(*a):
    from fwair.lib import call as _c
    return _c(*a)


def rnd(*shape, seed=0, scale=1.0, dev=DEV):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, dtype=torch.float32) * scale).to(dev)


def ref_device(B, H, W, C):
    """where the conv2d reference runs: on the device for the shapes the issue names (bench shapes, the ragged one), on the host --
    as test_in_out_proj does -- for the channel-count corner cases, which are about the entry points' domain, not about the library
    convolution at 1 x 9 x 33 images with 1 000 channels"""
    return DEV if (B, H, W, C) in [s[:4] for s in SHAPES] or C <= 6 else 'cpu'


def close(a, b, tol, what=''):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, f'{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}'
    assert torch.isfinite(a).all(), f'{what}: non-finite values'
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item() / scale
    print(f'{what}: rel-to-max err {err:.3e} (limit {tol:.1e}, scale {scale:.3e})')
    assert err < tol, f'{what}: rel-to-max err {err:.3e} >= {tol:.1e} (scale {scale:.3e})'


def rows(n, C, ld, fill=None):
    """a [n, C] view of a buffer whose rows are ld floats apart (pad columns poisoned: nothing may read or depend on them)"""
    buf = torch.full((n, ld), float('nan') if fill is None else fill, device=DEV)
    return buf[:, :C]


def strided(x, ld):
    v = rows(x.shape[0], x.shape[1], ld)
    v.copy_(x)
    return v


@pytest.mark.parametrize('B,H,W,C,ld', SHAPES, ids=IDS)
def test_inproj(B, H, W, C, ld):
    img = rnd(B, 3, H, W)
    w = (rnd(C, 3, 3, 3, seed=1) * 0.2).requires_grad_(True)
    b = (rnd(C, seed=2) * 0.1).requires_grad_(True)
    ref = F.leaky_relu(F.conv2d(img, w, b, padding=1), 0.01).permute(0, 2, 3, 1).reshape(-1, C)
    out = rows(B * H * W, C, ld)
    call('fw_inproj_fwd', img, w.detach(), b.detach(), out, ld, B, H, W, C, 0.01)
    close(out, ref, 2e-5, 'inproj')
    dy = rnd(B * H * W, C, seed=3)
    ref.backward(dy)
    dys, outs = strided(dy, ld), strided(ref.detach(), ld)
    pre_w, pre_b = rnd(C, 3, 3, 3, seed=8), rnd(C, seed=9)
    dw, db = pre_w.clone(), pre_b.clone()
    for n in (1, 2):                                        # accumulates: pre-fill + n * gradient
        call('fw_inproj_bwd', img, outs, ld, dys, ld, dw, db, B, H, W, C, 0.01)
        close(dw - pre_w, n * w.grad, 1e-4, f'inproj dw x{n}')
        close(db - pre_b, n * b.grad, 1e-4, f'inproj db x{n}')
    if ld > C:
        assert torch.isnan(out.as_strided((B * H * W, ld - C), (ld, 1), C)).all(), 'inproj wrote into the pad columns'


@pytest.mark.parametrize('B,H,W,C', [(2, 19, 45, 6), (1, 9, 33, 1), (1, 9, 33, 301), (1, 9, 33, 1028)], ids=['c6', 'c1', 'c301_sliced', 'c1028_sliced'])
def test_inproj_bwd_any_channel_count(B, H, W, C):
    """fw_inproj_bwd has no C % 4 condition (one channel per lane) and no upper limit on C (channel slices of 256 / 1 024)"""
    R = ref_device(B, H, W, C)
    img = rnd(B, 3, H, W, dev=R)
    w = (rnd(C, 3, 3, 3, seed=1, dev=R) * 0.2).requires_grad_(True)
    b = (rnd(C, seed=2, dev=R) * 0.1).requires_grad_(True)
    ref = F.leaky_relu(F.conv2d(img, w, b, padding=1), 0.01).permute(0, 2, 3, 1).reshape(-1, C)
    dy = rnd(B * H * W, C, seed=3, dev=R)
    ref.backward(dy)
    pre_w, pre_b = rnd(C, 3, 3, 3, seed=8), rnd(C, seed=9)
    dw, db = pre_w.clone(), pre_b.clone()
    for n in (1, 2):
        call('fw_inproj_bwd', img.to(DEV), ref.detach().contiguous().to(DEV), C, dy.to(DEV), C, dw, db, B, H, W, C, 0.01)
        close(dw - pre_w, n * w.grad, 1e-4, f'inproj dw x{n}')
        close(db - pre_b, n * b.grad, 1e-4, f'inproj db x{n}')


@pytest.mark.parametrize('residual', [True, False], ids=['residual', 'plain'])
@pytest.mark.parametrize('B,H,W,C,ld', SHAPES + [(2, 16, 16, 112, 112), (1, 9, 33, 604, 604), (1, 9, 33, 896, 896)], ids=IDS + ['c112', 'c604', 'c896_lds_limit'])
def test_outproj(B, H, W, C, ld, residual):
    R = ref_device(B, H, W, C)
    img = rnd(B, 3, H, W, dev=R)
    fea = rnd(B * H * W, C, seed=4, dev=R).requires_grad_(True)
    w = (rnd(3, C, 3, 3, seed=5, dev=R) * 0.1).requires_grad_(True)
    b = (rnd(3, seed=6, dev=R) * 0.1).requires_grad_(True)
    ref = F.conv2d(fea.view(B, H, W, C).permute(0, 3, 1, 2), w, b, padding=1)
    if residual:
        ref = ref + img
    feas = strided(fea.detach().to(DEV), ld)
    o = torch.empty(B, 3, H, W, device=DEV)
    call('fw_outproj_fwd', feas, ld, w.detach().to(DEV), b.detach().to(DEV), img.to(DEV) if residual else None, o, B, H, W, C)
    close(o, ref, 2e-5, 'outproj')
    if not residual:
        return
    do = rnd(B, 3, H, W, seed=7, dev=R)
    ref.backward(do)
    dfea = rows(B * H * W, C, ld)
    pre_w, pre_b = rnd(3, C, 3, 3, seed=8), rnd(3, seed=9)
    dw, db = pre_w.clone(), pre_b.clone()
    for n in (1, 2):
        call('fw_outproj_bwd', do.to(DEV), feas, ld, w.detach().to(DEV), dfea, ld, dw, db, B, H, W, C)
        close(dfea, fea.grad, 1e-4, 'outproj dfea')
        close(dw - pre_w, n * w.grad, 1e-4, f'outproj dw x{n}')
        close(db - pre_b, n * b.grad, 1e-4, f'outproj db x{n}')
    if ld > C:
        assert torch.isnan(dfea.as_strided((B * H * W, ld - C), (ld, 1), C)).all(), 'outproj_bwd wrote into the pad columns'
