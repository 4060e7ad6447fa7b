"""fw_restore_gather / fw_restore_blend (csrc/fw_data.hip) and EvalEngine's overlap / ensemble / pad_small path against the numpy
restatement of tests/restore_cases.py: tiles that leave the image (reflection), overlap weighted by a ramp, the eight flips and
rotations turned back before they are averaged.  Tile 16 and stub networks, except for the one run of the seeded model."""
import numpy as np
import pytest
import torch

import airnet_oracle as O
import data_oracle as D
import restore_cases as RC
from helpers import close, make_opt, schema

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = RC.T
SITE = 0x7B000000
CASES = [(ov, nm) for ov in RC.OVERLAPS for nm in (1, 8)]
SIZE_LISTS = [RC.SIZES, RC.ALIGNED]


def _dev(imgs):
    return [torch.from_numpy(i).to(DEV) for i in imgs]


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(clean, degraded, sizes, overlap, nmodes, sigma=0.0):
    """one chunk: -> device itab, ttab, gtab (8 columns), gtab4, sigma and the host rows"""
    from fwair.evaluate import plan_tiles_ex
    ttab, gtab, chunks = plan_tiles_ex(sizes, T, 65535, overlap, nmodes, True)
    assert chunks == [(0, len(sizes), 0, len(ttab))]
    itab = np.array([[clean[i].data_ptr() if clean else 0, degraded[i].data_ptr() if degraded else 0, h, w] for i, (h, w) in enumerate(sizes)],
                    dtype=np.int64)
    return dict(itab=_up(itab), ttab=_up(ttab), gtab=_up(gtab), gtab4=_up(gtab[:, :4]), sigma=_up(np.full(len(sizes), sigma, dtype=np.float32)),
                rows=[tuple(r) for r in ttab.tolist()], n=len(ttab))


def _share(err, tol):
    return float((err[tol > 0] / tol[tol > 0]).max())


def _gather(tb, seed=5, rows=None):
    from fwair.lib import call
    ttab, n = (tb['ttab'], tb['n']) if rows is None else (_up(np.array(rows, dtype=np.int32)), len(rows))
    tiles = torch.full((n, 3, T, T), -1.0, device=DEV)
    call('fw_restore_gather', tb['itab'], ttab, tb['sigma'], torch.tensor([seed], dtype=torch.int32, device=DEV), SITE, tiles, n, T)
    return tiles.cpu().numpy()


@pytest.mark.parametrize('overlap,nmodes', CASES)
def test_restore_gather_pairs_bit_equal_to_restatement(overlap, nmodes):
    gt, dg = RC.images(21, RC.SIZES), RC.noisy(RC.images(21, RC.SIZES), 5)
    clean, degraded = _dev(gt), _dev(dg)
    tb = _tables(clean, degraded, RC.SIZES, overlap, nmodes, sigma=25.0)                  # sigma is ignored where a degraded image is given
    out = _gather(tb)
    for t, (i, y0, x0, m) in enumerate(tb['rows']):
        assert np.array_equal(out[t], RC.gather(RC.unit(dg[i]), y0, x0, m, T)), f'tile {t}: image {i} at ({y0}, {x0}) mode {m}'


def test_restore_gather_origins_far_outside_the_image():
    """no origin reads outside the image: tiles above, left of, below and far beyond it, aligned (x0 % 4 == 0 inside a W % 4 == 0 image:
    the 4-wide path) and not, in every mode"""
    sizes = [(17, 40), (5, 7), (1, 16), (50, 23)]
    dg = RC.images(22, sizes)
    degraded = _dev(dg)
    tb = _tables(None, degraded, sizes, 0, 1)
    rows = [(i, y0, x0, m) for i, (h, w) in enumerate(sizes) for y0, x0 in
            [(-T - 3, -2 * T + 1), (h - 1, w + T + 5), (-7, 4), (h + 5, 8), (-1000, 1000), (0, 0), (1, 24 if w == 40 else 3)] for m in range(8)]
    out = _gather(tb, rows=rows)
    for t, (i, y0, x0, m) in enumerate(rows):
        assert np.array_equal(out[t], RC.gather(RC.unit(dg[i]), y0, x0, m, T)), f'tile {t}: image {i} at ({y0}, {x0}) mode {m}'


def test_restore_gather_synthesised_noise():
    """sigma 25, no degraded image: one noisy image behind every tile -- the overlap, the reflected pixels and the eight turns -- and
    that image is the oracle's up to the limits of test_eval_gather_synthesised_noise_vs_oracle"""
    gt = RC.images(23, RC.SIZES)
    clean = _dev(gt)
    seed_v, overlap = 31337, 5
    tb = _tables(clean, None, RC.SIZES, overlap, 8, sigma=25.0)
    out = _gather(tb, seed=seed_v)
    # the noisy image as the device drew it: unturned tiles at stride T (no overlap), cut to the image
    flat = _tables(clean, None, RC.SIZES, 0, 1, sigma=25.0)
    cut = _gather(flat, seed=seed_v)
    noisy = [np.full((3, h, w), -1.0, dtype=np.float32) for h, w in RC.SIZES]
    for t, (i, y0, x0, _) in enumerate(flat['rows']):
        h, w = RC.SIZES[i]
        hh, ww = min(T, h - y0), min(T, w - x0)
        old = noisy[i][:, y0:y0 + hh, x0:x0 + ww]
        assert ((old == -1.0) | (old == cut[t][:, :hh, :ww])).all(), 'overlapping tiles see the same noisy image'
        noisy[i][:, y0:y0 + hh, x0:x0 + ww] = cut[t][:, :hh, :ww]
    ndiff = tot = 0
    for i, g in enumerate(gt):
        assert noisy[i].min() >= 0
        z = D.hashed_normal(seed_v, SITE + i, g.size).reshape(g.shape)                      # counter = flat CHW index of the SOURCE pixel
        ref = RC.unit(np.clip(g + z * 25.0, 0, 255).astype(np.uint8))
        diff = np.abs(noisy[i] - ref) * 255
        assert diff.max() <= 1.0 + 1e-4, f'image {i}: off by {diff.max():.3f} grey levels'
        ndiff, tot = ndiff + int((diff > 1e-4).sum()), tot + diff.size
        if g.size > 1000:
            assert np.abs(noisy[i] - RC.unit(g)).max() > 0.1, 'noise is there'
    print(f'restore gather noise: {ndiff} of {tot} pixels differ from the oracle')
    assert ndiff / tot < 1e-3
    # every tile, reflected and turned, is cut from that one image, bit for bit
    for t, (i, y0, x0, m) in enumerate(tb['rows']):
        assert np.array_equal(out[t], RC.gather(noisy[i], y0, x0, m, T)), f'tile {t}: image {i} at ({y0}, {x0}) mode {m}'
        if m:
            assert np.array_equal(out[t], RC.turn(out[t - m], m)), f'tile {t}: mode {m} is the mode-0 tile turned'
    # sigma 0 without a degraded image: the clean image itself
    tb0 = _tables(clean, None, RC.SIZES, overlap, 8, sigma=0.0)
    out0 = _gather(tb0, seed=seed_v)
    for t, (i, y0, x0, m) in enumerate(tb0['rows']):
        assert np.array_equal(out0[t], RC.gather(RC.unit(gt[i]), y0, x0, m, T))


@pytest.mark.parametrize('sizes', SIZE_LISTS, ids=['sizes', 'aligned'])
@pytest.mark.parametrize('overlap,nmodes', CASES)
def test_restore_blend_identity_network(overlap, nmodes, sizes):
    """the gathered tiles blended as they are: the image comes back within (2 K + 4) 2^-24 max|v| (exactly at overlap 0 without the
    ensemble: a mean of at most four equal values), uint8 as image_io.py:383 makes it, PSNR / SSIM as the oracle computes them"""
    from fwair.lib import call
    gt, dg = RC.images(24, sizes), RC.noisy(RC.images(24, sizes), 6)
    clean, degraded = _dev(gt), _dev(dg)
    tb = _tables(clean, degraded, sizes, overlap, nmodes)
    rest = torch.from_numpy(_gather(tb)).to(DEV)
    I, px = len(sizes), sum(3 * h * w for h, w in sizes)
    packed = torch.full((px,), -1.0, device=DEV)
    u8 = torch.zeros(px, dtype=torch.uint8, device=DEV)
    sse, ssum = torch.zeros(I, device=DEV), torch.zeros(I, device=DEV)
    call('fw_restore_blend', tb['itab'], tb['gtab'], tb['ttab'], rest, packed, u8, sse, 0, I, tb['n'], T, max(overlap, 1))
    call('fw_eval_ssim7', tb['itab'], tb['gtab4'], packed, ssum, 0, I)
    packed, u8, sse, ssum = packed.cpu().numpy(), u8.cpu().numpy(), sse.cpu().numpy(), ssum.cpu().numpy()
    off = 0
    for i, (H, W) in enumerate(sizes):
        x = packed[off:off + 3 * H * W].reshape(3, H, W)
        want = RC.unit(dg[i])
        rows = [r for r in tb['rows'] if r[0] == i]
        ref, K, vmax = RC.blend(np.stack([RC.gather(want, y0, x0, m, T) for _, y0, x0, m in rows]), rows, H, W, T, max(overlap, 1))
        err, tol = np.abs(x.astype(np.float64) - want), RC.blend_bound(K, vmax)
        print(f'image {i} ({H} x {W}): K up to {K.max()}, max err / bound {_share(err, tol):.3f}')
        assert (err <= tol).all(), f'image {i}: {int((err > tol).sum())} pixels beyond the bound'
        assert (np.abs(x.astype(np.float64) - ref) <= tol).all()
        if overlap == 0 and nmodes == 1:
            assert np.array_equal(x, want), f'image {i}: a mean of equal values is exact'
        assert np.array_equal(u8[off:off + 3 * H * W].reshape(3, H, W), np.clip(x * 255, 0, 255).astype(np.uint8)), f'image {i}: uint8'
        g = RC.unit(gt[i])
        psnr = 10.0 * np.log10(3.0 * H * W / sse[i])
        if H >= 7 and W >= 7:
            rp, rs, _ = D.psnr_ssim(torch.from_numpy(x)[None], torch.from_numpy(g)[None])
            ssim = ssum[i] / (3.0 * (H - 6) * (W - 6))
            print(f'image {i}: psnr {psnr:.5f} (oracle {rp:.5f}), ssim {ssim:.6f} (oracle {rs:.6f})')
            assert abs(psnr - rp) < 1e-3 and abs(ssim - rs) < 1e-4
        else:                                                                    # no 7 x 7 window: data_oracle.psnr_ssim's PSNR alone
            rp = 10.0 * np.log10(1.0 / np.mean((np.clip(x, 0, 1).astype(np.float64) - g.astype(np.float64)) ** 2))
            assert abs(psnr - rp) < 1e-3 and ssum[i] == 0
        off += 3 * H * W


class _Stub(torch.nn.Module):
    """out = 0.5 x + ramp[c][i][j]: NOT equivariant under flips and rotations, and different at every position of the tile, so a swapped
    rotation direction, a wrong inverse or weights taken in the tile's frame show."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer('ramp', torch.from_numpy(self.table()))

    @staticmethod
    def table():
        return (np.random.RandomState(77).rand(3, T, T) * 0.5).astype(np.float32)

    def forward(self, x_query, x_key):
        return x_query * 0.5 + self.ramp

    @staticmethod
    def numpy(tile):
        return (tile * np.float32(0.5) + _Stub.table()).astype(np.float32)        # 0.5 x is exact: one rounding, as on the device


@pytest.fixture(scope='module', params=SIZE_LISTS, ids=['sizes', 'aligned'])
def stub_case(request):
    sizes = request.param
    gt, dg = RC.images(25, sizes), RC.noisy(RC.images(25, sizes), 7)
    return sizes, gt, dg, _dev(gt), _dev(dg), _Stub().to(DEV)


@pytest.mark.parametrize('ensemble', [False, True])
@pytest.mark.parametrize('overlap', RC.OVERLAPS)
def test_eval_engine_with_a_network_that_is_not_equivariant(stub_case, overlap, ensemble):
    from fwair.evaluate import EvalEngine
    sizes, gt, dg, clean, degraded, net = stub_case
    eng = EvalEngine(net, tile=T, tile_batch=7, use_graph=False, overlap=overlap, ensemble=ensemble, pad_small=True)
    p, s, u8, f32 = eng.run(clean, degraded, want_u8=True, want_f32=True)
    rows = RC.plan(sizes, T, overlap, 8 if ensemble else 1)
    for i, (H, W) in enumerate(sizes):
        assert f32[i].shape == u8[i].shape == (3, H, W)
        x = f32[i].cpu().numpy()
        ref, K, vmax = RC.restore(RC.unit(dg[i]), [r for r in rows if r[0] == i], H, W, T, max(overlap, 1), _Stub.numpy)
        err, tol = np.abs(x.astype(np.float64) - ref), RC.blend_bound(K, vmax)
        print(f'image {i} ({H} x {W}): K up to {K.max()}, max err / bound {_share(err, tol):.3f}')
        assert (err <= tol).all(), f'image {i}: {int((err > tol).sum())} pixels beyond the bound, max err {err.max():.3e}'
        assert np.array_equal(u8[i].cpu().numpy(), np.clip(x * 255, 0, 255).astype(np.uint8))
        rp = 10.0 * np.log10(1.0 / np.mean((np.clip(x, 0, 1).astype(np.float64) - RC.unit(gt[i]).astype(np.float64)) ** 2))
        assert abs(float(p[i]) - rp) < 1e-3
    if ensemble and overlap == 8:                      # the bound tells a wrong turn apart: the same tiles blended as if all were mode 0
        i = sizes.index((17, 40))
        H, W = sizes[i]
        mine = [r for r in rows if r[0] == i]
        rest = np.stack([_Stub.numpy(RC.gather(RC.unit(dg[i]), y0, x0, m, T)) for _, y0, x0, m in mine])
        wrong, K, vmax = RC.blend(rest, [(a, b, c, 0) for a, b, c, _ in mine], H, W, T, 8)
        assert (np.abs(f32[i].cpu().numpy() - wrong) > RC.blend_bound(K, vmax)).mean() > 0.9


@pytest.mark.parametrize('overlap,ensemble,chunk_tiles,tile_batch', [(5, False, 10, 5), (8, True, 96, 7), (0, False, 6, 4)])
def test_chunks_and_batches_do_not_change_the_result(overlap, ensemble, chunk_tiles, tile_batch):
    """a small tile buffer: images straddle tile batches, chunks close early, the last batch of a chunk is padded -- bit for bit the
    run that holds everything in one chunk"""
    from fwair.evaluate import EvalEngine
    gt, dg = RC.images(29, RC.SIZES), RC.noisy(RC.images(29, RC.SIZES), 9)
    clean, degraded, net = _dev(gt), _dev(dg), _Stub().to(DEV)
    kw = dict(tile=T, use_graph=False, overlap=overlap, ensemble=ensemble, pad_small=True)
    one = EvalEngine(net, tile_batch=64, chunk_tiles=4096, **kw)
    p1, s1, u1, f1 = one.run(clean, degraded, want_u8=True, want_f32=True)
    small = EvalEngine(net, tile_batch=tile_batch, chunk_tiles=chunk_tiles, **kw)
    p2, s2, u2, f2 = small.run(clean, degraded, want_u8=True, want_f32=True)
    (plan1,), (plan2,) = one._plans.values(), small._plans.values()
    assert plan1['ex'] and plan2['ex'] and len(plan1['chunks']) == 1 and len(plan2['chunks']) >= 3
    assert any((t1 - t0) % tile_batch for _, _, t0, t1 in plan2['chunks']), 'a padded last batch'
    for i in range(len(RC.SIZES)):
        assert torch.equal(f1[i], f2[i]) and torch.equal(u1[i], u2[i]), f'image {i}'
    assert float((p1 - p2).abs().max()) < 1e-5                  # the squared error is summed by atomics: the order is not fixed
    big = torch.zeros((3, 70, 70), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='the tile buffer holds'):
        EvalEngine(net, tile_batch=4, chunk_tiles=8, **kw).run(None, [big])


def test_defaults_are_the_old_path():
    """overlap=0, ensemble=False, no small image: the old tables and entries -- the same tensors as an engine that was not given the
    new arguments (restored images bit for bit; the two metrics are sums of atomics, equal up to the order of their terms)"""
    from fwair.evaluate import EvalEngine
    from test_folder_eval_gpu import SIZES, _Identity

    class Affine(_Identity):
        def forward(self, x_query, x_key):
            return x_query * 1.3 - 0.1

    gt, dg = RC.images(26, SIZES), RC.noisy(RC.images(26, SIZES), 8)
    clean, degraded = _dev(gt), _dev(dg)
    net = Affine().to(DEV)
    old = EvalEngine(net, 128, 5, False, 10)
    new = EvalEngine(net, 128, 5, False, 10, overlap=0, ensemble=False)
    new_pad = EvalEngine(net, 128, 5, False, 10, overlap=0, ensemble=False, pad_small=True)
    res = [e.run(clean, degraded, want_u8=True, want_f32=True) for e in (old, new, new_pad)]
    for e in (old, new, new_pad):
        (plan,) = e._plans.values()
        assert not plan['ex'] and plan['gtab'].shape[1] == 4 and int(plan['ttab'][:, 3].abs().max()) == 0
    for r in res[1:]:
        for i in range(4):
            assert torch.equal(r[2][i], res[0][2][i]) and torch.equal(r[3][i], res[0][3][i]), f'image {i}'
        assert torch.allclose(r[0], res[0][0], rtol=0, atol=1e-5) and torch.allclose(r[1], res[0][1], rtol=0, atol=1e-5)
    # and the new entries at overlap 0 compute the same images (the plain mean), from their own tables
    ex = EvalEngine(net, 128, 5, False, 10, overlap=0, ensemble=False, pad_small=True)
    small = torch.zeros((3, 8, 8), dtype=torch.uint8, device=DEV)
    r = ex.run(clean + [small], degraded + [small], want_u8=True, want_f32=True)
    assert list(ex._plans.values())[0]['ex']
    for i in range(4):
        assert torch.equal(r[2][i], res[0][2][i]) and torch.equal(r[3][i], res[0][3][i]), f'image {i}: new entries'


def test_refused_calls_write_nothing():
    from fwair.lib import call
    sizes = [(17, 40)]
    dg = RC.images(27, sizes)
    degraded = _dev(dg)
    tb = _tables(degraded, degraded, sizes, 0, 1)
    n, px = tb['n'], 3 * 17 * 40
    seed = torch.tensor([1], dtype=torch.int32, device=DEV)
    tiles = torch.full((n, 3, T, T), 7.0, device=DEV)
    for args in ([tb['itab'], tb['ttab'], tb['sigma'], seed, SITE, tiles, n, 6],
                 [None, tb['ttab'], tb['sigma'], seed, SITE, tiles, n, T],
                 [tb['itab'], None, tb['sigma'], seed, SITE, tiles, n, T],
                 [tb['itab'], tb['ttab'], tb['sigma'], seed, SITE, tiles.view(-1)[1:], n, T],          # not 16-byte aligned
                 [tb['itab'], tb['ttab'], tb['sigma'], seed, SITE, tiles, 65536, T]):
        with pytest.raises(RuntimeError, match='argument check'):
            call('fw_restore_gather', *args)
    torch.cuda.synchronize()
    assert bool((tiles == 7.0).all())
    rest = torch.rand((n, 3, T, T), device=DEV)
    packed = torch.full((px,), 7.0, device=DEV)
    u8 = torch.full((px,), 7, dtype=torch.uint8, device=DEV)
    sse = torch.full((1,), 7.0, device=DEV)
    good = [tb['itab'], tb['gtab'], tb['ttab'], rest, packed, u8, sse, 0, 1, n, T, 1]
    for pos, val in ((10, 6), (11, 0), (11, T // 2 + 1), (11, -1), (3, None), (4, None), (0, None), (6, None), (8, 65536)):
        bad = list(good)
        bad[pos] = val
        if pos == 10:
            bad[11] = 1
        with pytest.raises(RuntimeError, match='argument check'):
            call('fw_restore_blend', *bad)
    torch.cuda.synchronize()
    assert bool((packed == 7.0).all()) and bool((u8 == 7).all()) and float(sse[0]) == 7.0
    for ramp in (1, T // 2):                                                       # the limits themselves are accepted
        call('fw_restore_blend', tb['itab'], tb['gtab'], tb['ttab'], rest, packed, u8, sse, 0, 1, n, T, ramp)
    torch.cuda.synchronize()
    assert bool((packed != 7.0).all())


@pytest.fixture(scope='module')
def seeded():
    from net.model import AirNet
    opt = make_opt('all3')
    net = AirNet(opt)
    st = O.fill_state_seeded(schema('all3'))
    sd = net.state_dict()
    for k in sd:
        if st.get(k) is not None and sd[k].is_floating_point():
            sd[k] = st[k]
    net.load_state_dict(sd)
    return net.to(DEV).eval()


def test_real_network_overlap_ensemble_graph_vs_eager(seeded):
    """the seeded model at tile 128, a 136 x 200 and a 100 x 90 image, overlap 32 with the ensemble: 32 + 8 tiles in batches of 8;
    HIP-graph replay against eager launches at the tolerance of test_eval_engine_graph_vs_eager, output shapes = input shapes"""
    from fwair.evaluate import EvalEngine
    sizes = [(136, 200), (100, 90)]
    clean = _dev(RC.images(28, sizes))
    res = []
    for use_graph in (True, False):
        eng = EvalEngine(seeded, tile=128, tile_batch=8, use_graph=use_graph, overlap=32, ensemble=True, pad_small=True)
        res.append(eng.run(clean, sigma=25, seed=7, want_u8=True, want_f32=True))
        assert eng.use_graph == use_graph, 'the capture fell back to eager launches'
        (plan,) = eng._plans.values()
        assert plan['ex'] and plan['chunks'] == [(0, 2, 0, 40)]
    (pg, sg, ug, fg), (pe, se, ue, fe) = res
    for i, (h, w) in enumerate(sizes):
        assert fg[i].shape == ug[i].shape == (3, h, w) and ug[i].dtype == torch.uint8
        close(fg[i], fe[i], 1e-4, f'image {i}: graph vs eager')
        assert bool(torch.isfinite(fg[i]).all())
    print('graph vs eager: psnr diff', float((pg - pe).abs().max()), 'ssim diff', float((sg - se).abs().max()))
    assert float((pg - pe).abs().max()) < 1e-5 and float((sg - se).abs().max()) < 1e-5
