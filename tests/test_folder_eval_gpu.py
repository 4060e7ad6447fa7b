"""Batched device evaluation (csrc/fw_data.hip: fw_eval_gather / fw_eval_blend / fw_eval_ssim7; fwair/evaluate.py: EvalEngine) against
the per-image kernels and the CPU oracle (oracle/data_oracle.py around oracle/airnet_oracle.py):
  * fw_eval_gather from uint8 pairs: bit-equal to fw_tile_gather on u8 / 255; with in-kernel noise: the oracle's f64 evaluation of the
    same counter-based draws up to one grey level on a < 1e-3 fraction of the pixels (the limits of test_train_batch_vs_oracle), and
    overlapping tiles agree exactly;
  * fw_eval_blend / fw_eval_ssim7 fed the gathered tiles themselves (an identity "network"): exact images, exact uint8, oracle metrics;
  * EvalEngine around the HIP network against the oracle's test.py loops around the ORACLE network, images straddling batches and
    chunks, the last batch padded; HIP-graph replay against eager launches; no host synchronisation inside run()."""
import time

import numpy as np
import pytest
import torch

import airnet_oracle as O
import data_oracle as D
from helpers import close, make_opt, schema

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = [(200, 248), (128, 128), (136, 272), (128, 300)]              # 4 + 1 + 6 + 3 = 14 tiles of 128


def _images(seed, sizes):                                             # the generator of tests/test_data_gpu.py:_images
    rs = np.random.RandomState(seed)
    out = []
    for (h, w) in sizes:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        img = np.stack([127 + 90 * np.sin(xx / (7 + c) + yy / (11 + 2 * c)) + rs.randn(h, w) * 12 for c in range(3)])
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def _noisy(imgs, seed, sigma=25):
    rs = np.random.RandomState(seed)
    return [np.clip(i + rs.randn(*i.shape) * sigma, 0, 255).astype(np.uint8) for i in imgs]


def _dev(imgs):
    return [torch.from_numpy(i).to(DEV) for i in imgs]


def _tables(clean, degraded, sigma):
    from fwair.evaluate import plan_tiles
    sizes = [tuple(t.shape[1:]) for t in clean]
    ttab, gtab, chunks = plan_tiles(sizes, 128, 64)
    itab = np.array([[clean[i].data_ptr(), degraded[i].data_ptr() if degraded else 0, sizes[i][0], sizes[i][1]] for i in range(len(clean))],
                    dtype=np.int64)
    up = lambda a: torch.from_numpy(a).to(DEV)
    return up(itab), up(ttab), up(gtab), up(np.full(len(clean), sigma, dtype=np.float32)), ttab, chunks


def test_eval_gather_pairs_bit_equal_to_tile_gather():
    from fwair.evaluate import tile_origins
    from fwair.lib import call
    gt, dg = _images(11, SIZES), _noisy(_images(11, SIZES), 3)
    clean, degraded = _dev(gt), _dev(dg)
    itab, ttab, _, sigma, ttab_h, chunks = _tables(clean, degraded, 25.0)          # sigma is ignored where a degraded image is given
    assert chunks == [(0, 4, 0, 14)]
    seed = torch.tensor([5], dtype=torch.int32, device=DEV)
    tiles = torch.full((14, 3, 128, 128), -1.0, device=DEV)
    call('fw_eval_gather', itab, ttab, sigma, seed, 0x7B000000, tiles, 14, 128)
    t = 0
    for i, (H, W) in enumerate(SIZES):
        ys, xs = tile_origins(H, 128), tile_origins(W, 128)
        # u8 / 255 as ToTensor divides (correctly rounded, numpy); a device-side `tensor / 255` may multiply by the rounded reciprocal
        img = torch.from_numpy(dg[i].astype(np.float32) / 255.0).to(DEV)
        ref = torch.empty((len(ys) * len(xs), 3, 128, 128), device=DEV)
        call('fw_tile_gather', img, torch.tensor(ys, dtype=torch.int32, device=DEV), torch.tensor(xs, dtype=torch.int32, device=DEV), ref,
             3, H, W, len(ys), len(xs), 128)
        assert torch.equal(tiles[t:t + ref.shape[0]], ref), f'image {i}'
        t += ref.shape[0]
    assert t == 14


def test_eval_gather_synthesised_noise_vs_oracle():
    from fwair.lib import call
    gt = _images(12, SIZES)
    clean = _dev(gt)
    itab, ttab, _, sigma, ttab_h, _ = _tables(clean, None, 25.0)
    seed_v, site = 31337, 0x7B000000
    seed = torch.tensor([seed_v], dtype=torch.int32, device=DEV)
    tiles = torch.empty((14, 3, 128, 128), device=DEV)
    call('fw_eval_gather', itab, ttab, sigma, seed, site, tiles, 14, 128)
    out = tiles.cpu().numpy()
    ref = np.empty_like(out)
    noisy = []
    for i, g in enumerate(gt):
        z = D.hashed_normal(seed_v, site + i, g.size).reshape(g.shape)              # counter = flat CHW pixel index of the full image
        noisy.append(np.clip(g + z * 25.0, 0, 255).astype(np.uint8).astype(np.float32) / 255.0)
    for t, (i, y0, x0, _) in enumerate(ttab_h.tolist()):
        ref[t] = noisy[i][:, y0:y0 + 128, x0:x0 + 128]
    diff = np.abs(out - ref) * 255
    print(f'eval gather noise: max {diff.max():.4f} grey levels, {(diff > 1e-4).mean():.2e} of the pixels differ')
    assert diff.max() <= 1.0 + 1e-4, f'off by {diff.max():.3f} grey levels'
    assert (diff > 1e-4).mean() < 1e-3, f'{(diff > 1e-4).mean():.2e} of the pixels differ'
    assert np.abs(out - np.stack([gt[i][:, y0:y0 + 128, x0:x0 + 128] for i, y0, x0, _ in ttab_h.tolist()]) / 255.0).max() > 0.1   # noise is there
    # image 0 (200 x 248): tiles 0 / 1 start at x = 0 / 120, tiles 0 / 2 at y = 0 / 72 -- the overlap is the same noisy image
    assert ttab_h[:4].tolist() == [[0, 0, 0, 0], [0, 0, 120, 0], [0, 72, 0, 0], [0, 72, 120, 0]]
    assert np.array_equal(out[0][:, :, 120:], out[1][:, :, :8])
    assert np.array_equal(out[0][:, 72:, :], out[2][:, :56, :])
    # sigma 0 without a degraded image: the clean image itself
    call('fw_eval_gather', itab, ttab, torch.zeros_like(sigma), seed, site, tiles, 14, 128)
    assert np.array_equal(tiles[4].cpu().numpy(), gt[1].astype(np.float32) / 255.0)


class _Identity(torch.nn.Module):
    """A "network" that returns its tiles: EvalEngine then blends the gathered tiles themselves."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x_query, x_key):
        return x_query.clone()


@pytest.mark.parametrize('chunk_tiles', [15, 10])
def test_eval_blend_and_ssim_on_gathered_tiles(chunk_tiles):
    """chunk_tiles 10: two chunks ([0, 2) with 5 tiles, [2, 4) with 9), batches of 5 straddle images, the last batch is padded."""
    from fwair.evaluate import EvalEngine
    gt, dg = _images(13, SIZES), _noisy(_images(13, SIZES), 4)
    clean, degraded = _dev(gt), _dev(dg)
    eng = EvalEngine(_Identity().to(DEV), tile=128, tile_batch=5, use_graph=False, chunk_tiles=chunk_tiles)
    p, s, u8, f32 = eng.run(clean, degraded, want_u8=True, want_f32=True)
    assert p.is_cuda and s.is_cuda and p.shape == s.shape == (4,)
    for i in range(4):
        x = f32[i].cpu().numpy()
        assert np.array_equal(x, dg[i].astype(np.float32) / 255.0), f'image {i}: an average of equal values is exact'
        assert np.array_equal(u8[i].cpu().numpy(), np.clip(x * 255, 0, 255).astype(np.uint8)), f'image {i}: uint8'
        rp, rs, _ = D.psnr_ssim(torch.from_numpy(x)[None], torch.from_numpy(gt[i].astype(np.float32) / 255.0)[None])
        print(f'image {i}: psnr {float(p[i]):.5f} (oracle {rp:.5f}), ssim {float(s[i]):.6f} (oracle {rs:.6f})')
        assert abs(float(p[i]) - rp) < 1e-3 and abs(float(s[i]) - rs) < 1e-4


def test_eval_blend_uint8_truncates_and_clips():
    """image_io.py:383 on values outside [0, 1] and between grey levels."""
    from fwair.evaluate import EvalEngine

    class Affine(_Identity):
        def forward(self, x_query, x_key):
            return x_query * 1.3 - 0.1

    gt = _images(14, [(128, 136)])
    eng = EvalEngine(Affine().to(DEV), tile=128, tile_batch=2, use_graph=False)
    _, _, u8, f32 = eng.run(_dev(gt), want_u8=True, want_f32=True)
    x = f32[0].cpu().numpy()
    assert x.min() < 0 and x.max() > 1
    assert np.array_equal(u8[0].cpu().numpy(), np.clip(x * 255, 0, 255).astype(np.uint8))


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
    return net.to(DEV).eval(), opt, st


def test_eval_engine_vs_oracle_network(seeded):
    """fp32, tile_batch 5 over 14 tiles (5 + 5 + 4 padded with one copy), two chunks: every restored image and both metrics against
    oracle/data_oracle.tiled_restore around oracle/airnet_oracle.airnet_forward."""
    from fwair.evaluate import EvalEngine
    net, opt, st = seeded
    gt, dg = _images(15, SIZES), _noisy(_images(15, SIZES), 6)
    eng = EvalEngine(net, tile=128, tile_batch=5, use_graph=True, chunk_tiles=10)
    p, s, f32 = eng.run(_dev(gt), _dev(dg), want_f32=True)
    for i in range(4):
        img = torch.from_numpy(dg[i].astype(np.float32) / 255.0)[None]
        with torch.no_grad():
            ref = D.tiled_restore(lambda t: O.airnet_forward(st, opt, t, t, False), img, 128)
        err = close(f32[i][None], ref, 1e-4, f'image {i}: restored vs oracle')
        rp, rs, _ = D.psnr_ssim(ref, torch.from_numpy(gt[i].astype(np.float32) / 255.0)[None])
        print(f'image {i}: err {err:.2e}, psnr {float(p[i]):.5f} (oracle {rp:.5f}), ssim {float(s[i]):.6f} (oracle {rs:.6f})')
        assert abs(float(p[i]) - rp) < 1e-3 and abs(float(s[i]) - rs) < 1e-4


def test_eval_engine_graph_vs_eager(seeded):
    from fwair.evaluate import EvalEngine
    net, _, _ = seeded
    clean = _dev(_images(16, SIZES))
    res = []
    for use_graph in (True, False):
        eng = EvalEngine(net, tile=128, tile_batch=5, use_graph=use_graph)
        res.append(eng.run(clean, sigma=25, seed=7, want_f32=True))          # in-kernel noise, same seed: the same noisy images
        assert eng.use_graph == use_graph, 'the capture fell back to eager launches'
    (pg, sg, fg), (pe, se, fe) = res
    for i in range(4):
        close(fg[i], fe[i], 1e-4, f'image {i}: graph vs eager')
    print('graph vs eager: psnr diff', float((pg - pe).abs().max()), 'ssim diff', float((sg - se).abs().max()))
    assert float((pg - pe).abs().max()) < 1e-5 and float((sg - se).abs().max()) < 1e-5
    p2, _ = EvalEngine(net, tile=128, tile_batch=5, use_graph=False).run(clean, sigma=25, seed=8)
    assert float((p2 - pe).abs().max()) > 1e-4, 'another seed, another noise'


def test_eval_engine_run_does_not_wait_for_the_device(seeded):
    from fwair.evaluate import EvalEngine
    net, _, _ = seeded
    clean = _dev(_images(17, SIZES))
    eng = EvalEngine(net, tile=128, tile_batch=5, use_graph=True)
    eng.run(clean, sigma=25)                                              # warm-up: tables uploaded, graph captured
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, s = eng.run(clean, sigma=25)
    t_issue = time.perf_counter() - t0                                    # host time to ISSUE the run: no sync inside means launch cost only
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print(f'EvalEngine.run: host issue {t_issue * 1e3:.2f} ms, until the device is done {t_all * 1e3:.2f} ms')
    assert p.is_cuda and s.is_cuda and bool(torch.isfinite(p).all()) and bool(((s > 0) & (s < 1)).all())
    assert t_issue < 0.5 * t_all
