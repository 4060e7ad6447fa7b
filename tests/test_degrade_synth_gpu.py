"""fw_train_batch_synth (csrc/fw_data.hip) through fwair.augment.DeviceBatcher(synth='kernel'): rain, haze and motion blur made inside the
batch launch, bit for bit against the numpy restatement of tests/degrade_cases.py; one degraded image per sample, fresh rain per slot
and call; the default batcher untouched; synthesize_u8; the rate of the mixed `4tasks` batch; the driver's --synthesize_tasks."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import degrade_cases as DC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
S = 32
SEED = 31337
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd')


@pytest.fixture()
def frozen_seed():
    from fwair import functional as Fn
    Fn.set_dropout_seed(SEED, DEV, frozen=True)
    try:
        yield SEED
    finally:
        Fn.set_dropout_seed(1, DEV, frozen=False)


def _records():
    """Every parameter extreme of the three degradations, then the two kinds of code-0 slot: 20 records, padded to 32 slots."""
    from fwair.augment import synth_record as rec
    out = [('blur', rec('deblurring', a, n)) for n in (1, 3, 25) for a in (0, 7, 16, 31)]
    out += [('rain', rec('deraining', a, L, 4096, s8)) for (a, L) in ((5, 1), (11, 32)) for s8 in (0, 255)]
    out += [('haze', rec('dehazing', j)) for j in (0, 15)]
    out += [('noise', [0] * 8), ('given', [0] * 8)]
    out += [('rain', rec('deraining', 8, 32, 4096, 255)), ('blur', rec('deblurring', 23, 25)), ('haze', rec('dehazing', 9, 100)),
            ('noise', [0] * 8), ('given', [0] * 8), ('rain', rec('deraining', 0, 32, 4096, 255)), ('blur', rec('deblurring', 16, 25)),
            ('rain', rec('deraining', 16, 32, 4096, 255)), ('blur', rec('deblurring', 0, 25)), ('rain', rec('deraining', 31, 32, 4096, 255)),
            ('blur', rec('deblurring', 9, 13)), ('haze', rec('dehazing', 4, 255))]
    assert len(out) == 32
    return out[0::2] + out[1::2]                     # both batches of 16 mix the codes


def _rnd(H, W, shift):
    """[16][9]: all 7 modes in each view; origins at 0, at H - S / W - S and in between, different for the two views."""
    ys, xs = [0, H - S, (H - S) // 2, min(1, H - S)], [W - S, 0, min(3, W - S), (W - S) // 2]
    rows = []
    for b in range(16):
        k = b + shift
        rows.append([ys[k % 4], xs[(k // 2) % 4], k % 7, ys[(k + 1) % 4], xs[(k + 3) % 4], (k + 3) % 7, 0, 0, 0])
    r = np.array(rows, dtype=np.int32)
    assert set(1 + r[:, 2] % 7) == set(1 + r[:, 5] % 7) == set(range(1, 8))
    assert {0, H - S} <= set(r[:, 0]) | set(r[:, 3]) and {0, W - S} <= set(r[:, 1]) | set(r[:, 4])
    return r


@pytest.mark.parametrize('H,W', [(32, 32), (33, 47), (40, 64), (96, 80)])
def test_bit_exact_vs_restatement(H, W, frozen_seed):
    from fwair import augment as A
    imgs = DC.images(10 + H, [(H, W)] * 4)
    given = DC.images(20 + H, [(H, W)])[0]
    dev_imgs = [torch.from_numpy(i).to(DEV) for i in imgs]
    # index 0: noise 25 | 1: a pair on file | 2, 3: synthesised (the explicit records decide the task of a slot)
    bt = A.DeviceBatcher(dev_imgs, [25, 'deraining', 'deblurring', 'deraining'], S, synth='kernel',
                         degraded_u8=[None, torch.from_numpy(given).to(DEV), None, None])
    assert bt.synth and bt.degraded[2] is None and bt.degraded[3] is None
    recs = _records()
    seen_sat = False
    for half in range(2):
        kinds = [k for k, _ in recs[16 * half:16 * half + 16]]
        params = np.array([r for _, r in recs[16 * half:16 * half + 16]], dtype=np.int32)
        idx = [0 if k == 'noise' else 1 if k == 'given' else 2 + (s & 1) for s, k in enumerate(kinds)]
        rnd = _rnd(H, W, 5 * half)
        out = [t.cpu().numpy() for t in bt.batch(idx, rnd=rnd, params=params)]
        assert np.array_equal(bt.last_rnd.cpu().numpy(), rnd) and np.array_equal(bt.last_params.cpu().numpy(), params)
        ref, full = DC.train_batch([imgs[i] for i in idx], [given if i == 1 else None for i in idx], [bt.sigma[i] for i in idx],
                                   rnd, params, SEED, bt.last_site, S)
        for s, kind in enumerate(kinds):
            if kind == 'rain' and params[s][4] == 255:                          # the restatement itself: many streaks, some saturation
                _, seeds = DC.rain_layer(H, W, int(params[s][1]), int(params[s][2]), 4096, DC.site_key(SEED, bt.last_site + s))
                for v in range(2):
                    y0, x0 = rnd[s][3 * v] % (H - S + 1), rnd[s][3 * v + 1] % (W - S + 1)
                    assert seeds[y0:y0 + S, x0:x0 + S].sum() >= 24, (s, v)
                seen_sat |= bool(((full[s] == 255) & (imgs[idx[s]] < 255)).any())
                assert (full[s] > imgs[idx[s]]).mean() > 0.05
        noise = [s for s, k in enumerate(kinds) if k == 'noise']
        exact = [s for s, k in enumerate(kinds) if k != 'noise']
        for name, a, b in zip(('degrad_patch_1', 'degrad_patch_2', 'clean_patch_1', 'clean_patch_2'), out, ref):
            assert a.shape == b.shape == (16, 3, S, S) and a.dtype == np.float32
            if name.startswith('clean'):
                assert np.array_equal(a, b), name
                continue
            for s in exact:
                assert np.array_equal(a[s], b[s]), f'{name}[{s}] ({kinds[s]} {params[s][:5].tolist()}) at {H}x{W}: ' \
                                                  f'{(a[s] != b[s]).sum()} values differ, by up to {np.abs(a[s] - b[s]).max() * 255:.0f} levels'
            diff = np.abs(a[noise] - b[noise]) * 255                            # f32 vs f64 Box-Muller at a truncation boundary
            assert diff.max() <= 1.0 + 1e-4, f'{name}: noise off by {diff.max():.3f} grey levels'
            assert (diff > 1e-4).mean() < 1e-3, f'{name}: {(diff > 1e-4).mean():.2e} of the noisy pixels differ'
            assert not np.array_equal(a[noise], out[2 if name.endswith('1') else 3][noise])
    assert seen_sat


def _unturn(view, mode):
    py, px = DC.mode_preimage(mode, S)
    out = np.empty_like(view)
    out[:, py, px] = view
    return out


def test_both_views_cut_one_image(frozen_seed):
    from fwair import augment as A
    from fwair.augment import synth_record as rec
    H, W = 40, 64
    imgs = DC.images(31, [(H, W)])
    bt = A.DeviceBatcher([torch.from_numpy(imgs[0]).to(DEV)], ['deraining'], S, synth='kernel')
    params = np.array([rec('deraining', 7, 32, 4096, 255), rec('deblurring', 7, 25), rec('dehazing', 15),
                       rec('deraining', 7, 32, 4096, 255), rec('deblurring', 7, 25), rec('dehazing', 15)], dtype=np.int32)
    rnd = np.array([[3, 9, 4, 3, 9, 4, 0, 0, 0]] * 3 + [[0, 0, 2, 5, 9, 5, 0, 0, 0]] * 3, dtype=np.int32)
    d1, d2, c1, c2 = [t.cpu().numpy() for t in bt.batch([0] * 6, rnd=rnd, params=params)]
    for s in range(3):                                                          # the same origin and mode
        assert np.array_equal(d1[s], d2[s]) and not np.array_equal(d1[s], c1[s])
    for s in range(3, 6):                                                       # origins (0, 0) and (5, 9), modes 3 and 6
        u1, u2 = _unturn(d1[s], 1 + 2 % 7), _unturn(d2[s], 1 + 5 % 7)
        assert np.array_equal(u1[:, 5:, 9:], u2[:, :S - 5, :S - 9])
        assert not np.array_equal(u1, u2) and not np.array_equal(d1[s], c1[s])
        assert np.array_equal(_unturn(c1[s], 3)[:, 5:, 9:], _unturn(c2[s], 6)[:, :S - 5, :S - 9])


def test_rain_is_fresh_blur_and_haze_repeat(frozen_seed):
    from fwair import augment as A
    from fwair.augment import synth_record as rec
    imgs = DC.images(32, [(40, 64)])
    bt = A.DeviceBatcher([torch.from_numpy(imgs[0]).to(DEV)], ['deraining'], S, synth='kernel')
    params = np.array([rec('deraining', 8, 16, 4096, 255)] * 2 + [rec('deblurring', 5, 9)] * 2 + [rec('dehazing', 3)] * 2, dtype=np.int32)
    rnd = np.array([[2, 17, 1, 6, 30, 4, 0, 0, 0]] * 6, dtype=np.int32)
    first = [t.cpu().numpy() for t in bt.batch([0] * 6, rnd=rnd, params=params)]
    site = bt.last_site
    second = [t.cpu().numpy() for t in bt.batch([0] * 6, rnd=rnd, params=params)]
    assert bt.last_site != site
    for d_a, d_b in zip(first[:2], second[:2]):
        assert not np.array_equal(d_a[0], d_a[1])                               # the same index in two slots: another rain layer
        assert not np.array_equal(d_a[0], d_b[0])                               # and in the next call
        assert np.array_equal(d_a[2], d_a[3]) and np.array_equal(d_a[2], d_b[2])           # blur with equal parameters
        assert np.array_equal(d_a[4], d_a[5]) and np.array_equal(d_a[4], d_b[4])           # haze
    assert np.array_equal(first[2], second[2]) and np.array_equal(first[2][0], first[2][1])


def test_default_batcher_is_untouched(frozen_seed):
    from fwair import augment as A
    imgs = DC.images(33, [(50, 70), (32, 100), (64, 64), (33, 32), (81, 50)])
    tasks = [25, 'denoising_15', 'deraining', 'dehazing', 50]
    dev_imgs = [torch.from_numpy(i).to(DEV) for i in imgs]
    idx = [4, 0, 1, 2, 3, 0, 2]
    runs = []
    for kw in ({}, {'synth': 'once'}):
        host = torch.Generator().manual_seed(5)
        bt = A.DeviceBatcher(dev_imgs, tasks, S, generator=host, **kw)
        g = torch.Generator(device=DEV).manual_seed(9)
        out = bt.batch(idx, generator=g)
        runs.append((bt, out, torch.rand(3, generator=host), torch.randint(0, 1000, (5,), device=DEV, generator=g).cpu()))
        assert not bt.synth and bt.last_params is None and bt.code == [0] * 5
        assert bt.last_rnd.shape == (7, 7)
    (b1, o1, h1, p1), (b2, o2, h2, p2) = runs
    assert torch.equal(b1.last_rnd, b2.last_rnd) and b1.last_site == b2.last_site
    assert all(torch.equal(a, b) for a, b in zip(o1, o2))
    assert torch.equal(h1, h2) and torch.equal(p1, p2)
    # the construction drew what degrade() draws for the two paired tasks, the batch ONE [B, 7] randint: probes of fresh generators agree
    host = torch.Generator().manual_seed(5)
    rain, hz = A.degrade(dev_imgs[2], 'deraining', host), A.degrade(dev_imgs[3], 'dehazing', host)
    assert torch.equal(b1.degraded[2], rain) and torch.equal(b1.degraded[3], hz) and torch.equal(torch.rand(3, generator=host), h1)
    g = torch.Generator(device=DEV).manual_seed(9)
    rnd = torch.randint(0, 2 ** 31 - 1, (7, 7), dtype=torch.int32, device=DEV, generator=g)
    assert torch.equal(rnd, b1.last_rnd) and torch.equal(torch.randint(0, 1000, (5,), device=DEV, generator=g).cpu(), p1)
    # and its outputs are fw_train_batch's: the same slots through the new entry with code 0 everywhere agree bit for bit
    o3 = b1.batch(idx, rnd=b1.last_rnd[:, :7], params=np.zeros((7, 8), np.int32))
    assert b1.last_site != b2.last_site
    for s in (3, 4, 6):                                                         # the slots without noise (the noise follows the call's site)
        assert all(torch.equal(a[s], b[s]) for a, b in zip(o1, o3))


def test_kernel_batcher_draws_records_and_keeps_no_image(frozen_seed):
    from fwair import augment as A
    imgs = [torch.from_numpy(i).to(DEV) for i in DC.images(34, [(48, 64)] * 8)]
    tasks = ['denoising_0', 'deraining', 'dehazing', 'deblurring'] * 2
    bt = A.DeviceBatcher(imgs, tasks, S, synth='kernel')
    assert all(d is None for d in bt.degraded) and bt.code == [0, 1, 2, 3] * 2
    g = torch.Generator(device=DEV).manual_seed(3)
    seen = set()
    for _ in range(24):
        out = bt.batch(list(range(8)), generator=g)
        p, r = bt.last_params.cpu().numpy(), bt.last_rnd.cpu().numpy()
        assert r.shape == (8, 9) and p.shape == (8, 8) and p.dtype == np.int32
        for b in range(8):
            code, p1, p2, p3, p4 = p[b][:5]
            assert code == b % 4 and not p[b][5:].any()
            if code == 0:
                assert not p[b][1:].any()
            elif code == 1:
                assert p1 == 5 + r[b][7] % 7 and (p2, p3, p4) == (A.rain_length(S), 164, 179)
            elif code == 2:
                assert p1 == r[b][7] % 16 and (p2, p3, p4) == (204, 0, 0)
            else:
                assert p1 == r[b][7] % 32 and p2 == 7 + 2 * (r[b][8] % 10) and 7 <= p2 <= 25 and (p3, p4) == (0, 0)
            seen.add((code, p1, p2))
    assert len({k for k in seen if k[0] == 3}) > 12 and len({k for k in seen if k[0] == 1}) > 3
    d1, d2, c1, c2 = [t.cpu().numpy() for t in out]
    sig = bt.last_sigma.cpu().numpy()
    assert set(sig[[0, 4]]) <= {15.0, 25.0, 50.0} and not sig[[1, 2, 3, 5, 6, 7]].any()
    for b in range(8):
        assert not np.array_equal(d1[b], c1[b])                                 # every task degrades
    ref, _ = DC.train_batch([i.cpu().numpy() for i in imgs], [None] * 8, sig, r, p, SEED, bt.last_site, S)
    for s in (1, 2, 3, 5, 6, 7):
        assert np.array_equal(d1[s], ref[0][s]) and np.array_equal(d2[s], ref[1][s])
    # ONE RNG call per batch: a fresh generator's single [B, 9] draw is the first batch's
    g1 = torch.Generator(device=DEV).manual_seed(3)
    bt.batch(list(range(8)), generator=g1)
    g2 = torch.Generator(device=DEV).manual_seed(3)
    assert torch.equal(bt.last_rnd, torch.randint(0, 2 ** 31 - 1, (8, 9), dtype=torch.int32, device=DEV, generator=g2))
    assert torch.equal(torch.randint(0, 9, (4,), device=DEV, generator=g1), torch.randint(0, 9, (4,), device=DEV, generator=g2))


@pytest.mark.parametrize('task,params', [('deraining', (9, 32, 4096, 255)), ('dehazing', (15,)), ('deblurring', (7, 25))])
def test_synthesize_u8(task, params):
    from fwair import augment as A
    img = DC.images(35, [(33, 47)])[0]
    out = A.synthesize_u8(torch.from_numpy(img).to(DEV), task, params, 4242, 0x7A000300)
    assert out.dtype == torch.uint8 and out.shape == (3, 33, 47)
    ref = DC.degrade_image(img, A.synth_record(task, *params), 4242, 0x7A000300)
    assert np.array_equal(out.cpu().numpy(), ref) and not np.array_equal(ref, img)


def test_mixed_4tasks_rate_and_no_host_sync():
    """The loop and the bar of test_data_gpu.test_input_pipeline_rate_and_no_host_sync, on the mixed `4tasks` batch."""
    from fwair import augment as A
    imgs = [torch.from_numpy(i).to(DEV) for i in DC.images(4, [(256, 256)] * 64)]
    bt = A.DeviceBatcher(imgs, ['denoising_0', 'deraining', 'dehazing', 'deblurring'] * 16, 128, synth='kernel')
    idx = [list(range(k, k + 16)) for k in range(0, 64, 16)]
    g = torch.Generator(device=DEV).manual_seed(1)
    for i in range(8):
        bt.batch(idx[i % 4], generator=g)
    torch.cuda.synchronize()
    n = 200
    t0 = time.perf_counter()
    with torch.autograd.profiler.profile(enabled=False):
        for i in range(n):
            bt.batch(idx[i % 4], generator=g)
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    rate = 16 * n / t_all
    print(f'device input pipeline, 4tasks in the kernel: {rate:.0f} images/s ({t_all / n * 1e6:.0f} us per batch of 16; '
          f'host issue {t_issue / n * 1e6:.0f} us)')
    assert rate > 18000, 'the input pipeline must not bound a 1 800 images/s training step'
    assert t_issue < t_all


def test_driver_trains_default_4tasks(tmp_path):
    out = str(tmp_path) + '/'
    cmd = [sys.executable, os.path.join(PKG, 'train_ddp.py'), '--degradation_embedding_method', 'all_3_bands', '--contrast_loss_weight', '0.6',
           '--compute_dtype', 'bf16', '--per_gpu_batch', '2', '--synthetic_steps', '2', '--output_path', out, '--epochs', '1',
           '--epochs_encoder', '0', '--no_eval', '--synthesize_tasks', 'deraining', 'dehazing', 'deblurring']
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = open(out + 'train.log').read().splitlines()[0]
    m = re.fullmatch(r'Epoch \(0\)  Loss: l1_loss:(\d+\.\d{4}) contrast_loss:(\d+\.\d{4})', line)
    assert m and 0 < float(m.group(1)) < 1 and np.isfinite(float(m.group(2))), line
    opts = open(out + 'options.log').read()
    assert "['denoising_0', 'deraining', 'dehazing', 'deblurring']" in opts
