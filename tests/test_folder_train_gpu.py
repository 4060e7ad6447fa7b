"""Image folders end to end (fwair/data.py, train_ddp.py --data_root, restore.py) on a small tree written into tmp_path:
paired images from disk through DeviceBatcher, FolderTrainSet's first batch, a two-phase training run with the per-epoch evaluation
of the `<task>_test` folders, and restore.py on its checkpoint (same weights, same seeded noise -> the same PSNR; PNGs written)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import data_oracle as D

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd')


def _image(rs, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([127 + 90 * np.sin(xx / (7 + c) + yy / (11 + 2 * c)) + rs.randn(h, w) * 12 for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)                       # HWC


def _rain(rs, img):
    out = img.astype(np.float32)
    out[rs.rand(*img.shape[:2]) < 0.03] += 120
    return np.clip(out, 0, 255).astype(np.uint8)


def _save(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def make_tree(root):
    rs = np.random.RandomState(21)
    for k in range(4):
        _save(f'{root}/denoising_train/GT/img{k}.png', _image(rs, 160, 176))
    for k in range(3):
        g = _image(rs, 160, 176)
        _save(f'{root}/deraining_train/GT/rain-{k}.png', g)
        _save(f'{root}/deraining_train/Input/rain-{k}_{k + 1}.png', _rain(rs, g))
    for k in range(2):
        _save(f'{root}/denoising_bsd68_test/GT/test{k}.png', _image(rs, 200, 248))
        g = _image(rs, 200, 248)
        _save(f'{root}/deraining_test/GT/rain-{k}.png', g)
        _save(f'{root}/deraining_test/Input/rain-{k}_x.png', _rain(rs, g))
    return root


def test_device_batcher_paired_from_disk(tmp_path):
    from fwair import augment as A
    from fwair import data as FD
    from fwair import functional as Fn
    root = make_tree(str(tmp_path))
    gt_ids, in_ids = FD.pair_ids(root + '/deraining_train/', False)
    gt, dg = [FD.load_u8(p) for p in gt_ids], [FD.load_u8(p) for p in in_ids]
    assert gt[0].shape == (3, 160, 176) and not np.array_equal(gt[0], dg[0])
    extra = FD.load_u8(root + '/denoising_train/GT/img0.png')
    imgs = [torch.from_numpy(i).to(DEV) for i in gt + [extra]]
    degr = [torch.from_numpy(i).to(DEV) for i in dg] + [None]
    Fn.set_dropout_seed(4242, DEV, frozen=True)
    try:
        bt = A.DeviceBatcher(imgs, ['deraining'] * 3 + ['denoising_25'], 128, degraded_u8=degr)
        idx = [0, 3, 1, 2]
        out = [t.cpu().numpy() for t in bt.batch(idx, generator=torch.Generator(device=DEV).manual_seed(3))]
        allg, alld = gt + [extra], dg + [None]
        ref = D.train_batch([allg[i] for i in idx], [alld[i] for i in idx], [bt.sigma[i] for i in idx], bt.last_rnd.cpu().numpy()[:, :6],
                            4242, bt.last_site, 128)
    finally:
        Fn.set_dropout_seed(1, DEV, frozen=False)
    for s in (0, 2, 3):                                               # the paired samples: bit-exact crops of the images on disk
        for a, b in zip(out, ref):
            assert np.array_equal(a[s], b[s])
    assert np.array_equal(out[2][1], ref[2][1]) and np.abs(out[0][1] - ref[0][1]).max() * 255 <= 1.0 + 1e-4      # denoising beside them
    # default None: the synthetic stand-in, as before
    bt2 = A.DeviceBatcher(imgs[:1], ['deraining'], 128, generator=torch.Generator().manual_seed(5))
    bt3 = A.DeviceBatcher(imgs[:1], ['deraining'], 128, generator=torch.Generator().manual_seed(5), degraded_u8=None)
    assert torch.equal(bt2.degraded[0], bt3.degraded[0]) and not torch.equal(bt2.degraded[0], degr[0])


def test_folder_train_set_first_batch(tmp_path):
    from fwair import augment as A
    from fwair import data as FD
    from fwair import functional as Fn
    root = make_tree(str(tmp_path))
    de_type = ['denoising_25', 'deraining']
    Fn.set_dropout_seed(99, DEV, frozen=True)
    try:
        ds = FD.FolderTrainSet(root, de_type, 128, DEV, rank=1, world=2, per_gpu_batch=2, items_per_task=4, seed=5)
        assert ds.steps == 4 * 2 // 4 and ds.counts == [4, 3] and ds.base == [0, 4]
        assert ds.names[4] == ('rain-0', 'deraining')
        first = next(iter(ds.epoch(0)))
        # the same by hand: the schedule's first global step, rank 1's slice, the same generator
        items = FD.shard(FD.TaskSchedule(de_type, [4, 3], 5).take(4), 1, 2)
        idx = [ds.base[t] + i for t, i in items]
        assert [t for t, _ in items] == [0, 1]
        bt = A.DeviceBatcher(ds.batcher.images, ['denoising_25'] * 4 + ['deraining'] * 3, 128, degraded_u8=ds.batcher.degraded)
        ref = bt.batch(idx, generator=torch.Generator(device=DEV).manual_seed(5 + 7919))
    finally:
        Fn.set_dropout_seed(1, DEV, frozen=False)
    assert len(first) == 3
    for a, b in zip(first, (ref[0], ref[1], ref[2])):
        assert a.shape == (2, 3, 128, 128) and torch.equal(a, b)
    assert len(list(ds.epoch(1))) == 2
    with pytest.warns(UserWarning, match='skipped 7 training images'):
        with pytest.raises(ValueError):
            FD.FolderTrainSet(root, de_type, 192, DEV)
    with pytest.raises(MemoryError, match='--data_cache_gb'):
        FD.FolderTrainSet(root, de_type, 128, DEV, cache_gb=1e-4)


def _run(script, *args):
    env = dict(os.environ, PYTHONPATH=PKG)                             # only the package directory: no reference, no torchvision
    r = subprocess.run([sys.executable, os.path.join(PKG, script), *args], cwd=PKG, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_train_and_restore_on_folders(tmp_path):
    root = make_tree(str(tmp_path / 'data'))
    out = str(tmp_path / 'run') + '/'
    model = ['--degradation_embedding_method', 'all_3_bands', '--test_de_type', 'denoising_bsd68_25', 'deraining', '--output_path', out]
    _run('train_ddp.py', '--data_root', root, '--de_type', 'denoising_25', 'deraining', '--epochs', '2', '--epochs_encoder', '1',
         '--items_per_task', '4', '--per_gpu_batch', '2', *model)
    log = open(out + 'train.log').read().splitlines()
    assert len(log) == 2
    assert re.fullmatch(r'Epoch \(0\)  Loss: contrast_loss:\d+\.\d{4}', log[0])
    assert re.fullmatch(r'Epoch \(1\)  Loss: l1_loss:\d+\.\d{4} contrast_loss:\d+\.\d{4}', log[1])
    res = open(out + 'results.log').read().splitlines()
    assert res[0] == '2 Epochs Results:' and len(res) == 3
    vals = {}
    for line, task in zip(res[1:], ('denoising_bsd68_25', 'deraining')):
        m = re.fullmatch(re.escape(task) + ': ' + ' ' * (25 - len(task)) + r'PSNR/SSIM: (-?\d+\.\d{2})/(-?\d\.\d{4})', line)
        assert m, line
        vals[task] = float(m.group(1))
        assert np.isfinite(vals[task]) and np.isfinite(float(m.group(2)))
    assert os.path.exists(out + 'ckpt/epoch_2.pth')
    # restore.py on that checkpoint: same weights, same seeded noise
    _run('restore.py', '--data_root', root, '--de_type', 'denoising_25', 'deraining', '--epochs', '2', '--save_imgs', 'True', *model)
    res2 = open(out + 'epoch_2_results.log').read().splitlines()
    assert len(res2) == 2
    for line, task in zip(res2, ('denoising_bsd68_25', 'deraining')):
        m = re.fullmatch(re.escape(task) + ': ' + ' ' * (25 - len(task)) + r'PSNR/SSIM: (-?\d+\.\d{2})/(-?\d\.\d{4})', line)
        assert m, line
        print(f'{task}: results.log {vals[task]:.2f} dB, restore.py {float(m.group(1)):.2f} dB')
        assert abs(float(m.group(1)) - vals[task]) <= 0.01 + 1e-9
    for task, names in (('denoising_bsd68_25', ('test0', 'test1')), ('deraining', ('rain-0_x', 'rain-1_x'))):
        for n in names:
            png = np.array(Image.open(out + f'epoch_2_imgs/test_{task}/{n}.png'))
            assert png.shape == (192, 240, 3) and png.dtype == np.uint8           # 200 x 248 after crop_img(base=16)
    # arbitrary images without ground truth
    dst = str(tmp_path / 'restored')
    _run('restore.py', '--ckpt', out + 'ckpt/epoch_2.pth', '--input', root + '/deraining_test/Input', '--output', dst,
         '--de_type', 'denoising_25', 'deraining', *model)
    assert sorted(os.listdir(dst)) == ['rain-0_x.png', 'rain-1_x.png']
    assert np.array(Image.open(dst + '/rain-0_x.png')).shape == (192, 240, 3)
