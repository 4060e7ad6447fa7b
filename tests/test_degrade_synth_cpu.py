"""Rain, haze and motion blur of fw_train_batch_synth without a GPU: properties of the two tables (fwair/augment.py) and of the numpy
restatement the GPU tests compare against (tests/degrade_cases.py), FolderTrainSet(synthesize=...) on a folder tree that has clean
images only, and the driver's --synthesize_tasks flag."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

import data_oracle as D
import degrade_cases as DC
from fwair import augment as A
from fwair import data as FD


def test_ray_table():
    R = A.RAY
    assert R.shape == (32, 32, 2) and R.dtype == np.int8
    assert not R[:, 0].any()                                                    # step 0 stays
    t = np.arange(32)
    assert np.array_equal(R[0, :, 0], 0 * t) and np.array_equal(R[0, :, 1], t)      # a = 0: along x
    assert np.array_equal(R[16, :, 0], t) and np.array_equal(R[16, :, 1], 0 * t)    # a = 16: down y
    assert (R[:, :, 0] >= 0).all()                                              # angles 0 .. pi: never upwards
    f = np.stack([t[None] * np.sin(np.pi * np.arange(32) / 32)[:, None], t[None] * np.cos(np.pi * np.arange(32) / 32)[:, None]], -1)
    assert np.abs(R - f).max() <= 0.5 + 1e-9
    assert np.abs(np.diff(R.astype(int), axis=1)).max() <= 1                    # a connected line: the next step is a neighbour


def test_tap_set_is_point_symmetric():
    for a in range(32):
        for n in (1, 3, 7, 25):
            taps = []
            for t in range(n):
                s = t - (n - 1) // 2
                taps.append(tuple(int(np.sign(s)) * int(v) for v in A.RAY[a][abs(s)]))
            assert sorted(taps) == sorted((-y, -x) for y, x in taps) and taps[(n - 1) // 2] == (0, 0)


def test_haze_table():
    T = A.HAZE_T.astype(np.int64)
    assert T.shape == (16, 256) and A.HAZE_T.dtype == np.uint16
    assert (np.diff(T, axis=1) >= 0).all() and (T[:, -1] > T[:, 0]).all()       # clearer towards the bottom row
    assert (np.diff(T, axis=0) <= 0).all() and (T[-1] < T[0]).all()             # thicker with beta
    assert T[0, 255] == round(65535 * np.exp(-0.6 * 0.1)) and T[15, 0] == round(65535 * np.exp(-1.8))
    assert A.HAZE_BETAS[0] == 0.6 and abs(A.HAZE_BETAS[-1] - 1.8) < 1e-12


def test_blur_restatement():
    img = DC.images(1, [(21, 34)])[0]
    for a in range(32):
        for n in range(1, 26, 2):
            const = np.full((3, 9, 13), 10 * a % 256, np.uint8)
            assert np.array_equal(DC.blur(const, a, n), const), (a, n)
        assert np.array_equal(DC.blur(img, a, 1), img)
    # a = 0, n = 3 is the horizontal 3-tap mean with the border pixel repeated, rounded to nearest
    p = np.pad(img.astype(np.int64), ((0, 0), (0, 0), (1, 1)), mode='edge')
    assert np.array_equal(DC.blur(img, 0, 3), (2 * (p[:, :, :-2] + p[:, :, 1:-1] + p[:, :, 2:]) + 3) // 6)


def test_rain_restatement():
    img = DC.images(2, [(40, 56)])[0]
    key = DC.site_key(77, 0x7A000100)
    for a, L in ((5, 1), (8, 32), (11, 5)):
        m, seeds = DC.rain_layer(40, 56, a, L, 4096, key)
        out = DC.rain(img, a, L, 4096, 255, key)
        assert (out >= img).all()                                               # rain never darkens
        assert np.array_equal(out[:, m == 0], img[:, m == 0]) and (m == 0).any()          # no seed on the back-ray: untouched
        assert (m[seeds] > 0).all() and 40 * 56 // 32 < seeds.sum() < 40 * 56 // 8        # about 1 / 16 of the pixels seed a streak
        assert np.array_equal(DC.rain(img, a, L, 4096, 0, key), img)            # strength 0
        assert np.array_equal(DC.rain(img, a, L, 0, 255, key), img)             # no seeds
    assert not np.array_equal(DC.rain_layer(40, 56, 8, 32, 4096, key)[0], DC.rain_layer(40, 56, 8, 32, 4096, DC.site_key(77, 0x7A000101))[0])
    m, seeds = DC.rain_layer(40, 56, 0, 4, 4096, key)                           # a = 0: a streak runs to the right of its seed and fades
    y, x = [int(v[0]) for v in np.nonzero(seeds[:, :50])]
    h = int(DC.pixel_hash(40, 56, key)[y, x])
    amp = 128 + ((h >> 16) & 127)
    assert all(m[y, x + t] >= amp * (4 - t) for t in range(4))

def test_haze_restatement():
    for j in (0, 7, 15):
        for a8 in (0, 204, 255):
            const = np.full((3, 17, 5), a8, np.uint8)
            assert np.array_equal(DC.haze(const, j, a8), const)                 # the airlight's own value stays
    img = DC.images(3, [(33, 20)])[0]
    out = DC.haze(img, 15, 204).astype(int)
    assert (np.abs(out - 204) <= np.abs(img.astype(int) - 204)).all()           # every pixel moves towards the airlight
    assert np.abs(out[:, 0] - 204).mean() < np.abs(out[:, -1] - 204).mean()     # most at the top (far)
    ref = img / 255.0 * np.exp(-1.8 * np.linspace(1, 0.1, 33))[None, :, None]
    ref = (ref + 0.8 * (1 - np.exp(-1.8 * np.linspace(1, 0.1, 33)))[None, :, None]) * 255
    assert np.abs(out - ref).max() < 2.5                                        # add_haze's model up to the 8-bit depth ramp


def test_mode_map_is_the_reference_augmentation():
    S = 6
    crop = np.arange(3 * S * S, dtype=np.uint8).reshape(3, S, S)
    for mode in range(1, 8):
        py, px = DC.mode_preimage(mode, S)
        ref = D.data_augmentation(crop.transpose(1, 2, 0), mode).transpose(2, 0, 1)
        assert np.array_equal(crop[:, py, px], ref), mode


def test_records_and_defaults():
    assert A.synth_record('deraining', 5, 16) == [1, 5, 16, 164, 179, 0, 0, 0]
    assert A.synth_record('dehazing', 15) == [2, 15, 204, 0, 0, 0, 0, 0]
    assert A.synth_record('deblurring', 31, 25) == [3, 31, 25, 0, 0, 0, 0, 0]
    assert A.rain_length(128) == 16 and A.rain_length(16) == 4 and A.rain_length(512) == 32
    with pytest.raises(AssertionError):
        A.synth_record('deblurring', 0, 8)                                      # an even tap count


def _png(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def test_folder_train_set_synthesize(tmp_path):
    rs = np.random.RandomState(0)
    for k in range(3):
        _png(str(tmp_path / f'denoising_train/GT/im{k}.png'), rs.randint(0, 256, (48, 64, 3)).astype(np.uint8))
    root = str(tmp_path)
    de_type = ['denoising_0', 'deraining', 'dehazing', 'deblurring']
    ts = FD.FolderTrainSet(root, de_type, 32, 'cpu', synthesize=('deraining', 'dehazing', 'deblurring'))
    assert ts.counts == [3, 3, 3, 3] and ts.synthesize == de_type[1:]
    bt = ts.batcher
    assert bt.synth and bt.code == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert all(d is None for d in bt.degraded)
    assert bt.random_sigma == [True] * 3 + [False] * 9
    for t in range(1, 4):                                                       # every synthesised task holds the denoising set's tensors
        assert [bt.images[ts.base[t] + k].data_ptr() for k in range(3)] == [bt.images[k].data_ptr() for k in range(3)]
    assert ts.names[3] == ('im0', 'deraining')
    # a task's own GT folder wins over the denoising set's
    _png(str(tmp_path / 'dehazing_train/GT/own.png'), rs.randint(0, 256, (32, 32, 3)).astype(np.uint8))
    ts = FD.FolderTrainSet(root, de_type, 32, 'cpu', synthesize=('deraining', 'dehazing', 'deblurring'))
    assert ts.counts == [3, 3, 1, 3] and ts.names[ts.base[2]] == ('own', 'dehazing')
    # an unlisted paired task behaves as before
    with pytest.raises(FileNotFoundError):
        FD.FolderTrainSet(root, de_type, 32, 'cpu', synthesize=('deraining', 'dehazing'))
    with pytest.raises(FileNotFoundError):
        FD.FolderTrainSet(root, de_type, 32, 'cpu')
    with pytest.raises(ValueError):
        FD.FolderTrainSet(root, de_type, 32, 'cpu', synthesize=('denoising_0',))
    plain = FD.FolderTrainSet(root, ['denoising_25'], 32, 'cpu')
    assert not plain.batcher.synth and plain.synthesize == []


def test_driver_parses_synthesize_tasks(monkeypatch, capsys):
    def parsed(extra):
        monkeypatch.setattr(sys, 'argv', ['train_ddp.py', '--degradation_embedding_method', 'all_3_bands'] + extra)
        for name in ('train_ddp', 'option'):
            sys.modules.pop(name, None)
        try:
            import train_ddp
            return train_ddp._ARGS, list(sys.argv), list(train_ddp.opt.de_type)
        finally:
            for name in ('train_ddp', 'option'):
                sys.modules.pop(name, None)

    a, _, de = parsed([])
    assert a.synthesize_tasks == [] and de == ['denoising_0', 'deraining', 'dehazing', 'deblurring']
    a, argv, _ = parsed(['--synthetic_steps', '2', '--synthesize_tasks', 'deraining', 'dehazing', 'deblurring', '--epochs', '1'])
    assert a.synthesize_tasks == ['deraining', 'dehazing', 'deblurring'] and a.synthetic_steps == 2
    assert argv[1:] == ['--degradation_embedding_method', 'all_3_bands', '--epochs', '1']
    with pytest.raises(SystemExit):
        parsed(['--synthesize_tasks', 'denoising_25'])
    assert 'synthesize_tasks' in capsys.readouterr().err
