#!/usr/bin/env python3
"""Test a checkpoint on the image folders of a data tree, or restore arbitrary images -- the reference's test.py (its name is not
reused: a `test.py` on sys.path shadows the standard library's `test` package).

    python restore.py --epochs 1000 --output_path output/run/ --test_de_type denoising_bsd68_25 deraining [--data_root data/]
                      [--ckpt FILE] [--save_imgs True]
    python restore.py --ckpt FILE --input PATH --output DIR          (PATH: an image or a directory of images; no ground truth, no metrics)
                      [--keep_size] [--tile_overlap N] [--self_ensemble]
    either of them with [--band_report N] [--band_images N]

`--tile_overlap N` lets neighbouring tiles share N pixels (at most half a tile) and blends them with a linear ramp, so that the tile grid
does not show; `--self_ensemble` averages the 8 flips / rotations of every tile; both also apply to the test sets, whose PSNR / SSIM
then are those of the blended / ensembled images.  `--input` takes images of any size (one smaller than the tile is reflect-padded);
`--keep_size` restores them at their own size instead of the datasets' centre crop to multiples of 16.

Loads `<output_path>ckpt/epoch_<epochs>.pth` (train.py:126) unless `--ckpt` names a file, restores every test set of `--test_de_type`
through fwair.evaluate.EvalEngine (tiles of `--crop_test_imgs_size`, test.py:47-71 averaging the RESTORED tiles; Gaussian noise of
the denoising sets from seed 0, test.py:88) and writes `<output_path>epoch_<epochs>_results.log` in the line format of test.py:96-100.
`--band_report N` (N bands; 0, the default, turns it off) says WHERE in the spectrum the restoration errs (fwair/spectrum.py).  With test
sets it writes `<output_path>epoch_<epochs>_bands.log`: per task one line per band -- the band's radius range as a fraction of the
spectrum's corner radius, the mean over the images of the band's share E_b / sum_b E_b of the squared error, and PSNR_b =
10 log10(3 H W / E_b) averaged over the images as the set's PSNR is -- and a closing line with 10 log10(3 H W / sum_b E_b), which by
Parseval is the set's PSNR.  With `--input` (no ground truth) it writes `<output>/bands.log`: the normalised ring distribution of the
reference's get_frequency_distribution (grey image, rings of width 1 / N of half the image width) of every input and of its restoration.
The results log and the PNGs do not depend on the flag.
`--band_images N` (0, the default, turns it off) writes the N frequency bands of every restored image next to its PNG, as
`<name>_band<k>.png`, k = 0 .. N - 1: fwair.spectrum.band_images of the clamped f32 restoration, per colour channel, at the image's own
size (8 to 1024 pixels a side), the bands being those of --band_report.  Band 0 holds DC and is written as clamp(b, 0, 1); the bands k >= 1
are zero-mean and are written as clamp(0.5 + b, 0, 1); band0 + sum_k (band_k - 0.5) is the restoration again.  With `--input` the bands
of the input are written too, as `<name>_input_band<k>.png`; with test sets the flag needs `--save_imgs True`.  Everything else
written is the same with and without the flag.
`--save_imgs True` also writes `<output_path>epoch_<E>_imgs/test_<task>/<name>.png` (test.py:20-26,77-78).  The model flags
(`--degradation_embedding_method`, `--compute_dtype`, ...) must be those the checkpoint was trained with; the training batch size,
`--learnable_modulator` and `--embed_dim` are read off the checkpoint itself (net.model.options_from_checkpoint).
"""
import argparse
import os
import sys

_own = argparse.ArgumentParser(add_help=False)
_own.add_argument('--data_root', type=str, default='data/', help='directory of the <task>_test folders (fwair/data.py)')
_own.add_argument('--ckpt', type=str, default='', help='checkpoint file (default: <output_path>ckpt/epoch_<epochs>.pth)')
_own.add_argument('--input', type=str, default='', help='an image, or a directory of images, to restore without ground truth')
_own.add_argument('--output', type=str, default='', help='where --input images are written')
_own.add_argument('--tile_batch', type=int, default=64, help='tiles per forward pass')
_own.add_argument('--no_graph', action='store_true', help='eager launches instead of HIP-graph replay')
_own.add_argument('--tile_overlap', type=int, default=0, help='pixels neighbouring tiles share (at most half a tile), blended with a ramp')
_own.add_argument('--self_ensemble', action='store_true', help='average the 8 flips / rotations of every tile (8 times the work)')
_own.add_argument('--keep_size', action='store_true', help='--input: restore the image at its own size, not cropped to multiples of 16')
_own.add_argument('--band_report', type=int, default=0, help='number of spectral bands of the per-band report (0: no report)')
_own.add_argument('--band_images', type=int, default=0, help='number of spectral bands written as <name>_band<k>.png (0: none)')
_ARGS, _rest = _own.parse_known_args()
if _ARGS.band_images < 0 or _ARGS.band_images > 32:
    _own.error('--band_images takes 0 (off) to 32 bands')
sys.argv = [sys.argv[0]] + _rest                       # option.py parses sys.argv at import (reference option.py:3)

import torch                                            # noqa: E402

from fwair.data import FolderTestSet, load_u8          # noqa: E402
from fwair.evaluate import EvalEngine                   # noqa: E402
from net.model import AirNet, options_from_checkpoint   # noqa: E402
from option import options as opt                       # noqa: E402

if _ARGS.band_images and not _ARGS.input and not opt.save_imgs:
    _own.error('--band_images with test sets needs --save_imgs True: the bands are written next to the restored PNGs')

_ENGINE = {}


def _engine(net, pad_small=False):
    if _ENGINE.get('net') is not net or _ENGINE.get('pad_small') != pad_small:
        _ENGINE.update(net=net, pad_small=pad_small,
                       engine=EvalEngine(net, tile=opt.crop_test_imgs_size, tile_batch=_ARGS.tile_batch, use_graph=not _ARGS.no_graph,
                                         overlap=_ARGS.tile_overlap, ensemble=_ARGS.self_ensemble, pad_small=pad_small))
    return _ENGINE['engine']


def save_u8(img, path):
    """utils/image_io.py:375-391 on the uint8 image fw_eval_blend wrote: [3, H, W] -> PNG."""
    from PIL import Image
    Image.fromarray(img.cpu().numpy().transpose(1, 2, 0)).save(path)


def save_bands(img, stem, nbands):
    """--band_images: img [3, H, W], f32 in [0, 1] or u8 -> <stem>_band<k>.png (see the module docstring)"""
    from fwair import spectrum
    x = img.float() / 255.0 if img.dtype == torch.uint8 else img.float().clamp(0, 1)
    b = spectrum.band_images(x.contiguous(), nbands)                                    # [nbands, 3, H, W]
    b[1:] += 0.5
    u8 = (b.clamp(0, 1) * 255.0).round().to(torch.uint8)
    for k in range(nbands):
        save_u8(u8[k], '%s_band%d.png' % (stem, k))


def band_lines(task, clean, restored, nbands):
    """--band_report: the lines of one test set (see the module docstring)"""
    from fwair import spectrum
    E = spectrum.band_report(clean, restored, nbands)                                   # [I][nbands], double
    npix = torch.tensor([float(im.numel()) for im in clean], dtype=torch.float64, device=E.device)
    share = (E / E.sum(1, keepdim=True)).mean(0).tolist()
    psnr_b = (10.0 * torch.log10(npix[:, None] / E)).mean(0).tolist()
    psnr = float((10.0 * torch.log10(npix / E.sum(1))).mean())
    head = task + ': ' + ' ' * (25 - len(task))
    lines = []
    for b in range(nbands):
        lo, hi = b / nbands, (b + 1) / nbands
        lines.append(head + 'band %d [%.4f, %.4f%s error share: %.4f PSNR: %.2f' % (b, lo, hi, ']' if b == nbands - 1 else ')', share[b], psnr_b[b]))
    lines.append(head + 'all %d bands PSNR: %.2f' % (nbands, psnr))
    return lines


def distribution_lines(names, imgs, restored, nrings):
    """--band_report with --input: get_frequency_distribution (normalised, grey, size = 1 / nrings) of every image and its restoration"""
    from fwair import spectrum
    lines = []
    for name, a, b in zip(names, imgs, restored):
        for tag, im in (('input', a), ('restored', b)):
            d = spectrum.frequency_distribution(spectrum.rgb2gray(im.permute(1, 2, 0)), size=1.0 / nrings, norm=True)[0].tolist()
            lines.append('%s %s: ' % (name, tag) + ' '.join('%.6f' % v for v in d))
    return lines


def test_by_task(net, task, epochs, bands=None):
    """test.py:17-84 -> 'PSNR/SSIM: %.2f/%.4f' (means over the images of the set, AverageMeter with N = 1 per image).
    bands: a list the --band_report lines of this set are appended to."""
    print('starting testing %s...' % (task))
    dev = next(net.parameters()).device
    ts = FolderTestSet(_ARGS.data_root, task)
    clean, degraded = ts.load(dev)
    for im in clean:
        H, W = im.shape[1:]
        assert H >= opt.crop_test_imgs_size and W >= opt.crop_test_imgs_size, "invalid test image size (%d, %d)" % (H, W)     # test.py:43
    want_f32 = bands is not None or bool(_ARGS.band_images)
    out = _engine(net).run(clean, degraded, sigma=ts.sigma, seed=0, want_u8=bool(opt.save_imgs), want_f32=want_f32)
    if bands is not None:
        bands.extend(band_lines(task, clean, out[-1], _ARGS.band_report))
    if opt.save_imgs:
        output_path = opt.output_path + 'epoch_%s_imgs/' % str(epochs) + 'test_' + task + '/'
        os.makedirs(output_path, exist_ok=True)
        for name, img in zip(ts.names, out[2]):
            save_u8(img, output_path + name + '.png')
        if _ARGS.band_images:
            for name, img in zip(ts.names, out[-1]):
                save_bands(img, output_path + name, _ARGS.band_images)
    result = 'PSNR/SSIM: %.2f/%.4f' % (float(out[0].mean()), float(out[1].mean()))
    print(result)
    return result


def restore_files(net, src, dst):
    """--input / --output: every image of `src` (cropped to multiples of 16 as the datasets do, unless --keep_size), restored, written
    as <name>.png.  Any size goes: an image smaller than the tile is reflect-padded to one tile and cut back."""
    paths = sorted(os.path.join(src, f) for f in os.listdir(src)) if os.path.isdir(src) else [src]
    dev = next(net.parameters()).device
    imgs = [torch.from_numpy(load_u8(p, crop=not _ARGS.keep_size)).to(dev) for p in paths]
    os.makedirs(dst, exist_ok=True)
    res = _engine(net, pad_small=True).run(None, imgs, want_u8=True, want_f32=bool(_ARGS.band_images))
    out = res[2]
    for p, img in zip(paths, out):
        save_u8(img, os.path.join(dst, os.path.basename(p).split('.')[0] + '.png'))
    if _ARGS.band_images:
        for p, img, f32 in zip(paths, imgs, res[3]):
            stem = os.path.join(dst, os.path.basename(p).split('.')[0])
            save_bands(f32, stem, _ARGS.band_images)
            save_bands(img, stem + '_input', _ARGS.band_images)
    if _ARGS.band_report:
        with open(os.path.join(dst, 'bands.log'), 'w') as f:
            for line in distribution_lines([os.path.basename(p) for p in paths], imgs, out, _ARGS.band_report):
                f.write(line + '\n')
    return len(paths)


def main():
    torch.cuda.set_device(opt.cuda)
    dev = torch.device('cuda', opt.cuda)
    path = _ARGS.ckpt or opt.ckpt_path + 'epoch_%s.pth' % str(opt.epochs)
    sd = torch.load(path, map_location=dev, weights_only=True)
    options_from_checkpoint(opt, sd)                          # batch_size from the MoCo queue, learnable_modulator from the tables, embed_dim from the input projection
    net = AirNet(opt).to(dev)
    net.load_state_dict(sd)
    net.eval()
    if _ARGS.input:
        assert _ARGS.output, '--input needs --output DIR'
        n = restore_files(net, _ARGS.input, _ARGS.output)
        print('restored %d images into %s' % (n, _ARGS.output))
        return
    os.makedirs(opt.output_path, exist_ok=True)
    bands = [] if _ARGS.band_report else None
    with open(os.path.join(opt.output_path, 'epoch_%s_results.log' % str(opt.epochs)), 'w') as result_log_file:
        for task in opt.test_de_type:
            result = test_by_task(net, task=task, epochs=opt.epochs, bands=bands)
            result_log_file.write(task + ': ' + ' ' * (25 - len(task)) + result + '\n')
    if bands is not None:
        with open(os.path.join(opt.output_path, 'epoch_%s_bands.log' % str(opt.epochs)), 'w') as f:
            for line in bands:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
