"""Where in the spectrum a signal, or a restoration's error, sits: radial band statistics of images of any size on the device
(csrc/fw_spec.hip: fw_band_stats), and the bands themselves (fw_band_split).

  ring_index              the band of every frequency bin: the rings of the reference's get_frequency_distribution
                          (utils/visualization_utils.py:158-184, kind 'plot') or the partition of the band decomposition
                          (fwair.lfs.band_masks_shifted, kind 'bands')
  frequency_distribution  get_frequency_distribution for device tensors
  band_report             error energy per band of restored images against their ground truth; by Parseval its bands add up to the
                          squared error the evaluation engine's PSNR is computed from
  band_split              fw_band_split: band images, masked spectra or shifted magnitudes of maps [n, H, W] for any ring table
  band_images             the band images of an image or a batch, 8 <= H, W <= 1024 independent of each other
  BandSplit               the reference's FrequencyDecompose(type, size, h, w, inverse) for any such (h, w), forward only;
                          net/utils/frequency_decompose.py keeps the square sides of the model's hot path and the autograd function
"""
import math

import numpy as np
import torch
from torch import nn

from . import lfs
from .lib import call

_rings, _panels = {}, {}


def ring_edges(kind, size, h, w):
    """-> [(lo, hi)] radius range of every band in pixels of the shifted spectrum, and the radius the fractions refer to
    ('plot': int(w / 2); 'bands', 'bands_1': the corner radius; 'bands_1' has DC alone, (0, 0), as band 0, then (lo, hi] rings)."""
    if kind == 'plot':
        diag = int(w / 2)
        return [(diag * (sz - size), diag * sz) for sz in np.linspace(size, 1, int(1 / size))], diag
    if kind == 'bands':
        rmax = math.sqrt(int(w / 2) ** 2 + int(h / 2) ** 2)
        szs = [float(s) for s in torch.linspace(size, 1, math.floor(1. / size + 0.1))]
        return [(rmax * lo, rmax * hi) for lo, hi in zip([0.0] + szs[:-1], szs)], rmax
    if kind == 'bands_1':
        rmax = math.sqrt(int(w / 2) ** 2 + int(h / 2) ** 2)
        szs = [float(s) for s in torch.linspace(0, 1, math.floor(1. / size + 0.1) + 1)]
        return [(0.0, 0.0)] + [(rmax * lo, rmax * hi) for lo, hi in zip(szs[:-1], szs[1:])], rmax
    raise ValueError(kind)


def ring_index(kind, size, h, w):
    """u8 numpy [h][w] in fftshift-ed coordinates: the band of every bin, 255 = in no band.
    'plot': ring i of get_frequency_distribution, float64 arithmetic as there: diag = int(w / 2), int(1 / size) rings over
    np.linspace(size, 1, .), diag (sz - size) <= d < diag sz, the ring with sz == 1 closed.  A bin in two rings is a ValueError (the
    reference would count it twice).  'bands': the partition of lfs.band_masks_shifted('frequency_decompose', size, h, w);
    'bands_1': that of lfs.band_masks_shifted('frequency_decompose_1', size, h, w), DC alone being band 0."""
    if kind == 'plot':
        center = (int(w / 2), int(h / 2))
        Y, X = np.ogrid[:h, :w]
        dist = np.sqrt((X - center[0]) ** 2 + (Y - center[1]) ** 2)
        diag = center[0]
        n = int(1 / size)
        if not 1 <= n < 255:
            raise ValueError(f'ring_index: size {size} gives {n} rings')
        ring = np.full((h, w), 255, dtype=np.uint8)
        for idx, sz in enumerate(np.linspace(size, 1, n)):
            if sz == 1:
                m = (diag * (sz - size) <= dist) & (dist <= diag * sz)
            elif sz < 1:
                m = (diag * (sz - size) <= dist) & (dist < diag * sz)
            else:
                continue
            if (ring[m] != 255).any():
                raise ValueError(f'ring_index: a bin of the {h} x {w} spectrum falls into two rings of size {size}')
            ring[m] = idx
        return ring
    if kind in ('bands', 'bands_1'):
        masks = torch.stack(lfs.band_masks_shifted('frequency_decompose' if kind == 'bands' else 'frequency_decompose_1', size, h, w))
        if masks.shape[0] >= 255 or not bool((masks.sum(0) == 1).all()):
            raise ValueError(f'ring_index: the bands of size {size} do not partition the {h} x {w} spectrum')
        return masks.to(torch.uint8).argmax(0).to(torch.uint8).numpy()
    raise ValueError(kind)


def ring_table(kind, size, h, w, device):
    """-> (u8 [h][w] device tensor in UN-shifted coordinates, number of bands); cached per (kind, size, h, w, device)"""
    key = (kind, float(size), h, w, str(device))
    if key not in _rings:
        nb = len(ring_edges(kind, size, h, w)[0])
        ring = np.fft.ifftshift(ring_index(kind, size, h, w))
        _rings[key] = (torch.from_numpy(np.ascontiguousarray(ring)).to(device), nb)
    return _rings[key]


def padded(n):
    return (n + 63) // 64 * 64


def panels_host(n):
    """f32 numpy [3][Np][Np], Np = 64 ceil(n / 64): cos, sin, -sin of 2 pi i j / n for i, j < n, zero elsewhere"""
    i = np.arange(n, dtype=np.int64)
    ang = 2 * np.pi * ((i[:, None] * i[None, :]) % n).astype(np.float64) / n
    p = np.zeros((3, padded(n), padded(n)), dtype=np.float32)
    p[0, :n, :n], p[1, :n, :n], p[2, :n, :n] = np.cos(ang), np.sin(ang), -np.sin(ang)
    return p


def panels(n, device):
    key = (n, str(device))
    if key not in _panels:
        _panels[key] = torch.from_numpy(panels_host(n)).to(device)
    return _panels[key]


def work_floats(nimg, h, w, nbands):
    """the work buffer of fw_band_stats (include/fwair.h)"""
    wh = padded(w // 2 + 1)                     # the columns v <= w / 2 of the spectrum of a real map
    return nimg * (2 * padded(h) * wh + (padded(h) // 64) * (wh // 64) * nbands)


def _source(name, src, clean):
    """the source of fw_band_stats / fw_band_split checked -> (source kind, src, clean), both contiguous"""
    kind = 2 if clean is not None else (1 if src.dtype == torch.uint8 else 0)
    if kind != 1 and src.dtype != torch.float32:
        raise TypeError(f'{name}: {src.dtype} maps (float32 or uint8)')
    if clean is not None and (clean.dtype != torch.uint8 or clean.shape != src.shape):
        raise TypeError(f'{name}: clean must be uint8 of the shape of the restored maps')
    return kind, src.contiguous(), clean.contiguous() if clean is not None else None


def band_stats(src, ring, nbands, power, clean=None):
    """fw_band_stats on src [n, H, W] (f32 or u8, contiguous; with `clean` u8 [n, H, W]: the error map of restored f32 `src`).
    -> double [n, nbands]"""
    n, h, w = src.shape
    kind, src, clean = _source('band_stats', src, clean)
    out = torch.empty((n, nbands), dtype=torch.float64, device=src.device)
    work = torch.empty(work_floats(n, h, w, nbands), dtype=torch.float32, device=src.device)
    call('fw_band_stats', kind, src, clean, ring, panels(h, src.device), panels(w, src.device), work, out, n, h, w, nbands, power)
    return out


def split_work_floats(nimg, h, w, nbands, mode):
    """the work buffer of fw_band_split (include/fwair.h)"""
    return nimg * padded(h) * padded(w // 2 + 1) * (4 + (2 * min(nbands, 4) if mode == 0 else 0))


def band_split(src, ring, nbands, mode, clean=None):
    """fw_band_split on src [n, H, W] (f32 or u8, contiguous; with `clean` u8 [n, H, W]: the error map of restored f32 `src`); ring: u8
    [H, W] device table in UN-shifted coordinates.  mode 0 -> band images f32 [nbands, n, H, W]; 1 -> (re, im) of the masked spectra
    [nbands, n, H, W, 2]; 2 -> their magnitudes in fftshift-ed coordinates [nbands, n, H, W]"""
    if src.dim() != 3:
        raise ValueError(f'band_split: maps [n, H, W], not {tuple(src.shape)}')
    n, h, w = src.shape
    kind, src, clean = _source('band_split', src, clean)
    if ring.dtype != torch.uint8 or tuple(ring.shape) != (h, w):
        raise TypeError(f'band_split: the ring must be uint8 [{h}, {w}]')
    if mode not in (0, 1, 2):
        raise ValueError(f'band_split: mode {mode} (0 band images, 1 masked spectra, 2 magnitudes)')
    out = torch.empty((nbands, n, h, w, 2) if mode == 1 else (nbands, n, h, w), dtype=torch.float32, device=src.device)
    work = torch.empty(split_work_floats(n, h, w, nbands, mode), dtype=torch.float32, device=src.device)
    call('fw_band_split', kind, src, clean, ring.contiguous(), panels(h, src.device), panels(w, src.device), work, out, n, h, w, nbands, mode)
    return out


def band_images(img, nbands, kind='bands', clean=None):
    """The band images of img [H, W], [n, H, W] or [B, C, H, W] (f32 or u8; 8 <= H, W <= 1024, any values): Re IDFT2 of the spectrum
    restricted to each band of ring_index(kind, 1 / nbands) -> f32 [nb, ...the leading axes of img..., H, W] with nb = nbands ('bands')
    or nbands + 1 ('bands_1', DC first); the bands sum to the image.  With `clean` (u8, the shape of img): the bands of the error map
    clamp(img, 0, 1) - clean / 255.  One size per call."""
    if img.dim() not in (2, 3, 4):
        raise ValueError(f'band_images: a map [H, W], a batch [n, H, W] or [B, C, H, W], not {tuple(img.shape)}')
    if clean is not None and clean.shape != img.shape:
        raise TypeError('band_images: clean must have the shape of img')
    h, w = img.shape[-2:]
    ring, nb = ring_table(kind, 1.0 / nbands, h, w, img.device)
    out = band_split(img.reshape(-1, h, w), ring, nb, 0, clean=None if clean is None else clean.reshape(-1, h, w))
    return out.reshape((nb,) + tuple(img.shape))


class BandSplit(nn.Module):
    """FrequencyDecompose(type, size, h, w, inverse) of the reference (net/utils/frequency_decompose.py:5-125) for ANY 8 <= h, w <= 1024:
        'frequency_decompose'    bands [0, s) ... [1 - s, 1]       -> [nb,     B, C, h, w]
        'frequency_decompose_1'  DC, (0, s] ... (1 - s, 1]         -> [nb + 1, B, C, h, w]
        'frequency_decompose_dc' mean / residual                   -> [2,      B, C, h, w]
    inverse=False -> [..., 2] (re, im) of the masked un-shifted spectrum; inverse='visual' -> magnitudes, fftshift-ed over ALL axes as
    the reference's dim-less fftshift does (batch and channels rolled by B // 2, C // 2).  Forward only: the training path keeps
    net.utils.frequency_decompose.FrequencyDecompose and its autograd function."""

    def __init__(self, type, size, h, w, inverse=True):
        super().__init__()
        self.type, self.size, self.h, self.w, self.inverse = type, size, h, w, inverse
        assert size > 0 and size <= 1, 'invalid frequency band width(size=%s)' % (size)
        if type not in ('frequency_decompose', 'frequency_decompose_1', 'frequency_decompose_dc'):
            raise ValueError(type)
        if inverse not in (True, False, 'visual'):
            raise ValueError(f'BandSplit: inverse={inverse!r}')
        if not (8 <= h <= 1024 and 8 <= w <= 1024):
            raise NotImplementedError('BandSplit handles maps of 8..1024 by 8..1024 pixels, not %sx%s' % (h, w))
        if type != 'frequency_decompose_dc':
            self.num_bands = math.floor(1. / self.size + 0.1)

    def forward(self, x):
        if x.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError('BandSplit is forward only; FrequencyDecompose (net/utils/frequency_decompose.py) is differentiable')
        B, C, h, w = x.shape
        xc = x.detach().contiguous().float()
        if self.type == 'frequency_decompose_dc':
            out = torch.empty((2, B, C, h, w), dtype=torch.float32, device=x.device)
            call('fw_dc_split', xc, out, B * C, h * w)
            return out
        assert h == self.h and w == self.w
        ring, nb = ring_table('bands' if self.type == 'frequency_decompose' else 'bands_1', self.size, h, w, x.device)
        mode = 0 if self.inverse is True else 1 if self.inverse is False else 2
        out = band_split(xc.reshape(B * C, h, w), ring, nb, mode)
        out = out.reshape((nb, B, C, h, w, 2) if mode == 1 else (nb, B, C, h, w))
        if mode == 2:
            out = torch.roll(out, shifts=(B // 2, C // 2), dims=(1, 2))
        return out


def rgb2gray(img_hwc):
    """utils/visualization_utils.py:148-155 for a tensor [H, W, C]"""
    if img_hwc.shape[2] == 1:
        return img_hwc[:, :, 0]
    img = img_hwc.to(torch.float32)
    gray = 0.2989 * img[:, :, 0] + 0.5870 * img[:, :, 1] + 0.1140 * img[:, :, 2]
    return gray.clamp(0, 255)


def frequency_distribution(img, size=0.2, norm=True):
    """get_frequency_distribution (utils/visualization_utils.py:158-184) of a device tensor [H, W] or a batch [n, H, W], f32 or u8:
    the sum of |DFT2| over each of the int(1 / size) rings -> double [n, int(1 / size)], each row divided by its sum if `norm`."""
    x = img if img.dim() == 3 else img.unsqueeze(0)
    if x.dim() != 3:
        raise ValueError(f'frequency_distribution: a map [H, W] or a batch [n, H, W], not {tuple(img.shape)}')
    ring, nb = ring_table('plot', size, x.shape[1], x.shape[2], x.device)
    out = band_stats(x, ring, nb, 0)
    return out / out.sum(1, keepdim=True) if norm else out


def band_report(clean_u8, restored_f32, nbands):
    """clean_u8, restored_f32: lists of [3, H, W] device tensors (uint8 / float32), sizes may differ from image to image.
    -> double [I][nbands], E_b = sum_c sum_{f in b} |F_c(e)|^2 / (H W) with e = clamp(restored, 0, 1) - clean / 255 and the bands of
    ring_index('bands', 1 / nbands): sum_b E_b = sum e^2, the squared error of the engine's PSNR.  Images of one size share a launch."""
    I = len(clean_u8)
    assert I == len(restored_f32) and I > 0
    dev = restored_f32[0].device
    E = torch.empty((I, nbands), dtype=torch.float64, device=dev)
    groups = {}
    for i, t in enumerate(restored_f32):
        groups.setdefault(tuple(t.shape[1:]), []).append(i)
    for (h, w), idx in groups.items():
        ring, nb = ring_table('bands', 1.0 / nbands, h, w, dev)
        assert nb == nbands
        r = torch.cat([restored_f32[i].reshape(-1, h, w) for i in idx])
        c = torch.cat([clean_u8[i].reshape(-1, h, w) for i in idx])
        ch = r.shape[0] // len(idx)
        s = band_stats(r, ring, nbands, 1, clean=c).view(len(idx), ch, nbands).sum(1) / (h * w)
        E[torch.tensor(idx, device=dev)] = s
    return E
