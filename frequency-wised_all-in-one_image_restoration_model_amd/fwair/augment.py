"""Input pipeline on the device: the per-sample work of utils/dataset_utils.py:122-135 -- Gaussian noise
synthesis on the uint8 grid, two independent random crops of the same degraded image, one of the 7 flip / rotation modes of
utils/image_utils.py:133-160 per crop -- as batched tensor ops, so that it runs on the GPU next to the model instead of in
DataLoader workers.  Images are channels-first ([..., C, H, W]); the reference's numpy code is HWC (flipud = flip H,
rot90 = counter-clockwise in the H-W plane), which maps to dims (-2, -1) here."""
import math

import numpy as np
import torch

from .lib import call


def augment(x, mode):
    """utils/image_utils.py:133-160 `data_augmentation(image, mode)` for channels-first tensors."""
    if mode == 0:
        return x
    k, flip = mode // 2, mode % 2 == 1          # 1: flipud | 2: rot90 | 3: rot90 + flipud | 4: rot180 | 5: +flipud | 6: rot270 | 7: +flipud
    out = torch.rot90(x, k, dims=(-2, -1)) if k else x
    return out.flip(-2) if flip else out


def add_noise(clean_u8, sigma, generator=None):
    """dataset_utils.py:126: clip(gt + randn * sigma, 0, 255).astype(uint8).  clean_u8: uint8 or float tensor on the 0..255 grid."""
    g = clean_u8.float()
    if generator is not None and generator.device != g.device:      # a host generator driving device data: draw there, move
        n = torch.randn(g.shape, device=generator.device, generator=generator).to(g.device)
    else:
        n = torch.randn(g.shape, device=g.device, generator=generator)
    return (g + n * float(sigma)).clamp_(0, 255).to(torch.uint8)          # float -> uint8 truncates, like numpy's astype


def add_rain(clean_u8, generator=None, streaks=None, length=None, angle_deg=None, strength=0.7):
    """Synthetic stand-in for the rain pairs the reference only loads from disk (dataset_utils.py:93-95,129):
    additive bright line streaks at 45 +- 15 degrees, drawn as `length` shifted copies of a sparse seed map.  uint8 in / out."""
    g = clean_u8.float()
    H, W = g.shape[-2:]
    dev = g.device
    rnd = lambda *shape: torch.rand(shape, generator=generator, device='cpu')
    ang = float(angle_deg) if angle_deg is not None else 30.0 + 30.0 * float(rnd(1))
    n = int(streaks) if streaks is not None else max(1, H * W // 400)
    L = int(length) if length is not None else max(4, H // 8)
    ys = (rnd(n) * H).long().clamp_(max=H - 1)
    xs = (rnd(n) * W).long().clamp_(max=W - 1)
    seed = torch.zeros((H, W), dtype=torch.float32)
    seed[ys, xs] = 0.5 + 0.5 * rnd(n)
    seed = seed.to(dev)
    dy, dx = math.sin(math.radians(ang)), math.cos(math.radians(ang))
    layer = torch.zeros((H, W), dtype=torch.float32, device=dev)
    for t in range(L):                                     # a streak = the seed pixel smeared along (dy, dx), fading towards its tail
        layer = torch.maximum(layer, torch.roll(seed, shifts=(int(round(t * dy)), int(round(t * dx))), dims=(0, 1)) * (1.0 - t / L))
    return (g + 255.0 * strength * layer).clamp_(0, 255).to(torch.uint8)


def add_haze(clean_u8, generator=None, beta=None, airlight=0.8):
    """Synthetic stand-in for the haze pairs: I = J t + A (1 - t), t = exp(-beta * depth), depth = a vertical ramp
    (far at the top of the frame), A = 0.8.  uint8 in / out."""
    g = clean_u8.float() / 255.0
    H = g.shape[-2]
    b = float(beta) if beta is not None else 0.6 + 1.2 * float(torch.rand((1,), generator=generator, device='cpu'))
    depth = torch.linspace(1.0, 0.1, H, device=g.device).view(H, 1)
    t = torch.exp(-b * depth)
    return ((g * t + airlight * (1.0 - t)) * 255.0).clamp_(0, 255).to(torch.uint8)


def degrade(clean_u8, task, generator=None):
    """The degraded image of one `--de_type` entry.  denoising_<sigma> as dataset_utils.py:123-126 (sigma 0 = a random choice of
    15 / 25 / 50); deraining / dehazing: the synthetic stand-ins above (the reference reads those pairs from disk)."""
    if task.startswith('denoising'):
        sigma = int(task.split('_')[-1])
        if sigma == 0:
            sigma = (15, 25, 50)[int(torch.randint(0, 3, (1,), generator=generator, device='cpu'))]
        return add_noise(clean_u8, sigma, generator)
    if task == 'deraining':
        return add_rain(clean_u8, generator)
    if task == 'dehazing':
        return add_haze(clean_u8, generator)
    raise ValueError(f'unknown de_type {task!r}')


def crop_pair(degraded, clean, size, generator=None):
    """dataset_utils.py `_crop_patch`: one random window, the same for the degraded and the clean image ([C, H, W] each)."""
    H, W = clean.shape[-2:]
    y = int(torch.randint(0, H - size + 1, (1,), generator=generator, device='cpu'))
    x = int(torch.randint(0, W - size + 1, (1,), generator=generator, device='cpu'))
    return degraded[..., y:y + size, x:x + size], clean[..., y:y + size, x:x + size]


def training_pair(clean_u8, size, sigma=None, degraded_u8=None, generator=None):
    """One dataset item (dataset_utils.py:122-135) from a clean uint8 image [3, H, W] on the device:
    -> (degrad_patch_1, degrad_patch_2, clean_patch_1, clean_patch_2), f32 in [0, 1] as ToTensor would give.
    Denoising: the degraded image is synthesised once (sigma), then cropped twice; other tasks pass `degraded_u8`."""
    if degraded_u8 is None:
        degraded_u8 = add_noise(clean_u8, sigma, generator)
    out = []
    for _ in range(2):
        d, c = crop_pair(degraded_u8, clean_u8, size, generator)
        mode = int(torch.randint(1, 8, (1,), generator=generator, device='cpu'))          # random_augmentation: 1..7, never 0
        out.append((augment(d, mode).float() / 255.0, augment(c, mode).float() / 255.0))
    (d1, c1), (d2, c2) = out
    return d1.contiguous(), d2.contiguous(), c1.contiguous(), c2.contiguous()


def training_batch(images_u8, size, sigmas, generator=None):
    """A batch: images_u8 = list of [3, H, W] uint8 device tensors (sizes may differ); sigmas = per image a noise level, or a
    `--de_type` name ('denoising_25', 'deraining', 'dehazing': the dataset cycles its tasks item by item, dataset_utils.py:99)."""
    items = []
    for img, s in zip(images_u8, sigmas):
        if isinstance(s, str):
            items.append(training_pair(img, size, degraded_u8=degrade(img, s, generator), generator=generator))
        else:
            items.append(training_pair(img, size, sigma=s, generator=generator))
    return tuple(torch.stack(t, 0) for t in zip(*items))


# ---------------------------------------------------------------------------------------------------------------
# the whole batch in ONE launch (csrc/fw_data.hip: fw_train_batch) -- no host round trip per crop
# ---------------------------------------------------------------------------------------------------------------
_TASK_SITE = 0x7A000000

# ---------------------------------------------------------------------------------------------------------------
# rain, haze and motion blur synthesised INSIDE the launch (csrc/fw_data.hip: fw_train_batch_synth).  They are stand-ins for the
# paired training sets the reference reads from disk -- enough to train every task of `4tasks` from clean images alone -- and not
# models of Rain100L / SOTS / GoPro.  The device evaluates integers only; the two tables below are built here once, in float64.
# ---------------------------------------------------------------------------------------------------------------
SYNTH_CODES = {'deraining': 1, 'dehazing': 2, 'deblurring': 3}
HAZE_BETAS = np.linspace(0.6, 1.8, 16)                                     # the range add_haze draws from
_t = np.arange(32, dtype=np.float64)[None, :]
_th = (np.pi * np.arange(32, dtype=np.float64) / 32.0)[:, None]
# RAY[a][t] = (dy, dx) of step t along angle pi a / 32 (a = 0: along x, a = 16: down y); halves round up (floor(v + 0.5))
RAY = np.stack([np.floor(_t * np.sin(_th) + 0.5), np.floor(_t * np.cos(_th) + 0.5)], -1).astype(np.int8)
# HAZE_T[j][k] = transmission * 65535 at depth 1 - 0.9 k / 255 (add_haze's vertical ramp: far at the top row, k = 0)
HAZE_T = np.floor(65535.0 * np.exp(-HAZE_BETAS[:, None] * (1.0 - 0.9 * np.arange(256, dtype=np.float64)[None, :] / 255.0)) + 0.5).astype(np.uint16)
del _t, _th
RAIN_DENSITY16, RAIN_STRENGTH8, HAZE_AIRLIGHT8 = 164, 179, 204             # 1/400 of the pixels seed a streak; 0.7 * 255; 0.8 * 255
BLUR_MAX_TAPS, RAIN_MAX_LENGTH = 25, 32
_dev_tables = {}


def rain_length(size):
    return min(RAIN_MAX_LENGTH, max(4, int(size) // 8))


def synth_tables(device):
    """(RAY, HAZE_T) on `device`, uploaded once."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else (torch.cuda.current_device() if device.type == 'cuda' else 0))
    t = _dev_tables.get(key)
    if t is None:
        t = _dev_tables[key] = (torch.from_numpy(RAY.copy()).to(device), torch.from_numpy(HAZE_T.view(np.int16).copy()).to(device))
    return t


def synth_record(task, *p):
    """One parameter record [8] of fw_train_batch_synth: deraining (a, L, density16, S8) | dehazing (j, A8) | deblurring (a, n)."""
    code = SYNTH_CODES[task]
    p = [int(v) for v in p]
    if code == 1:
        a, L = p[:2]
        dens, s8 = (p[2] if len(p) > 2 else RAIN_DENSITY16), (p[3] if len(p) > 3 else RAIN_STRENGTH8)
        assert 0 <= a < 32 and 1 <= L <= RAIN_MAX_LENGTH and 0 <= dens <= 65536 and 0 <= s8 <= 255
        return [1, a, L, dens, s8, 0, 0, 0]
    if code == 2:
        j, a8 = (p + [HAZE_AIRLIGHT8])[:2]
        assert 0 <= j < 16 and 0 <= a8 <= 255
        return [2, j, a8, 0, 0, 0, 0, 0]
    a, n = p
    assert 0 <= a < 32 and 1 <= n <= BLUR_MAX_TAPS and n % 2 == 1
    return [3, a, n, 0, 0, 0, 0, 0]


def synthesize_u8(clean_u8, task, params, seed, site):
    """The full degraded image (uint8 [3, H, W]) of one sample: `task` in SYNTH_CODES, params as synth_record takes them, (seed, site) as
    fw_train_batch_synth keys its rain layer (slot b of a batch uses site + b).  Same per-pixel device code as the batch kernel; for
    inspection and for writing examples, not for the training loop."""
    clean_u8 = clean_u8.contiguous()
    assert clean_u8.dtype == torch.uint8 and clean_u8.dim() == 3 and clean_u8.shape[0] == 3
    dev = clean_u8.device
    ray, hz = synth_tables(dev)
    prm = torch.tensor(synth_record(task, *params), dtype=torch.int32).to(dev)
    sd = torch.tensor([int(seed) - (1 << 32) if int(seed) >= (1 << 31) else int(seed)], dtype=torch.int32).to(dev)
    out = torch.empty_like(clean_u8)
    call('fw_synth_image', clean_u8, prm, ray, hz, sd, int(site), out, clean_u8.shape[1], clean_u8.shape[2])
    return out


class DeviceBatcher:
    """Training batches from uint8 images resident in HBM at device rate.

    images_u8: list of [3, H, W] uint8 device tensors (sizes may differ).  tasks[i]: a noise level, or a `--de_type` name; denoising is
    synthesised INSIDE the kernel (counter-based N(0, 1) per pixel of the full image, so the two crops of a sample share their noise
    exactly as the reference's two crops of one noisy image do, dataset_utils.py:126,131-132); 'deraining' / 'dehazing' samples carry
    a degraded image made once at construction (the reference reads those pairs from disk, :93-95,129).  degraded_u8: optional list
    beside images_u8; where an entry is given (a uint8 tensor of its image's shape, e.g. the pair read from disk by fwair.data) it IS
    the sample's degraded image, instead of the synthetic stand-in or the in-kernel noise.
    `batch(indices)`: crop origins and flip / rotation modes of the whole batch from ONE device RNG call, one kernel launch, no sync.
    The pointer table of a given index list is built once and cached (a training loop cycles a fixed schedule of index lists).
    synth='kernel' (default 'once'): 'deraining' / 'dehazing' / 'deblurring' samples without a given degraded image carry a task code
    instead of a pre-made image, and fw_train_batch_synth makes their rain / haze / motion blur in the launch, with parameters drawn
    afresh per batch from the same ONE RNG call (blur: n odd in 7..25, angle index 0..31; rain: angle index 5..11 = 28..62 degrees,
    length min(32, max(4, size / 8)), 1/400 seeds, strength 179 / 255; haze: beta index 0..15, airlight 204).  `degraded[i]` stays
    None for them.  A batcher without such a sample calls fw_train_batch as before."""

    def __init__(self, images_u8, tasks, size, generator=None, degraded_u8=None, synth='once'):
        from . import functional as Fn
        assert synth in ('once', 'kernel')
        self.size = int(size)
        self.images = [im.contiguous() for im in images_u8]
        self.dev = self.images[0].device
        self.degraded, self.sigma, self.code = [], [], []
        given = list(degraded_u8) if degraded_u8 is not None else [None] * len(self.images)
        assert len(given) == len(self.images)
        for im, t, dg in zip(self.images, tasks, given):
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[0] == 3 and min(im.shape[1:]) >= self.size
            code = 0
            if dg is not None:
                assert dg.dtype == torch.uint8 and dg.shape == im.shape and dg.device == im.device
                self.degraded.append(dg.contiguous()); self.sigma.append(0.0)
            elif synth == 'kernel' and t in SYNTH_CODES:
                code = SYNTH_CODES[t]
                self.degraded.append(None); self.sigma.append(0.0)
            elif isinstance(t, str) and not t.startswith('denoising'):
                self.degraded.append(degrade(im, t, generator).contiguous()); self.sigma.append(0.0)
            else:
                sg = float(t.split('_')[-1]) if isinstance(t, str) else float(t)
                self.degraded.append(None); self.sigma.append(sg)
            self.code.append(code)
        self.random_sigma = [s == 0.0 and d is None and isinstance(t, str) and c == 0
                             for s, d, t, c in zip(self.sigma, self.degraded, tasks, self.code)]
        self.synth = any(self.code)
        self.seed = Fn.dropout_seed(self.dev)
        self._tables = {}
        self._ptables = {}
        self._calls = 0
        self.last_params = None

    def _table(self, idx):
        key = tuple(idx)
        t = self._tables.get(key)
        if t is None:
            rows = [[self.images[i].data_ptr(), self.degraded[i].data_ptr() if self.degraded[i] is not None else 0,
                     self.images[i].shape[1], self.images[i].shape[2]] for i in idx]
            sig = torch.tensor([self.sigma[i] for i in idx], dtype=torch.float32)
            rs = torch.tensor([self.random_sigma[i] for i in idx], dtype=torch.bool)
            t = self._tables[key] = (torch.tensor(rows, dtype=torch.int64).to(self.dev), sig.to(self.dev), rs.to(self.dev))
        return t

    def _param_table(self, idx):
        """Per index list, cached: (code column [B, 1], moduli / factors / offsets [B, 2] of the two drawn fields, fixed fields [B, 5]),
        so that a batch's records are  offset + factor * (draw % modulus)  in three device ops."""
        key = tuple(idx)
        t = self._ptables.get(key)
        if t is None:
            L = rain_length(self.size)
            #        code: (modulus, factor, offset) of p1, of p2, then p3, p4
            rule = {0: ((1, 0, 0), (1, 0, 0), 0, 0),
                    1: ((7, 1, 5), (1, 0, L), RAIN_DENSITY16, RAIN_STRENGTH8),
                    2: ((16, 1, 0), (1, 0, HAZE_AIRLIGHT8), 0, 0),
                    3: ((32, 1, 0), (10, 2, 7), 0, 0)}
            rows = [rule[self.code[i]] for i in idx]
            i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(self.dev)
            t = self._ptables[key] = (i32([[self.code[i]] for i in idx]), i32([[r[0][0], r[1][0]] for r in rows]),
                                      i32([[r[0][1], r[1][1]] for r in rows]), i32([[r[0][2], r[1][2]] for r in rows]),
                                      i32([[r[2], r[3], 0, 0, 0] for r in rows]))
        return t

    def batch(self, indices, generator=None, rnd=None, params=None):
        """-> (degrad_patch_1, degrad_patch_2, clean_patch_1, clean_patch_2), f32 [B, 3, S, S] in [0, 1].
        rnd (int32 [B, >= 7], non-negative: y1, x1, mode1, y2, x2, mode2, sigma choice[, two parameter draws]) and params (int32 [B, 8]
        records of fw_train_batch_synth, see synth_record) replace the draw and the derived records: tests place every mode and every
        parameter extreme with them.  None: drawn here."""
        B, S = len(indices), self.size
        tab, sigma, rs = self._table(indices)
        synth = self.synth or params is not None
        if rnd is None:
            rnd = torch.randint(0, 2 ** 31 - 1, (B, 9 if synth else 7), dtype=torch.int32, device=self.dev, generator=generator)
        else:
            rnd = torch.as_tensor(rnd, dtype=torch.int32).to(self.dev)
            assert rnd.dim() == 2 and rnd.shape[0] == B and rnd.shape[1] >= (9 if synth and params is None else 7)
        if bool(any(self.random_sigma[i] for i in indices)):          # denoising_0: sigma drawn from {15, 25, 50} per sample (:124-125)
            choice = torch.tensor([15.0, 25.0, 50.0], device=self.dev)[(rnd[:, 6] % 3).long()]
            sigma = torch.where(rs, choice, sigma)
        out = [torch.empty((B, 3, S, S), dtype=torch.float32, device=self.dev) for _ in range(4)]
        self._calls += 1
        site = _TASK_SITE + (self._calls & 0xFFFF) * 256
        if synth:
            if params is None:
                code, mod, mul, off, fixed = self._param_table(indices)
                params = torch.cat([code, off + mul * (rnd[:, 7:9] % mod), fixed], 1)
            else:
                params = torch.as_tensor(params, dtype=torch.int32).to(self.dev).contiguous()
                assert params.shape == (B, 8)
            ray, hazet = synth_tables(self.dev)
            call('fw_train_batch_synth', tab, rnd[:, :6].contiguous(), sigma.contiguous(), params, ray, hazet, self.seed, site, *out, B, S)
        else:
            call('fw_train_batch', tab, rnd[:, :6].contiguous(), sigma.contiguous(), self.seed, site, *out, B, S)
        self.last_rnd, self.last_site, self.last_sigma, self.last_params = rnd, site, sigma, params if synth else None
        return tuple(out)
