"""Tiled evaluation on the device (reference test.py:36-71, utils/val_utils.py:50-66).

The reference cuts a test image into `crop_test_imgs_size` tiles at stride = tile size plus one last tile flush with the
border (test.py:47-48), runs the network on the stack of tiles (:57) and averages the overlap (:59-68).  It then accumulates
the INPUT tiles instead of the restored ones (:65, `patched_input_img[cnt]`), so its reported PSNR is that of the degraded
image; this module averages the RESTORED tiles, as the surrounding code intends (`accumulate='input'` reproduces the reference's
literal behaviour).  Everything stays on the GPU: fw_tile_gather cuts the tiles, one batched forward per `max_tiles`, fw_tile_blend
averages the overlap (gather form, no atomics), PSNR as utils/val_utils.py:52-63 and SSIM by fw_ssim7 (skimage's
structural_similarity defaults: 7x7 uniform window, sample covariance, 3-pixel border cropped -- scikit-image itself is not a dependency).

`EvalEngine` does the same for a whole test set at a time: images of different sizes are taken in chunks that fill a fixed tile buffer,
one fw_eval_gather / fw_eval_blend / fw_eval_ssim7 launch per chunk (tables in device memory), the network at ONE fixed batch shape
replayed from a HIP graph, metrics left on the device -- no host synchronisation per image.  With a tile overlap, the x8 self-ensemble
or images smaller than the tile it plans with `plan_tiles_ex` and launches fw_restore_gather / fw_restore_blend instead: tiles that may
leave the image (reflection), a ramp-weighted overlap, the eight flips / rotations turned back before they are averaged.
"""
import sys

import numpy as np
import torch

from .lib import call, gc_quiet, graph_capture


def tile_origins(size, tile):
    """test.py:47-48: range(0, size - tile, tile) + [size - tile]."""
    assert size >= tile, 'invalid test image size'
    return list(range(0, size - tile, tile)) + [size - tile]


@torch.no_grad()
def tiled_restore(net, img, tile=128, max_tiles=64, accumulate='restored'):
    """img: f32 [1, C, H, W] on the device -> restored [1, C, H, W] (overlap-averaged)."""
    assert img.dim() == 4 and img.shape[0] == 1 and tile % 8 == 0
    _, C, H, W = img.shape
    ys, xs = tile_origins(H, tile), tile_origins(W, tile)
    dev = img.device
    img = img.contiguous().float()
    yd, xd = torch.tensor(ys, dtype=torch.int32, device=dev), torch.tensor(xs, dtype=torch.int32, device=dev)
    tiles = torch.empty((len(ys) * len(xs), C, tile, tile), dtype=torch.float32, device=dev)
    call('fw_tile_gather', img, yd, xd, tiles, C, H, W, len(ys), len(xs), tile)
    if accumulate == 'input':                                  # test.py:65 as written
        rest = tiles
    else:
        outs = [net(x_query=tiles[i:i + max_tiles], x_key=tiles[i:i + max_tiles]) for i in range(0, tiles.shape[0], max_tiles)]
        rest = torch.cat(outs, 0).float().contiguous()
    out = torch.empty((1, C, H, W), dtype=torch.float32, device=dev)
    call('fw_tile_blend', rest, yd, xd, out, C, H, W, len(ys), len(xs), tile)
    return out


def psnr(restored, clean):
    """utils/val_utils.py:52-63 for a batch: mean over images of 10 log10(1 / mse(clip(a), clip(b)))."""
    a, b = restored.float().clamp(0, 1), clean.float().clamp(0, 1)
    mse = ((a - b) ** 2).flatten(1).mean(1)
    return float((10.0 * torch.log10(1.0 / mse)).mean())


def ssim(restored, clean):
    """utils/val_utils.py:64: mean over images of structural_similarity(clean, restored, data_range=1, channel_axis=2) on the device."""
    a, b = restored.float().contiguous(), clean.float().contiguous()
    assert a.shape == b.shape and a.dim() == 4 and a.is_cuda
    n, C, H, W = a.shape
    out = torch.zeros(n, dtype=torch.float32, device=a.device)
    call('fw_ssim7', a, b, out, n, C, H, W)
    return float((out / (C * (H - 6) * (W - 6))).mean())


# ---------------------------------------------------------------------------------------------------------------
# a whole test set at a time
# ---------------------------------------------------------------------------------------------------------------
_EVAL_SITE = 0x7B000000


def plan_tiles(sizes, tile, chunk_tiles):
    """sizes: [(H, W)] -> (ttab, gtab, chunks) for fw_eval_gather / fw_eval_blend / fw_eval_ssim7.
    ttab int32 [N, 4] = {image, y0, x0, 0}: the tiles of every image as test.py:47-55 enumerates them (rows major), image after image.
    chunks = [(i0, i1, t0, t1)]: images [i0, i1) own the rows [t0, t1) of ttab, t1 - t0 <= chunk_tiles; a chunk ends at an image
    boundary.  gtab int64 [I, 4] = {offset of the image in its chunk's packed buffer (elements), its first tile counted from t0, ny, nx}."""
    rows, geo, chunks = [], [], []
    i0 = t0 = off = 0
    for i, (H, W) in enumerate(sizes):
        ys, xs = tile_origins(H, tile), tile_origins(W, tile)
        n = len(ys) * len(xs)
        if n > chunk_tiles:
            raise ValueError(f'fwair: image {i} ({H} x {W}) has {n} tiles of {tile}, the tile buffer holds {chunk_tiles}')
        if len(rows) - t0 + n > chunk_tiles:
            chunks.append((i0, i, t0, len(rows)))
            i0, t0, off = i, len(rows), 0
        geo.append((off, len(rows) - t0, len(ys), len(xs)))
        rows += [(i, y, x, 0) for y in ys for x in xs]
        off += 3 * H * W
    chunks.append((i0, len(sizes), t0, len(rows)))
    return np.array(rows, dtype=np.int32).reshape(-1, 4), np.array(geo, dtype=np.int64).reshape(-1, 4), chunks


def tile_origins_ex(size, tile, overlap=0, pad_small=False):
    """Origins along one axis of an image of any size: P = max(size, tile), range(0, P - tile, tile - overlap) + [P - tile].  overlap = 0
    is test.py:47-48.  An image smaller than the tile gets the one origin 0: fw_restore_gather reflects it at the bottom / right."""
    assert 0 <= overlap <= tile // 2
    assert size >= tile or (pad_small and size >= 1), 'invalid test image size'
    P = max(size, tile)
    return list(range(0, P - tile, tile - overlap)) + [P - tile]


def plan_tiles_ex(sizes, tile, chunk_tiles, overlap=0, nmodes=1, pad_small=False):
    """plan_tiles for fw_restore_gather / fw_restore_blend: tiles that overlap by `overlap` pixels (tile_origins_ex), each in `nmodes`
    (1 or 8) flips / rotations, images smaller than the tile allowed with `pad_small`.
    ttab int32 [N, 4] = {image, y0, x0, mode}, the modes of a position next to each other; gtab int64 [I, 8] = {offset in the chunk's
    packed buffer, first tile counted from the chunk's t0, ny, nx, stride, nmodes, 0, 0}; chunks as plan_tiles makes them."""
    assert nmodes in (1, 8)
    rows, geo, chunks = [], [], []
    i0 = t0 = off = 0
    for i, (H, W) in enumerate(sizes):
        ys, xs = tile_origins_ex(H, tile, overlap, pad_small), tile_origins_ex(W, tile, overlap, pad_small)
        n = len(ys) * len(xs) * nmodes
        if n > chunk_tiles:
            raise ValueError(f'fwair: image {i} ({H} x {W}) has {n} tiles of {tile}, the tile buffer holds {chunk_tiles}')
        if len(rows) - t0 + n > chunk_tiles:
            chunks.append((i0, i, t0, len(rows)))
            i0, t0, off = i, len(rows), 0
        geo.append((off, len(rows) - t0, len(ys), len(xs), tile - overlap, nmodes, 0, 0))
        rows += [(i, y, x, m) for y in ys for x in xs for m in range(nmodes)]
        off += 3 * H * W
    chunks.append((i0, len(sizes), t0, len(rows)))
    return np.array(rows, dtype=np.int32).reshape(-1, 4), np.array(geo, dtype=np.int64).reshape(-1, 8), chunks


class EvalEngine:
    """test.py:36-84 for a list of images at device rate.

    run(clean_u8, degraded_u8=None, sigma=0, seed=0, want_u8=False) -> (psnr[I], ssim[I]) as device tensors (+ the restored uint8 images
    when asked; `want_f32` adds the restored f32 images).  clean_u8 / degraded_u8: lists of uint8 [3, H, W] device tensors.  Paired
    sets restore degraded_u8; otherwise the clean images get Gaussian noise of `sigma` (a number or one per image) synthesised inside
    fw_eval_gather from `seed` -- an explicit integer kept in the engine's own device word, NOT the live Dropout seed (which advances
    with every forward), so that the same seed gives the same noisy test images in every process.  clean_u8=None: no ground truth, no
    metrics (both None).
    The network always sees batches of exactly `tile_batch` tiles (the last batch of a chunk is padded with copies of its first tile;
    padded outputs are never read), so that ONE captured HIP graph serves every batch; use_graph=False launches the same forward eagerly.
    Nothing in run() waits for the device once the tables of a given input list are uploaded (they are cached); the caller
    synchronises when it reads the results.  The captured graph reads the weights in place: build a new engine (or call `reset()`)
    after the weights were changed by anything but in-place updates.
    overlap > 0: neighbouring tiles share `overlap` pixels (at most tile / 2) and are blended with a linear ramp of that width, so that
    no tile border shows.  ensemble: every tile also runs in its 7 flips / rotations and the 8 results, turned back, are averaged
    (the tile buffer then holds 8 times as many tiles by default).  pad_small: an image smaller than the tile is reflect-padded at the
    bottom and right instead of refused.  With all three off, and no small image, run() is the path above with its tables and entries;
    otherwise plan_tiles_ex, fw_restore_gather and fw_restore_blend (ramp = max(overlap, 1)) take their place -- nothing else changes."""

    def __init__(self, net, tile=128, tile_batch=64, use_graph=True, chunk_tiles=None, overlap=0, ensemble=False, pad_small=False):
        assert tile % 8 == 0, 'patch size should be a multiple of window_size'            # test.py:44
        self.net, self.tile, self.tb = net, int(tile), int(tile_batch)
        self.use_graph = bool(use_graph)
        self.overlap, self.ensemble, self.pad_small = int(overlap), bool(ensemble), bool(pad_small)
        if not 0 <= self.overlap <= self.tile // 2:
            raise ValueError(f'fwair: tile overlap {overlap} is not in 0 .. tile / 2 = {self.tile // 2}')
        self.cap = -(-int(chunk_tiles or 16 * self.tb * (8 if self.ensemble else 1)) // self.tb) * self.tb
        self.dev = next(net.parameters()).device
        self._seed = 0
        self.seed_word = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.tiles = self.rest = self.gin = self.gout = self.packed = None
        self._graph = None
        self._plans = {}

    def reset(self):
        self._graph = self.gout = None

    # ---- tables ------------------------------------------------------------------------------------------------------
    def _plan(self, clean, degraded, sigma):
        ref = clean if clean is not None else degraded
        I = len(ref)
        sig = [float(s) for s in sigma] if isinstance(sigma, (list, tuple)) else [float(sigma)] * I
        key = (tuple((t.data_ptr(), tuple(t.shape)) for t in clean) if clean is not None else None,
               tuple((t.data_ptr(), tuple(t.shape)) for t in degraded) if degraded is not None else None, tuple(sig), self.cap,
               self.overlap, self.ensemble, self.pad_small)
        plan = self._plans.get(key)
        if plan is None:
            for lst in (clean, degraded):
                for t, r in zip(lst or (), ref):
                    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[0] == 3 and t.is_contiguous() and t.device == self.dev
                    assert t.shape == r.shape, 'a degraded image must have the shape of its ground truth'
            sizes = [tuple(t.shape[1:]) for t in ref]
            ex = self.overlap > 0 or self.ensemble or any(min(h, w) < self.tile for h, w in sizes)
            if ex:
                ttab, gtab, chunks = plan_tiles_ex(sizes, self.tile, self.cap, self.overlap, 8 if self.ensemble else 1, self.pad_small)
            else:                                            # today's tables for today's entries: bit-identical results
                ttab, gtab, chunks = plan_tiles(sizes, self.tile, self.cap)
            itab = np.array([[clean[i].data_ptr() if clean is not None else 0, degraded[i].data_ptr() if degraded is not None else 0,
                              sizes[i][0], sizes[i][1]] for i in range(I)], dtype=np.int64)
            up = lambda a: torch.from_numpy(a).to(self.dev)
            if len(self._plans) >= 8:
                self._plans.clear()
            plan = self._plans[key] = dict(
                I=I, sizes=sizes, chunks=chunks, ex=ex, itab=up(itab), ttab=up(ttab), gtab=up(gtab),
                gtab4=up(np.ascontiguousarray(gtab[:, :4])), sigma=up(np.array(sig, dtype=np.float32)),
                npix=up(np.array([3.0 * h * w for h, w in sizes], dtype=np.float32)),
                nwin=up(np.array([3.0 * max(h - 6, 0) * max(w - 6, 0) for h, w in sizes], dtype=np.float32)),   # no 7 x 7 window: nan
                max_px=max(sum(3 * h * w for h, w in sizes[i0:i1]) for i0, i1, _, _ in chunks))
        return plan

    # ---- the network at one fixed shape ------------------------------------------------------------------------------
    def _buffers(self, plan):
        T = self.tile
        if self.tiles is None:
            self.tiles = torch.empty((self.cap, 3, T, T), dtype=torch.float32, device=self.dev)
            self.rest = torch.empty((self.cap, 3, T, T), dtype=torch.float32, device=self.dev)
            self.gin = torch.zeros((self.tb, 3, T, T), dtype=torch.float32, device=self.dev)
        if self.packed is None or self.packed.numel() < plan['max_px']:
            self.packed = torch.empty(plan['max_px'], dtype=torch.float32, device=self.dev)

    @gc_quiet()                                              # collect before the warm-up, no collection until the graph exists
    def _capture(self):
        cur = torch.cuda.current_stream()
        s = torch.cuda.Stream()
        s.wait_stream(cur)
        with torch.cuda.stream(s):                           # lazily built tables and operand copies must exist before the capture
            for _ in range(2):
                self.net(x_query=self.gin, x_key=self.gin)
        cur.wait_stream(s)
        torch.cuda.synchronize()
        try:
            g = torch.cuda.CUDAGraph()
            with graph_capture(g):
                self.gout = self.net(x_query=self.gin, x_key=self.gin)
            self._graph = g
        except RuntimeError as e:
            print(f'fwair: EvalEngine could not capture the forward pass ({type(e).__name__}: {e}); running it eagerly', file=sys.stderr)
            torch.cuda.synchronize()
            self.use_graph, self._graph, self.gout = False, None, None

    def _forward(self, s, k):
        """rest[s : s + k] = net(tiles[s : s + k]), k <= tile_batch."""
        if k == self.tb:
            self.gin.copy_(self.tiles[s:s + k])
        else:
            self.gin[:k].copy_(self.tiles[s:s + k])
            self.gin[k:].copy_(self.tiles[s:s + 1].expand(self.tb - k, -1, -1, -1))
        if self.use_graph and self._graph is None:
            self._capture()
        if self._graph is not None:
            self._graph.replay()
            out = self.gout
        else:
            out = self.net(x_query=self.gin, x_key=self.gin)
        self.rest[s:s + k].copy_(out[:k])

    @torch.no_grad()
    def run(self, clean_u8, degraded_u8=None, sigma=0, seed=0, want_u8=False, want_f32=False):
        plan = self._plan(clean_u8, degraded_u8, sigma)
        self._buffers(plan)
        seed = int(seed) & 0xFFFFFFFF
        if seed != self._seed:
            self.seed_word.fill_(seed - (1 << 32) if seed >= (1 << 31) else seed)
            self._seed = seed
        was_training = self.net.training
        self.net.eval()
        I, T = plan['I'], self.tile
        sse = torch.zeros(I, dtype=torch.float32, device=self.dev)
        ssum = torch.zeros(I, dtype=torch.float32, device=self.dev)
        u8s, f32s = [], []
        for i0, i1, t0, t1 in plan['chunks']:
            n = t1 - t0
            ttab = plan['ttab'][t0:]
            call('fw_restore_gather' if plan['ex'] else 'fw_eval_gather', plan['itab'], ttab, plan['sigma'], self.seed_word, _EVAL_SITE,
                 self.tiles, n, T)
            for s in range(0, n, self.tb):
                self._forward(s, min(self.tb, n - s))
            px = sum(3 * h * w for h, w in plan['sizes'][i0:i1])
            u8 = torch.empty(px, dtype=torch.uint8, device=self.dev) if want_u8 else None
            if plan['ex']:
                call('fw_restore_blend', plan['itab'], plan['gtab'], ttab, self.rest, self.packed, u8, sse, i0, i1 - i0, n, T,
                     max(self.overlap, 1))
            else:
                call('fw_eval_blend', plan['itab'], plan['gtab'], ttab, self.rest, self.packed, u8, sse, i0, i1 - i0, n, T)
            if clean_u8 is not None:
                call('fw_eval_ssim7', plan['itab'], plan['gtab4'], self.packed, ssum, i0, i1 - i0)     # [I][4]: the first four columns
            off = 0
            for h, w in plan['sizes'][i0:i1]:
                if want_u8:
                    u8s.append(u8[off:off + 3 * h * w].view(3, h, w))
                if want_f32:
                    f32s.append(self.packed[off:off + 3 * h * w].view(3, h, w).clone())
                off += 3 * h * w
        self.net.train(was_training)
        if clean_u8 is None:
            out = (None, None)
        else:
            out = (10.0 * torch.log10(plan['npix'] / sse), ssum / plan['nwin'])          # val_utils.py:52-63: 10 log10(1 / mse)
        return out + ((u8s,) if want_u8 else ()) + ((f32s,) if want_f32 else ())
