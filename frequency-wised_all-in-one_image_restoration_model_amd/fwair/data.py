"""Image folders on disk -> training batches and test sets on the device (reference utils/dataset_utils.py, restated without
torchvision or torch.utils.data; PIL and numpy decode, everything after the decode lives in HBM).

Data tree (the reference's `data/`, here any `--data_root`):

    <root>/denoising_train/GT/*                      clean images; the noise of denoising_<sigma> is synthesised (dataset_utils.py:89-92)
    <root>/<task>_train/{GT,Input}/*                 pairs: Input/<pre>_<rest>.<suf> belongs to GT/<pre>.<suf> (:31-46, :93-95)
    <root>/denoising_bsd68_test/GT/*                 test set of `denoising_bsd68_<sigma>` (:161-164)
    <root>/<task>_test/{GT,Input}/*                  paired test sets (:165-167)

Importing this module needs no GPU; FolderTrainSet and FolderTestSet.load upload to the device they are given.
"""
import os
import random
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def pair_ids(dir, need_synthesize=False):
    """dataset_utils.py:18-48 `get_data_ids` -> (gt_ids, input_ids).  need_synthesize: every file of GT/ is an item and its input id
    is ''.  Otherwise every file Input/<pre>_<rest>.<suf> pairs with GT/<pre>.<suf> (pre = the name up to its first '.' and first '_').
    Directories are listed SORTED: os.listdir's order, which the reference uses as it comes, depends on the file system, and a run
    would not be reproducible from one machine to the next."""
    dir = os.path.join(dir, '')
    input_dir, gt_dir = dir + 'Input/', dir + 'GT/'
    gt_ids, input_ids = [], []
    if need_synthesize:
        for file in sorted(os.listdir(gt_dir)):
            gt_ids.append(os.path.join(gt_dir, file))
            input_ids.append('')
    else:
        for file in sorted(os.listdir(input_dir)):
            pre = file.split('.')[0].split('_')[0]
            suf = file.split('.')[-1]
            gt_ids.append(os.path.join(gt_dir, pre + '.' + suf))
            input_ids.append(os.path.join(input_dir, file))
    return gt_ids, input_ids


def crop_img(arr, base=16):
    """utils/image_utils.py:59-64 on an HWC array: centre crop to multiples of `base` (the reference's default is 64; every caller in
    dataset_utils.py passes 16)."""
    h, w = arr.shape[0], arr.shape[1]
    crop_h, crop_w = h % base, w % base
    return arr[crop_h // 2:h - crop_h + crop_h // 2, crop_w // 2:w - crop_w + crop_w // 2, :]


def load_u8(path, crop=True):
    """dataset_utils.py:118: crop_img(np.array(Image.open(path).convert('RGB')), base=16), returned channels first: uint8 [3, H, W].
    crop=False keeps the image's own size (restore.py --keep_size)."""
    from PIL import Image
    with Image.open(path) as im:
        arr = np.array(im.convert('RGB'))
    return np.ascontiguousarray((crop_img(arr, base=16) if crop else arr).transpose(2, 0, 1))


def _name(path):
    return path.split('/')[-1].split('.')[0]                    # dataset_utils.py:119,183,186


def _task_dir(root, task, split):
    """dataset_utils.py:87-95 / :160-167: denoising tasks drop their sigma suffix."""
    if 'denoising' in task:
        task = task[0:-(len(task.split('_')[-1]) + 1)]
    return os.path.join(root, task + '_' + split, '')


def _decode_all(paths):
    """{path: uint8 [3, H, W]} of the distinct paths, decoded once each by at most 16 threads (PIL releases the GIL while decoding)."""
    uniq = sorted(set(paths))
    if not uniq:
        return {}
    with ThreadPoolExecutor(max_workers=min(16, len(uniq))) as pool:
        return dict(zip(uniq, pool.map(load_u8, uniq)))


class TaskSchedule:
    """The item stream of TrainDataset.__getitem__ (dataset_utils.py:97-139): item k belongs to task k % len(de_type); every task walks
    its own list round and round, and reshuffles it whenever its own iterator stands at 0 -- by the loop at :101-104 exactly as written
    (`randrange(1, t + 1)` for t = n-1 .. 1: position 0 never moves).  The reference draws from the global `random`; this class owns a
    private random.Random(seed), so that a schedule does not depend on who else draws.
    `next()` -> (task number, index into that task's list as it was given); `take(n)` -> the next n of them."""

    def __init__(self, de_type, counts, seed=0):
        assert len(de_type) == len(counts) and all(c > 0 for c in counts)
        self.de_type = list(de_type)
        self.order = [list(range(c)) for c in counts]
        self.de_iterator = [0] * len(counts)
        self.de_type_iterator = 0
        self.rng = random.Random(seed)

    def next(self):
        de_num = self.de_type_iterator % len(self.de_type)
        ids = self.order[de_num]
        if self.de_iterator[de_num] == 0:
            for t in reversed(range(1, len(ids))):
                j = self.rng.randrange(1, t + 1)
                ids[t], ids[j] = ids[j], ids[t]
        item = (de_num, ids[self.de_iterator[de_num]])
        self.de_iterator[de_num] = (self.de_iterator[de_num] + 1) % len(ids)
        self.de_type_iterator = (self.de_type_iterator + 1) % len(self.de_type)
        return item

    def take(self, n):
        return [self.next() for _ in range(n)]


def steps_per_epoch(items_per_task, n_tasks, per_gpu_batch, world):
    """len(TrainDataset) = 400 * len(de_type) (dataset_utils.py:143-144) under a DataLoader with drop_last."""
    return items_per_task * n_tasks // (per_gpu_batch * world)


def shard(items, rank, per_gpu_batch):
    """A global step consumes per_gpu_batch * world consecutive items; rank r takes [r * B, (r + 1) * B)."""
    return items[rank * per_gpu_batch:(rank + 1) * per_gpu_batch]


class FolderTrainSet:
    """TrainDataset (dataset_utils.py:69-147) with the images resident in HBM and the per-item work in one fw_train_batch launch.

    Every distinct file is decoded once (denoising_15 / _25 / _50 share denoising_train/GT) and kept as uint8 on `device`; one
    fwair.augment.DeviceBatcher serves all tasks -- denoising noise is synthesised in the kernel, paired tasks pass the degraded image
    read from disk.  `epoch(e)` yields (degrad_patch_1, degrad_patch_2, clean_patch_1) per step.  Every rank builds the same
    TaskSchedule (same seed) and takes its slice of each global step; crop origins and flip / rotation modes come from a device
    generator seeded with seed + 7919 * rank.  The schedule runs on from epoch to epoch as the reference's dataset object does.
    synthesize: tasks of de_type ('deraining', 'dehazing', 'deblurring') that need no Input/ folder: their clean images are
    <task>_train/GT if that exists, else denoising_train/GT (decoded once, shared), and their degraded crops are made inside the batch
    launch (DeviceBatcher synth='kernel': stand-ins for the paired sets, new streaks / haze / blur every batch)."""

    def __init__(self, root, de_type, patch_size, device, rank=0, world=1, per_gpu_batch=None, items_per_task=400, seed=0, cache_gb=48,
                 synthesize=()):
        import torch
        from .augment import SYNTH_CODES, DeviceBatcher
        self.de_type = list(de_type)
        self.rank, self.world = int(rank), int(world)
        self.B = int(per_gpu_batch or len(self.de_type))
        self.items_per_task = int(items_per_task)
        self.device = torch.device(device)
        self.synthesize = [t for t in self.de_type if t in set(synthesize)]
        unknown = sorted(set(synthesize) - set(SYNTH_CODES))
        if unknown:
            raise ValueError(f'fwair.data: no in-kernel synthesis for {unknown} (known: {sorted(SYNTH_CODES)})')
        ids = []
        for task in self.de_type:
            if task in self.synthesize:              # clean images only: the task's own GT/ if it has one, else the denoising set's
                own = _task_dir(root, task, 'train')
                gt, inp = pair_ids(own if os.path.isdir(own + 'GT/') else _task_dir(root, 'denoising_0', 'train'), True)
            else:
                gt, inp = pair_ids(_task_dir(root, task, 'train'), 'denoising' in task)
            if not gt:
                raise FileNotFoundError(f'fwair.data: no training images for {task!r} under {_task_dir(root, task, "train")}')
            ids.append(list(zip(gt, inp)))
        host = _decode_all([p for t in ids for pair in t for p in pair if p])
        small, kept = 0, []
        for t in ids:
            ok = []
            for gt, inp in t:
                g = host[gt]
                if inp and host[inp].shape != g.shape:
                    raise ValueError(f'fwair.data: {inp} is {host[inp].shape[1:]} after crop_img, its ground truth {gt} is {g.shape[1:]}')
                if min(g.shape[1:]) < patch_size:
                    small += 1
                    continue
                ok.append((gt, inp))
            kept.append(ok)
        if small:                  # the reference would raise inside random.randint(0, H - size), dataset_utils.py:53-54
            warnings.warn(f'fwair.data: skipped {small} training images smaller than patch_size {patch_size} after crop_img')
        for task, ok in zip(self.de_type, kept):
            if not ok:
                raise ValueError(f'fwair.data: every training image of {task!r} is smaller than patch_size {patch_size}')
        used = sorted({p for t in kept for pair in t for p in pair if p})
        need = sum(host[p].nbytes for p in used)
        if need > cache_gb * 2 ** 30:
            raise MemoryError(f'fwair.data: the decoded training set needs {need / 2 ** 30:.1f} GiB of device memory, above '
                              f'--data_cache_gb {cache_gb:g}; pass --data_cache_gb {int(need / 2 ** 30) + 1} or more '
                              '(streaming from host memory is not implemented)')
        dev = {p: torch.from_numpy(host[p]).to(self.device) for p in used}
        self.bytes = need
        images, degraded, tasks, self.base, self.names = [], [], [], [], []
        for task, ok in zip(self.de_type, kept):
            self.base.append(len(images))
            for gt, inp in ok:
                images.append(dev[gt]); degraded.append(dev[inp] if inp else None); tasks.append(task)
                self.names.append((_name(gt), task))
        self.counts = [len(ok) for ok in kept]
        self.schedule = TaskSchedule(self.de_type, self.counts, seed)
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed) + 7919 * self.rank)
        if self.synthesize:
            # a listed task's samples have no pair; an unlisted paired task always has one, so 'kernel' touches the listed ones only
            self.batcher = DeviceBatcher(images, tasks, patch_size, degraded_u8=degraded, synth='kernel')
        else:
            self.batcher = DeviceBatcher(images, tasks, patch_size, degraded_u8=degraded)
        self.steps = steps_per_epoch(self.items_per_task, len(self.de_type), self.B, self.world)

    def indices(self, items):
        """Schedule items -> indices into the batcher's image list."""
        return [self.base[t] + i for t, i in items]

    def epoch(self, e):
        for _ in range(self.steps):
            items = self.schedule.take(self.B * self.world)
            if len(self.batcher._tables) > 1024:              # the batcher caches a pointer table per index list; a shuffled stream never repeats one
                self.batcher._tables.clear()
                self.batcher._ptables.clear()
            d1, d2, c1, _ = self.batcher.batch(self.indices(shard(items, self.rank, self.B)), generator=self.generator)
            yield d1, d2, c1


class FolderTestSet:
    """TestDataset (dataset_utils.py:150-197): `denoising_bsd68_25` reads <root>/denoising_bsd68_test/GT/ and carries sigma 25 (the
    noise itself is synthesised by fw_eval_gather); any other task reads the pairs of <root>/<task>_test/.  names[i] as :183,186."""

    def __init__(self, root, task):
        self.task = task
        self.sigma = 0
        synth = 'denoising' in task
        if synth:
            self.sigma = int(task.split('_')[-1])
            if self.sigma == 0:
                raise ValueError(f'fwair.data: test task {task!r} has sigma 0 (dataset_utils.py:179-180 asserts)')
        self.gt_ids, self.input_ids = pair_ids(_task_dir(root, task, 'test'), synth)
        self.names = [_name(g if synth else i) for g, i in zip(self.gt_ids, self.input_ids)]

    def __len__(self):
        return len(self.gt_ids)

    def load(self, device):
        """-> (clean uint8 [3, H, W] device tensors, degraded ones or None for a synthesised task)."""
        import torch
        host = _decode_all([p for p in self.gt_ids + self.input_ids if p])
        clean = [torch.from_numpy(host[p]).to(device) for p in self.gt_ids]
        if self.sigma:
            return clean, None
        return clean, [torch.from_numpy(host[p]).to(device) for p in self.input_ids]
