"""Training data from the user's own files: a stored time series (or ready-made triplets), cut into
(img0, img1, gt) = (t, t + 2 gap, t + gap) triplets -- Flow-3D/load_datasets.py:29-190 `load_data`.

Three layers:
  * `load_series`: .npy (memory-mapped), .npz, .pkl (one pickled numpy array, the reference's own format);
  * `TripletPlan`: the index arithmetic -- which frames, which crop, which mirrors, which normalisation -- as
    64-byte records (ops.TRIPLET_JOB), pure numpy, no GPU;
  * `SeriesWriter` / `encode_numpy`: the way back -- an .npy file written frame by frame in a stored type
    (reconstruct.reconstruct_series), and the rule ops.series_encode applies, in numpy;
  * `FileTriplets` (a Dataset: the records applied with numpy, for the host loaders) and `DeviceSeriesLoader` (the
    stored array uploaded once in its stored type, a batch = one ops.triplet_gather launch over its records).

The reference appends flipped COPIES of the array (:147-152, 4x the memory); here a mirror is a bit in a record.
"""
import os
import pickle

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import ops

STORED_DTYPES = (np.uint8, np.uint16, np.float16, np.float32)
AUGMENT = ("ref", "none", "full")
NORMALIZE = ("global", "frame", "none")


def load_series(path, key=None, allow_pickle=False, nd=None):
    """The array stored in `path`, in its stored type (uint8 / uint16 / float16 / float32; float64 is narrowed to
    float32; anything else is refused).  `.npy` is memory-mapped, `.npz` needs `key` unless it holds one array, `.pkl`
    must hold one numpy array and is only opened with allow_pickle=True (un-pickling runs code from the file).
    With `nd` (2 or 3) the layout is checked too (`series_layout`)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        arr = np.load(path, mmap_mode="r", allow_pickle=False)
    elif ext == ".npz":
        with np.load(path, allow_pickle=False) as z:
            names = list(z.files)
            if key is None:
                if len(names) != 1:
                    raise ValueError("%s holds %s: name one with key / --series_key" % (path, names))
                key = names[0]
            if key not in names:
                raise ValueError("%s has no array %r (it holds %s)" % (path, key, names))
            arr = z[key]
    elif ext in (".pkl", ".pickle"):
        if not allow_pickle:
            raise ValueError("%s is a pickle: un-pickling executes code from the file, so it is only opened with "
                             "allow_pickle=True / --allow_pickle (or convert it to .npy once)" % path)
        with open(path, "rb") as f:
            arr = pickle.load(f)
        if not isinstance(arr, np.ndarray):
            raise ValueError("%s holds a %s, expected one numpy array" % (path, type(arr).__name__))
    else:
        raise ValueError("unknown series format %r: .npy, .npz or .pkl" % ext)
    if arr.dtype == np.float64:
        arr = arr.astype(np.float32)
    if arr.dtype not in [np.dtype(t) for t in STORED_DTYPES]:
        raise ValueError("%s stores %s: supported are uint8, uint16, float16, float32 (float64 is narrowed)" %
                         (path, arr.dtype))
    if arr.ndim < 3 or arr.ndim > 5:
        raise ValueError("%s has shape %s: expected [T,D,H,W], [T,1,D,H,W], [N,3,D,H,W] or the 2-D forms without D" %
                         (path, arr.shape))
    if nd is not None:
        series_layout(arr.shape, nd)
    return arr


def series_layout(shape, nd):
    """(kind, n, frame): 'series' with n frames ([T,*sp] or [T,1,*sp]) or 'triplets' with n items ([N,3,*sp], channels
    img0, img1, gt); frame = the nd spatial extents."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == nd + 1:
        return "series", shape[0], shape[1:]
    if len(shape) == nd + 2 and shape[1] == 1:
        return "series", shape[0], shape[2:]
    if len(shape) == nd + 2 and shape[1] == 3:
        return "triplets", shape[0], shape[2:]
    sp = ",".join("DHW"[3 - nd:])
    raise ValueError("a %d-D model takes [T,%s], [T,1,%s] or [N,3,%s], got %s" % (nd, sp, sp, sp, shape))


def frame_stats_numpy(arr, nframes):
    """[nframes, 3] float64: minimum and maximum over each frame's finite elements, count of non-finite ones -- what
    ops.series_stats computes on the GPU."""
    flat = np.asarray(arr).reshape(nframes, -1)
    out = np.empty((nframes, 3), np.float64)
    for t in range(nframes):
        v = flat[t].astype(np.float32)
        fin = np.isfinite(v)
        bad = int(v.size - fin.sum())
        if bad:
            v = v[fin]
        out[t] = (v.min() if v.size else np.inf, v.max() if v.size else -np.inf, bad)
    return out


class TripletPlan:
    """Which triplets a stored array yields, as records: pure index arithmetic.

    shape, nd     the stored array's shape and the model's dimensionality (`series_layout`)
    gap, stride   series only: item k is (img0, img1, gt) = frames (t, t + 2 gap, t + gap), t = first + k * stride;
                  the defaults 1 and 3 are the reference's non-overlapping `range(0, T, 3)` (load_datasets.py:174-175)
    first, stop   the frame range (series) or item range (triplets) this plan may use -- the train / validation split
    train         False: validation -- never augmented, centre crop
    augment       'ref': with N base items the set has 4N, item i is base i % N with H mirrored when (i // N) & 1 and D
                  mirrored when (i // 2N) & 1 -- the items of load_datasets.py:147-152's two np.append calls, in their
                  order, by index.  (The reference flips FRAMES and then cuts triplets, so the two agree when the range
                  holds a multiple of 3 frames -- 750 in the reference; a triplet here never straddles two flipped
                  copies.)  A 2-D array is a series of one-plane volumes: its D mirror changes nothing, as in the
                  reference's arithmetic on [T,1,1,H,W].  'none': the N base items.
                  'full': 'ref' plus, drawn per item from (seed, epoch, i), the W mirror and the swap of img0 and img1.
    crop          None (whole frame) or nd extents, multiples of `multiple` (32: what the models take without padding,
                  evaluate._pad32); origins drawn per item from (seed, epoch, i), along W in steps
                  of 4 elements (fs_triplet_gather then loads 4 elements at once; any origin is valid in a record)
    normalize     'none': lo = 0, inv = 1.  'global': lo / 1/(hi - lo) over the finite elements of all frames.
                  'frame': over the three frames of the item (one pair per item keeps their relative brightness).
                  Needs `set_stats`.
    """

    def __init__(self, shape, nd, gap=1, stride=3, first=0, stop=None, train=True, augment="ref", crop=None,
                 normalize="none", seed=1234, multiple=32):
        self.kind, self.n, self.frame = series_layout(shape, nd)
        self.nd = nd
        if gap < 1 or stride < 1:
            raise ValueError("gap and stride must be >= 1, got %d, %d" % (gap, stride))
        if augment not in AUGMENT:
            raise ValueError("augment must be one of %s, got %r" % (AUGMENT, augment))
        if normalize not in NORMALIZE:
            raise ValueError("normalize must be one of %s, got %r" % (NORMALIZE, normalize))
        stop = self.n if stop is None else stop
        if not 0 <= first <= stop <= self.n:
            raise ValueError("range [%d, %d) is not inside the %d stored %s" %
                             (first, stop, self.n, "frames" if self.kind == "series" else "items"))
        self.gap, self.stride, self.first, self.stop = gap, stride, first, stop
        if self.kind == "series":
            if stop - first < 2 * gap + 1:
                raise ValueError("a triplet at gap %d spans %d frames, the range [%d, %d) holds %d" %
                                 (gap, 2 * gap + 1, first, stop, stop - first))
            starts = np.arange(first, stop - 2 * gap, stride, dtype=np.int64)
            self.base = np.stack([starts, starts + 2 * gap, starts + gap], 1)  # frame indices of img0, img1, gt
        else:
            if stop - first < 1:
                raise ValueError("the item range [%d, %d) is empty" % (first, stop))
            items = np.arange(first, stop, dtype=np.int64)
            self.base = np.stack([3 * items, 3 * items + 1, 3 * items + 2], 1)
        self.crop = tuple(self.frame) if crop is None else tuple(int(c) for c in crop)
        if len(self.crop) != nd:
            raise ValueError("crop needs %d extents, got %s" % (nd, self.crop))
        for c, f in zip(self.crop, self.frame):
            if c < 1 or c > f:
                raise ValueError("crop %s is larger than the stored frames %s" % (self.crop, self.frame))
            if c % multiple:
                raise ValueError("crop extents must be multiples of %d (the model pads anything else), got %s%s" %
                                 (multiple, self.crop, "" if crop is not None else ": pass crop / --crop"))
        self.train, self.augment, self.normalize, self.seed = train, augment if train else "none", normalize, seed
        self.stats = None
        self.norm_range = None

    @property
    def frame_elems(self):
        return int(np.prod(self.frame))

    @property
    def nframes(self):
        return self.n if self.kind == "series" else 3 * self.n

    def __len__(self):
        return len(self.base) * (1 if self.augment == "none" else 4)

    def set_stats(self, stats, norm_range=None):
        """stats: [nframes, >= 2] (min, max) per stored frame (frame_stats_numpy / ops.series_stats).  norm_range:
        (lo, hi) to use under 'global' instead of this array's own -- a validation file takes the training file's; a
        range set earlier (here or by assigning `norm_range`) stays unless a new one is given."""
        self.stats = np.asarray(stats, np.float64)
        if self.stats.shape[0] != self.nframes:
            raise ValueError("stats for %d frames, the array has %d" % (self.stats.shape[0], self.nframes))
        if norm_range is not None:
            self.norm_range = norm_range

    def global_range(self):
        if self.norm_range is not None:
            return self.norm_range
        return float(self.stats[:, 0].min()), float(self.stats[:, 1].max())

    def records(self, epoch=0):
        """The ops.TRIPLET_JOB record of every item, for `epoch`: a function of (seed, epoch) and the item's index."""
        n, N = len(self), len(self.base)
        i = np.arange(n)
        rec = np.zeros(n, ops.TRIPLET_JOB)
        frames = self.base[i % N]
        flip = np.zeros(n, np.uint32)
        origin = np.stack([np.full(n, (f - c) // 2, np.int64) for f, c in zip(self.frame, self.crop)], 1)
        if self.augment != "none":
            first_bit, second_bit = 2, 4  # H, then D
            flip |= np.where((i // N) & 1, first_bit, 0).astype(np.uint32)
            flip |= np.where((i // (2 * N)) & 1, second_bit, 0).astype(np.uint32)
        if self.train:
            rng = np.random.default_rng([self.seed, epoch])  # item i owns position i of each draw
            draws = rng.random((n, 5))
            origin = np.stack([np.minimum((draws[:, k] * (f - c + 1)).astype(np.int64), f - c)
                               for k, (f, c) in enumerate(zip(self.frame, self.crop))], 1)
            origin[:, -1] -= origin[:, -1] % 4  # W origins in steps of 4 elements: the gather's vector-load path
            if self.augment == "full":
                flip ^= (draws[:, 3] < 0.5).astype(np.uint32)  # the W mirror
                swap = draws[:, 4] < 0.5
                frames = np.where(swap[:, None], frames[:, [1, 0, 2]], frames)
        rec["off"] = frames * self.frame_elems
        for k, name in enumerate(("z0", "y0", "x0")[3 - self.nd:]):
            rec[name] = origin[:, k]
        rec["flip"] = flip
        rec["lo"], rec["inv"] = 0.0, 1.0
        if self.normalize != "none":
            if self.stats is None:
                raise ValueError("normalize=%r needs the per-frame minima and maxima: call set_stats" % self.normalize)
            if self.normalize == "global":
                lo, hi = self.global_range()
                lo, hi = np.full(n, lo), np.full(n, hi)
            else:
                lo, hi = self.stats[frames, 0].min(1), self.stats[frames, 1].max(1)
            lo = np.where(np.isfinite(lo), lo, 0.0).astype(np.float32)
            hi = np.where(np.isfinite(hi), hi, 0.0).astype(np.float32)
            d = hi - lo  # fp32
            rec["lo"] = lo
            rec["inv"] = np.where(d > 0, np.float32(1) / np.where(d > 0, d, np.float32(1)), np.float32(1))
        return rec


def gather_numpy(arr, rec, frame, crop):
    """One record applied with numpy: fp32 [3,*crop], the values ops.triplet_gather writes, bit for bit."""
    nd = len(crop)
    frame3, crop3 = (1,) * (3 - nd) + tuple(frame), (1,) * (3 - nd) + tuple(crop)
    F = int(np.prod(frame3))
    flat = arr.reshape(-1)
    out = np.empty((3,) + crop3, np.float32)
    z0, y0, x0 = int(rec["z0"]), int(rec["y0"]), int(rec["x0"])
    flip = int(rec["flip"])
    for c in range(3):
        o = int(rec["off"][c])
        blk = flat[o:o + F].reshape(frame3)[z0:z0 + crop3[0], y0:y0 + crop3[1], x0:x0 + crop3[2]]
        if flip & 4:
            blk = blk[::-1]
        if flip & 2:
            blk = blk[:, ::-1]
        if flip & 1:
            blk = blk[:, :, ::-1]
        v = blk.astype(np.float32)
        if not np.issubdtype(arr.dtype, np.integer):
            v[~np.isfinite(v)] = 0.0
        out[c] = (v - np.float32(rec["lo"])) * np.float32(rec["inv"])
    return out.reshape((3,) + tuple(crop))


ENCODE_LIMITS = {"uint8": (0.0, 255.0), "uint16": (0.0, 65535.0), "float16": (-65504.0, 65504.0)}


def encode_numpy(x, dtype, lo=0.0, span=1.0):
    """fp32 `x` as `dtype` by the rule of ops.series_encode, bit for bit: y = x * span, then y + lo (two rounded fp32
    operations); a non-finite y is stored as 0; uint8 / uint16 clamp to the type and round to nearest even, float16
    saturates at +-65504 and rounds to nearest even, float32 keeps y.  With lo = 0, span = 1 this is also the
    conversion a stored keyframe gets when the output type differs from its own."""
    dtype = np.dtype(dtype)
    if dtype not in [np.dtype(t) for t in STORED_DTYPES]:
        raise ValueError("encode to uint8, uint16, float16 or float32, got %s" % dtype)
    with np.errstate(all="ignore"):
        y = np.asarray(x, np.float32) * np.float32(span)
        y = y + np.float32(lo)
        y = np.where(np.isfinite(y), y, np.float32(0))
        if dtype.name in ENCODE_LIMITS:
            a, b = ENCODE_LIMITS[dtype.name]
            y = np.clip(y, np.float32(a), np.float32(b))
            if dtype.kind == "u":
                y = np.rint(y)
        return y.astype(dtype)


class SeriesWriter:
    """An .npy file of `shape` and `dtype` written frame by frame (numpy.lib.format.open_memmap: the header first, the
    frames in place, nothing held in memory).  `source`: the file the series was read from -- writing over it is
    refused (the input is a memory map of that file).  An existing file is refused unless `overwrite`.  `close()`
    flushes; also a context manager."""

    def __init__(self, path, shape, dtype, overwrite=False, source=None):
        if os.path.splitext(path)[1].lower() != ".npy":
            raise ValueError("the output is written as .npy, got %r" % path)
        if source is not None and os.path.realpath(path) == os.path.realpath(source):
            raise ValueError("%s is the input itself: write the result somewhere else" % path)
        if os.path.exists(path) and not overwrite:
            raise FileExistsError("%s exists: pass overwrite=True / --overwrite to replace it" % path)
        dtype = np.dtype(dtype)
        if dtype not in [np.dtype(t) for t in STORED_DTYPES]:
            raise ValueError("write uint8, uint16, float16 or float32, got %s" % dtype)
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        self.path, self.shape, self.dtype = path, tuple(int(s) for s in shape), dtype
        self._mm = np.lib.format.open_memmap(path, mode="w+", dtype=dtype, shape=self.shape)

    def write(self, index, frame):
        """Frame `index` = `frame` (any shape with the frame's element count, the file's dtype)."""
        if self._mm is None:
            raise ValueError("%s is closed" % self.path)
        if not 0 <= index < self.shape[0]:
            raise IndexError("frame %d of %d" % (index, self.shape[0]))
        frame = np.asarray(frame)
        if frame.dtype != self.dtype:
            raise ValueError("frame %d is %s, the file stores %s" % (index, frame.dtype, self.dtype))
        self._mm[index] = frame.reshape(self.shape[1:])

    def close(self):
        if self._mm is not None:
            self._mm.flush()
            self._mm = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FileTriplets(Dataset):
    """A stored array seen through a TripletPlan: `__len__`, `__getitem__`, `item(i, device)` like the synthetic set,
    so DataLoader, HostCachedLoader and DeviceTripletLoader work on it unchanged (these gather on the host with
    numpy).  `set_epoch(e)` moves on to epoch e's crops and draws."""

    def __init__(self, arr, plan):
        self.arr, self.plan = arr, plan
        self.epoch = 0
        self._rec = None

    def set_epoch(self, epoch):
        if epoch != self.epoch:
            self.epoch = epoch
            self.invalidate()

    def invalidate(self):
        """The plan changed (another epoch, another normalisation range): rebuild the records on next use."""
        self._rec = None

    def records(self):
        if self._rec is None:
            if self.plan.normalize != "none" and self.plan.stats is None:
                self.plan.set_stats(frame_stats_numpy(self.arr, self.plan.nframes))
            self._rec = ops.check_triplet_jobs(self.plan.records(self.epoch), int(np.prod(self.arr.shape)),
                                               (1,) * (3 - self.plan.nd) + tuple(self.plan.frame),
                                               (1,) * (3 - self.plan.nd) + tuple(self.plan.crop))
        return self._rec

    def __len__(self):
        return len(self.plan)

    def __getitem__(self, i):
        return self.item(i, "cpu")

    def item(self, i, device):
        if not 0 <= i < len(self):
            raise IndexError(i)
        t = torch.from_numpy(gather_numpy(self.arr, self.records()[i], self.plan.frame, self.plan.crop))
        return t if str(device) == "cpu" else t.to(device)


# the step's working set per byte of batch: a Flow-3D step at 2 x 256^3 (a 403 MB batch) keeps about 23 GB
STEP_BYTES_PER_BATCH_BYTE = 64


class DeviceSeriesLoader:
    """DataLoader stand-in for FileTriplets: the same batches (sampler order, `drop_last` rule, item values) as
    `DataLoader(dataset, ...)`, but the stored array lives on the GPU in its stored type (uploaded once, here) and a
    batch is one ops.triplet_gather launch.  At the start of an epoch the whole epoch's records go to the device in
    one copy; from then to the epoch's last batch nothing is copied between host and device and nothing
    synchronises."""

    def __init__(self, dataset, batch_size, device, sampler=None, shuffle=False, drop_last=False, seed=0,
                 stored=None):
        self.dataset, self.batch_size, self.device = dataset, batch_size, torch.device(device)
        self.sampler, self.shuffle, self.drop_last = sampler, shuffle, drop_last
        self._gen = torch.Generator().manual_seed(seed)
        arr, plan = dataset.arr, dataset.plan
        if stored is not None:  # another loader over the same array has uploaded it
            self.stored = stored
            return
        free, _ = torch.cuda.mem_get_info(self.device)
        batch_bytes = 4 * 3 * batch_size * int(np.prod(plan.crop))
        room = free - STEP_BYTES_PER_BATCH_BYTE * batch_bytes
        if arr.nbytes > room:
            raise RuntimeError(
                "the stored series (%.2f GB) does not fit next to the training step: %.2f GB free on %s, about %.2f GB "
                "kept for a step at batch %d x %s -- use --host_data (the series stays in host memory)" %
                (arr.nbytes / 1e9, free / 1e9, self.device, STEP_BYTES_PER_BATCH_BYTE * batch_bytes / 1e9, batch_size,
                 plan.crop))
        self.stored = torch.empty(arr.shape, dtype=getattr(torch, arr.dtype.name), device=self.device)
        flat, src = self.stored.view(-1), arr.reshape(-1)
        chunk = max(1, (256 << 20) // arr.dtype.itemsize)  # a memory-mapped file is read 256 MB at a time
        for a in range(0, src.shape[0], chunk):
            flat[a:a + chunk].copy_(torch.from_numpy(np.array(src[a:a + chunk])))
        if plan.normalize != "none" and plan.stats is None:
            plan.set_stats(ops.series_stats(self.stored.view(plan.nframes, -1)).cpu().numpy())

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        if self.sampler is not None:
            order = list(iter(self.sampler))
        elif self.shuffle:
            order = torch.randperm(len(self.dataset), generator=self._gen).tolist()
        else:
            order = list(range(len(self.dataset)))
        B, nb, crop = self.batch_size, len(self), self.dataset.plan.crop
        order = order[:nb * B]
        if not order:
            return
        jobs = ops.upload_triplet_jobs(self.dataset.records()[np.asarray(order)], self.stored, crop, checked=True)
        for k in range(nb):
            rows = jobs[k * B:(k + 1) * B]
            yield ops.triplet_gather(self.stored, rows, (rows.shape[0], 3) + tuple(crop))
