"""Sequence evaluation of an interpolation model (the reference's third task, error.py:78-150, 374-436): keep every
`factor`-th frame of a time series, rebuild the frames in between with the model by recursive bisection, score every
rebuilt frame with PSNR and SSIM (ops.frame_metrics), compare with a linear blend of the keyframes and select the time
steps whose PSNR falls below a threshold.  Shared by the flow2d / flow3d `evaluate` entry points:

    python -m opticalflowscivis_amd.flow3d.evaluate --dataset jets3d --size 128 --frames 17 --exp 1 2 3 --baseline
    python -m opticalflowscivis_amd.flow2d.evaluate --seq frames.npy --exp 1 2 3 --out result.json

--seq takes a [T,H,W] (flow2d) or [T,D,H,W] (flow3d) array in [0,1]; metrics use data range 1."""
import argparse
import json
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .error import select_from_psnr
from .rife import load_pretrained


def _pad32(x, nd):
    pad = []
    for s in reversed(x.shape[-nd:]):
        pad += [0, ((s - 1) // 32 + 1) * 32 - s]
    return F.pad(x, pad)


def _mid(model, a, b):
    m = model.inference(a, b)[0]
    return m[2] if isinstance(m, list) else m


def bisection_groups(T, factor, batch, device):
    """The model calls of bisect_keyframes on a [T, ...] sequence, in order: [(idx, half, step, positions)] with idx
    the device tensor of the left parents' indices of one group of at most `batch` pairs and positions = the list
    idx + half.  Every index of every level goes up in ONE copy from pinned memory that does not block the host: a
    `torch.tensor(list, device=...)` per group is a pageable copy, and PyTorch synchronises the stream behind it --
    the host would wait for every model call before it could launch the next."""
    groups, flat = [], []
    step = factor
    while step > 1:
        half = step // 2
        left = list(range(0, T - 1, step))
        for i in range(0, len(left), batch):
            g = left[i:i + batch]
            groups.append((len(flat), len(g), half, step, [l + half for l in g]))
            flat += g
        step = half
    if not flat:
        return []
    dev = torch.tensor(flat).pin_memory().to(device, non_blocking=True)
    return [(dev[a:a + n], half, step, pos) for a, n, half, step, pos in groups]


def bisect_keyframes(seq, factor, batch, mid, groups=None):
    """The keyframe-level loop of interpolate_sequence (shared with reconstruct.reconstruct_series, which runs it on
    one chunk of keyframes at a time): seq [T,1,*padded], T = (K-1)*factor + 1, holds the keyframes at seq[::factor];
    every other frame is filled in place, level by level (step = factor, factor/2, ..., 2), the midpoints of one level
    in groups of `batch` pairs from the left: seq[i + step/2] = mid(seq[i], seq[i + step], positions), positions = the
    list of the indices i + step/2 of the group.  groups: bisection_groups(T, factor, batch, device) when the caller
    has them already (the same T again and again); nothing here makes the host wait for the device."""
    if groups is None:
        groups = bisection_groups(seq.shape[0], factor, batch, seq.device)
    with torch.no_grad():
        for idx, half, step, pos in groups:
            seq[idx + half] = mid(seq[idx], seq[idx + step], pos)


def interpolate_sequence(model, frames, factor, batch=1):
    """Rebuild [T, *spatial] `frames` from its keyframes frames[::factor]: recursive bisection with model.inference
    (flow{2,3}d/inference_img.py), inputs padded to multiples of 32 and the results cropped as there.  Every midpoint of
    one bisection level goes through the model in batches of `batch` pairs.  Returns [(K-1)*factor + 1, *spatial] fp32
    on the frames' device, K = number of keyframes; keyframe positions hold the original frames bit for bit."""
    if factor < 1 or factor & (factor - 1):
        raise ValueError("factor must be a power of two (bisection), got %d" % factor)
    nd = frames.dim() - 1
    keys = frames[::factor]
    K = keys.shape[0]
    if K < 2:
        raise ValueError("need at least two keyframes: %d frames at factor %d" % (frames.shape[0], factor))
    T = (K - 1) * factor + 1
    sp = tuple(frames.shape[1:])
    padded = _pad32(keys.to(torch.float32).reshape((K, 1) + sp), nd)
    seq = padded.new_zeros((T,) + tuple(padded.shape[1:]))
    seq[::factor] = padded
    bisect_keyframes(seq, factor, batch, lambda a, b, pos: _mid(model, a, b))
    out = seq[(slice(None), 0) + tuple(slice(0, s) for s in sp)].clone()
    out[::factor] = frames[::factor]  # (bit for bit, also for inputs that are not fp32)
    return out


def ratio_inference(model, img0, img1, ratio, rthreshold=0.02, rmaxcycles=8):
    """The frame at `ratio` in (0, 1) between img0 and img1 by bisection (Flow-3D/inference_img.py:64-87): img0 / img1
    themselves when `ratio` lies within rthreshold / 2 of 0 / 1, else the first midpoint whose position lies within
    rthreshold / 2 of `ratio`, or the last one when `rmaxcycles` bisections did not get there."""
    lo, hi = 0.0, 1.0
    if ratio <= lo + rthreshold / 2:
        return img0
    if ratio >= hi - rthreshold / 2:
        return img1
    if rmaxcycles < 1:
        raise ValueError("rmaxcycles must be >= 1, got %d" % rmaxcycles)
    a, b = img0, img1
    for _ in range(rmaxcycles):
        middle = _mid(model, a, b)
        pos = (lo + hi) / 2
        if ratio - rthreshold / 2 <= pos <= ratio + rthreshold / 2:
            break
        if ratio > pos:
            a, lo = middle, pos
        else:
            b, hi = middle, pos
    return middle


def linear_baseline(frames, factor):
    """Linear blend of the keyframes frames[::factor]: frame k0 + j (0 < j < factor) = (1 - t) k0 + t k1, t = j / factor.
    The reference's loop (error.py:415-421) weights the two keyframes the other way round, t k0 + (1 - t) k1; at factor 2
    (t = 1/2) the two agree."""
    keys = frames[::factor].to(torch.float32)
    K = keys.shape[0]
    T = (K - 1) * factor + 1
    out = keys.new_empty((T,) + tuple(keys.shape[1:]))
    out[::factor] = keys
    for j in range(1, factor):
        t = j / factor
        out[j::factor] = (1 - t) * keys[:-1] + t * keys[1:]
    return out


def _score(pred, gt, factor, window):
    psnr, ssim = ops.frame_metrics(pred.unsqueeze(1), gt.unsqueeze(1), 1.0, window)
    psnr, ssim = psnr.cpu().numpy(), ssim.cpu().numpy()
    mid = [i for i in range(len(psnr)) if i % factor != 0]
    return {"psnr": [float(v) for v in psnr], "ssim": [float(v) for v in ssim],
            "psnr_mean": float(np.mean(psnr[mid])), "ssim_mean": float(np.mean(ssim[mid]))}


def evaluate_sequence(model, seq, exps, batch=1, baseline=False):
    """Per factor 2**exp: per-frame and mean (in-between frames) PSNR / SSIM of the model and, with `baseline`, of the
    linear blend; the selected time steps and their threshold; wall time of inference and of metrics."""
    nd = seq.dim() - 1
    window = "%dd" % nd
    results = []
    for e in exps:
        factor = 2 ** int(e)
        T = (seq.shape[0] - 1) // factor * factor + 1
        gt = seq[:T]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred = interpolate_sequence(model, gt, factor, batch)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r = {"exp": int(e), "factor": factor, "frames": T, "model": _score(pred, gt, factor, window)}
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        sel, thr = select_from_psnr(r["model"]["psnr"], factor)
        r["selected"], r["threshold"] = sel, thr
        if baseline:
            r["baseline"] = _score(linear_baseline(gt, factor), gt, factor, window)
        torch.cuda.synchronize()
        r["time_inference_s"] = t1 - t0
        r["time_metrics_s"] = time.perf_counter() - t1  # (scoring the model's frames and the baseline's)
        results.append(r)
    return results


def _dataset(name, frames, size, seed):
    from .data import synthetic
    if name == "rectangle2d":
        return synthetic.rectangle2d_sequence(frames, seed)[0]
    if name == "droplet2d":
        h, w = (size + size)[:2] if size else (160, 224)
        return synthetic.droplet2d_sequence(frames, h, w, seed)
    s = size[0] if size else 64
    if name == "droplet3d":
        return synthetic.droplet3d_sequence(frames, s, seed)
    if name == "jets3d":
        return synthetic.jets3d_sequence(frames, s, seed)
    raise ValueError("unknown dataset %r" % name)


DATASETS = {2: ("rectangle2d", "droplet2d"), 3: ("droplet3d", "jets3d")}


def _load_seq(path, nd, normalize="none"):
    """--seq FILE through data.series.load_series (.npy / .npz; uint8, uint16, float16, float32 or float64) as fp32
    [T,*sp]; a file of ready-made triplets or of another rank is refused.  normalize 'none' passes the values through
    as stored; 'global' / 'frame' read non-finite values as 0 and map the file's / each frame's range to [0,1]."""
    from .data.series import load_series, series_layout
    arr = load_series(path, nd=nd)
    if series_layout(arr.shape, nd)[0] != "series":
        raise ValueError("--seq takes a series [T,%s], got ready-made triplets %s" % (",".join("DHW"[3 - nd:]), arr.shape))
    arr = np.asarray(arr).astype(np.float32)
    if arr.ndim == nd + 2 and arr.shape[1] == 1:
        arr = arr[:, 0]
    if normalize != "none":
        arr[~np.isfinite(arr)] = 0.0
        ax = None if normalize == "global" else tuple(range(1, arr.ndim))
        lo, hi = arr.min(axis=ax, keepdims=True), arr.max(axis=ax, keepdims=True)
        arr = (arr - lo) / np.where(hi > lo, hi - lo, np.float32(1))
    return torch.from_numpy(arr)


def main(Model, nd, argv=None):
    ap = argparse.ArgumentParser(description="interpolate a time series from every factor-th frame and score it")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dataset", choices=DATASETS[nd], help="synthetic sequence")
    src.add_argument("--seq", help=".npy sequence [T,%s] in [0,1]" % ",".join("DHW"[3 - nd:]))
    ap.add_argument("--normalize", choices=("global", "frame", "none"), default="none",
                    help="--seq: map the stored values to [0,1] by the range of the file / of each frame (default: "
                         "the file is in [0,1] already)")
    ap.add_argument("--frames", type=int, default=17, help="frames of a synthetic sequence")
    ap.add_argument("--size", type=int, nargs="+", default=None, help="synthetic extent (S, or H W in 2-D)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--exp", type=int, nargs="+", default=[1, 2, 3], help="factors 2**exp")
    ap.add_argument("--model", default="train_log", help="directory holding flownet.pkl")
    ap.add_argument("--batch", type=int, default=1, help="midpoints per model call")
    ap.add_argument("--baseline", action="store_true", help="also score the linear blend of the keyframes")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    model = load_pretrained(Model, args.model, dev)
    if args.seq:
        seq = _load_seq(args.seq, nd, args.normalize)
        name = os.path.basename(args.seq)
    else:
        seq = _dataset(args.dataset, args.frames, args.size, args.seed)
        name = args.dataset
    if seq.dim() != nd + 1:
        raise ValueError("sequence must be [T,%s], got %s" % (",".join("DHW"[3 - nd:]), tuple(seq.shape)))
    t0 = time.perf_counter()
    results = evaluate_sequence(model, seq.to(dev), args.exp, args.batch, args.baseline)
    doc = {"sequence": name, "shape": list(seq.shape), "batch": args.batch, "results": results,
           "wall_s": time.perf_counter() - t0}
    for r in results:
        line = "factor %3d: PSNR %.3f dB  SSIM %.5f" % (r["factor"], r["model"]["psnr_mean"], r["model"]["ssim_mean"])
        if "baseline" in r:
            line += "  | linear PSNR %.3f dB  SSIM %.5f" % (r["baseline"]["psnr_mean"], r["baseline"]["ssim_mean"])
        print(line + "  | selected %d (threshold %.3f dB)  inference %.3f s  metrics %.3f s" % (
            len(r["selected"]), r["threshold"], r["time_inference_s"], r["time_metrics_s"]))
    if args.out:
        d = os.path.dirname(os.path.abspath(args.out))
        os.makedirs(d, exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return doc
