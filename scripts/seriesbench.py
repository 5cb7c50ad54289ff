"""Batches from a device-resident series: ops.triplet_gather (fs_triplet_gather) against the stock formulation on the
same GPU (index the three frames, flip, slice, to(float32), subtract, multiply, stack), B = 2 crops of 256^3 out of a
16-frame series, f32 and u8 storage.  Times are HIP events around `iters` calls after `warmup` calls, the two
alternating per case; bytes are the compulsory traffic (ops.triplet_gather_cost), set against the 8 TB/s HBM peak
(AMD's MI355X spec; ~6.3 TB/s is what a float4 copy reaches).

With --train: `flow3d.train` at 2 x 256^3 (default driver) on three data paths in this one call -- device-generated
synthetic triplets (twice: the box's spread), `--series` device-resident, `--series --host_data --host_cache` -- each a
child process, ms/step from the trainer's own "train loop" line.

    python scripts/seriesbench.py [--train] [--out profiles/seriesbench.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402

HBM_BPS = 8.0e12


def torch_gather(stored, rec, crop):
    """The stock formulation of one batch."""
    F = stored[0].numel()
    out = []
    for r in rec:
        z0, y0, x0, fl = int(r["z0"]), int(r["y0"]), int(r["x0"]), int(r["flip"])
        dims = [d for d, bit in ((1, 4), (2, 2), (3, 1)) if fl & bit]
        fr = torch.stack([stored[int(o) // F] for o in r["off"]])
        fr = fr[:, z0:z0 + crop[0], y0:y0 + crop[1], x0:x0 + crop[2]]
        if dims:
            fr = fr.flip(dims)
        out.append((fr.to(torch.float32) - float(r["lo"])) * float(r["inv"]))
    return torch.stack(out)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def case(name, stored, flip, x0, crop, warmup, iters):
    F = stored[0].numel()
    rec = np.zeros(2, ops.TRIPLET_JOB)
    rec["off"] = np.array([[0, 2, 1], [9, 11, 10]]) * F
    rec["x0"], rec["flip"], rec["lo"], rec["inv"] = x0, flip, 0.5, 1 / 3
    jobs = ops.upload_triplet_jobs(rec, stored, crop)
    shape = (2, 3) + crop
    out = torch.empty(shape, device="cuda")
    ms = timed(lambda: ops.triplet_gather(stored, jobs, shape, out=out), warmup, iters)
    ms_t = timed(lambda: torch_gather(stored, rec, crop), warmup, iters)
    ms = min(ms, timed(lambda: ops.triplet_gather(stored, jobs, shape, out=out), 1, iters))
    ms_t = min(ms_t, timed(lambda: torch_gather(stored, rec, crop), 1, iters))
    same = bool(torch.equal(ops.triplet_gather(stored, jobs, shape), torch_gather(stored, rec, crop)))
    nbytes, _ = ops.triplet_gather_cost(2, crop, stored.element_size())
    return {"case": name, "dtype": str(stored.dtype), "crop": list(crop), "flip": flip, "x0": x0, "hip_ms": ms,
            "torch_ms": ms_t, "speedup_vs_torch": ms_t / ms, "algo_bytes": nbytes, "hip_TBps": nbytes / ms / 1e9,
            "share_of_hbm_roof": nbytes / HBM_BPS * 1e3 / ms, "equal_to_torch": same}


def copy_case(warmup, iters):
    """A float4 copy of the gather's output size: what this box's HBM gives a plain stream today."""
    a = torch.empty(2 * 3 * 256 ** 3, device="cuda").normal_()
    b = torch.empty_like(a)
    ms = timed(lambda: b.copy_(a), warmup, iters)
    return {"case": "torch copy_ of 403 MB", "ms": ms, "TBps": 2 * a.numel() * 4 / ms / 1e9,
            "share_of_hbm_roof": 2 * a.numel() * 4 / HBM_BPS * 1e3 / ms}


def train_runs(tmp, steps_samples=24):
    from opticalflowscivis_amd.data import synthetic
    seq = synthetic.droplet3d_sequence(18, 256, seed=3, device="cuda")
    path = os.path.join(tmp, "series_u8.npy")
    np.save(path, torch.round(seq * 255).to(torch.uint8).cpu().numpy())
    del seq
    torch.cuda.empty_cache()
    base = [sys.executable, "-m", "opticalflowscivis_amd.flow3d.train", "--mode", "train", "--epoch", "2", "--batch_size",
            "2", "--log_every", "1000", "--log_path", tmp]
    synth = ["--dataset", "droplet3d", "--size", "256", "--samples", str(steps_samples)]
    series = ["--series", path, "--val_from", "15", "--stride", "1", "--augment", "none"]  # 13 items, 6 steps per epoch
    runs = [("synthetic, device-generated (1)", synth), ("synthetic, device-generated (2)", synth),
            ("--series, device-resident", series), ("--series --host_data --host_cache", series + ["--host_data", "--host_cache"])]
    rows = []
    for name, extra in runs:
        r = subprocess.run(base + extra, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        out = r.stdout.decode()
        if r.returncode != 0:
            raise SystemExit("train run %r failed:\n%s" % (name, out[-3000:]))
        ms = [float(m) for m in re.findall(r"train loop: \d+ steps in [0-9.]+ s = ([0-9.]+) ms/step", out)]
        rows.append({"path": name, "ms_per_step_by_epoch": ms, "ms_per_step": ms[-1]})  # (epoch 0 holds the graph capture)
        print("%-42s %s ms/step" % (name, ms), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seriesbench needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for dt in (torch.float32, torch.float16, torch.uint8):
        S = (16, 256, 256, 264)  # rows of 264 leave room for an unaligned origin
        if dt == torch.float32:
            stored = torch.rand(S, device="cuda", generator=g)
        elif dt == torch.float16:
            stored = torch.rand(S, device="cuda", generator=g, dtype=torch.float16)
        else:
            stored = torch.randint(0, 256, S, device="cuda", generator=g, dtype=torch.uint8)
        crop = (256, 256, 256)
        for name, flip, x0 in (("plain", 0, 0), ("D+H mirrored", 6, 0), ("W mirrored", 1, 0), ("origin x0 = 4", 0, 4),
                                ("unaligned origin", 0, 3)):
            rows.append(case(name, stored, flip, x0, crop, args.warmup, args.iters))
            r = rows[-1]
            print("%-8s %-17s HIP %6.3f ms  torch %7.3f ms  x%5.1f  %5.2f TB/s  %.2f of the 8 TB/s roof  equal %s" % (
                r["dtype"].replace("torch.", ""), r["case"], r["hip_ms"], r["torch_ms"], r["speedup_vs_torch"],
                r["hip_TBps"], r["share_of_hbm_roof"], r["equal_to_torch"]), flush=True)
        del stored
    cp = copy_case(args.warmup, args.iters)
    print("%-26s %6.3f ms  %5.2f TB/s  %.2f of the roof" % (cp["case"], cp["ms"], cp["TBps"], cp["share_of_hbm_roof"]))
    doc = {"device": torch.cuda.get_device_name(0), "triplet_gather": rows, "copy": cp}
    torch.cuda.empty_cache()
    if args.train:
        with tempfile.TemporaryDirectory() as tmp:
            doc["train"] = train_runs(tmp)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
