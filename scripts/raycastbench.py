"""Ray casting on the GPU: ops.raycast (fs_raycast3d: one launch; with bricks one more for the jump map) against the same
picture composed from stock torch ops on the same device in the same process: per sample slab k the positions of all
pixels, F.grid_sample (trilinear, border padding, align_corners) for the values, the coverage weights, the table lookup by
index arithmetic, and the emission / absorption blend (or the running maximum) -- a Python loop over the slabs that can
meet the box.  One 256^3 volume of the synthetic jets set, a 1024 x 1024 orthographic picture from azimuth 30, elevation
20, steps of half a node; dvr and mip; the table is the `iso` preset, which leaves most of the volume empty, with and
without the brick ranges (ops.brick_ranges, timed on its own: it is paid once per volume, not per view).

Per case: `warmup` calls of each, then `reps` rounds that time one HIP call and (in the first n rounds, as many as fit
20 s, at least 3) one torch call in turn, each between two HIP events; the table gives the median and the 10th / 90th
percentile.  Gather bytes are the algorithm's (ops.raycast_cost with the samples the kernel counted: 32 bytes per
sample; most of them hit lines a neighbouring ray fetched, so the rate is a cache rate, not an HBM rate).

    python scripts/raycastbench.py [--out profiles/raycast.txt] [--json raycast.json] [--size 256] [--image 1024]

One process, the cases one after another, each under its own time limit (SIGALRM): a case that overruns ends the run."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops, render  # noqa: E402
from opticalflowscivis_amd.data import synthetic  # noqa: E402

CASE_LIMIT_S = 280
TORCH_BUDGET_S = 20.0


def torch_raycast(vol, cam, tf, lo, hi, dt, image, mode, k0, k1):
    """vol [D,H,W], cam 18 numbers, tf [n,4] (all on the device), spacing 1 -> [Hi,Wi,4]; the slabs k0..k1."""
    Hi, Wi = image
    D, H, W = vol.shape
    n = tf.shape[0]
    c = cam.view(6, 3)
    i = torch.arange(Wi, device=vol.device, dtype=torch.float32).view(1, Wi, 1)
    j = torch.arange(Hi, device=vol.device, dtype=torch.float32).view(Hi, 1, 1)
    o = c[0] + i * c[1] + j * c[2]
    g = c[3] + i * c[4] + j * c[5]
    d = g / g.norm(dim=-1, keepdim=True)
    N1 = torch.tensor([W - 1.0, H - 1.0, D - 1.0], device=vol.device)
    v5 = vol[None, None]
    C = torch.zeros(Hi, Wi, 3, device=vol.device)
    T = torch.ones(Hi, Wi, device=vol.device)
    m = torch.zeros(Hi, Wi, device=vol.device)
    for k in range(k0, k1 + 1):
        q = o + ((k + 0.5) * dt) * d
        cov = (1.0 - torch.maximum(-q, q - N1).clamp(min=0.0)).clamp(min=0.0).prod(-1)
        grid = (q.clamp(min=0.0).minimum(N1) * (2.0 / N1) - 1.0).view(1, 1, Hi, Wi, 3)
        v = F.grid_sample(v5, grid, mode="bilinear", padding_mode="border", align_corners=True).view(Hi, Wi)
        u = ((v - lo) * (1.0 / (hi - lo))).clamp(0.0, 1.0)
        if mode == "mip":
            m = torch.maximum(m, cov * u)
            continue
        s = u * (n - 1)
        j0 = s.floor().long().clamp(max=n - 2)
        ft = (s - j0).unsqueeze(-1)
        row = tf[j0] + ft * (tf[j0 + 1] - tf[j0])
        e = torch.exp(-(row[..., 3] * cov) * dt)
        C = C + (T * (1.0 - e)).unsqueeze(-1) * row[..., :3]
        T = T * e
    if mode == "mip":
        s = m * (n - 1)
        j0 = s.floor().long().clamp(max=n - 2)
        return tf[j0] + (s - j0).unsqueeze(-1) * (tf[j0 + 1] - tf[j0])
    return torch.cat([C, (1.0 - T).unsqueeze(-1)], -1)


def pct(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


def timed_pair(fa, fb, warmup, reps):
    """(median, p10, p90) ms of fa over `reps` rounds and of fb (None: not timed) over the first n of them; n."""
    fa()
    n = 0
    if fb is not None:
        fb()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fb()
        torch.cuda.synchronize()
        n = min(reps, max(3, int(TORCH_BUDGET_S / max(time.perf_counter() - t0, 1e-6))))
    for _ in range(warmup):
        fa()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    for i, (a0, a1, b0, b1) in enumerate(ev):
        a0.record()
        fa()
        a1.record()
        if i < n:
            b0.record()
            fb()
            b1.record()
    torch.cuda.synchronize()
    return (pct([e[0].elapsed_time(e[1]) for e in ev]),
            pct([e[2].elapsed_time(e[3]) for e in ev[:n]]) if n else (float("nan"),) * 3, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--image", type=int, default=1024)
    ap.add_argument("--iso", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "raycastbench needs a GPU"
    S, image = args.size, (args.image, args.image)
    vol = synthetic.jets3d_sequence(1, S, device="cuda").contiguous()
    diag = (3 ** 0.5) * (S - 1)
    dt = 0.5
    tf = torch.from_numpy(render.tf_preset("iso:%g" % args.iso, 256, 0.0, 1.0, 8.0 / diag * 20)).cuda()
    cam = torch.from_numpy(render.orbit_camera((S,) * 3, 1.0, 30.0, 20.0, None, image)).cuda()
    # the slabs that can meet the box grown by a cell: the eye is 1.5 diagonals from the centre
    k0 = max(0, int((1.5 * diag - 0.5 * diag - 2.0) / dt) - 1)
    k1 = int((1.5 * diag + 0.5 * diag + 2.0) / dt) + 1
    signal.alarm(CASE_LIMIT_S)
    (bms, blo, bhi), _, _ = timed_pair(lambda: ops.brick_ranges(vol), None, args.warmup, args.reps)
    bricks = ops.brick_ranges(vol)
    signal.alarm(0)
    rows = []
    for mode in ("dvr", "mip"):
        ref_img = None
        for with_bricks in (False, True):
            signal.alarm(CASE_LIMIT_S)
            br = bricks if with_bricks else None
            hip = lambda: ops.raycast(vol, cam, tf, 0.0, 1.0, dt, 1.0, mode, 0.0, br, False, image)
            tch = None if with_bricks else (lambda: torch_raycast(vol[0], cam, tf, 0.0, 1.0, dt, image, mode, k0, k1))
            (ms, lo, hi), (ms_t, lo_t, hi_t), n = timed_pair(hip, tch, args.warmup, args.reps)
            r = ops.raycast(vol, cam, tf, 0.0, 1.0, dt, 1.0, mode, 0.0, br, True, image)
            samples = int(r["counts"].sum(dtype=torch.int64))
            nbytes, flops = ops.raycast_cost((S,) * 3, image, 1, dt, 1.0, samples)
            row = {"mode": mode, "bricks": with_bricks, "volume": [S] * 3, "image": list(image), "reps": args.reps,
                   "hip_ms": ms, "hip_ms_p10": lo, "hip_ms_p90": hi, "samples": samples, "gather_bytes": nbytes,
                   "gather_TBps": nbytes / ms / 1e9, "samples_per_ns": samples / ms / 1e6,
                   "mean_opacity": float(r["image"][..., 3].mean())}
            if tch is not None:
                ref_img = r["image"]
                t_img = tch()
                row.update(torch_ms=ms_t, torch_ms_p10=lo_t, torch_ms_p90=hi_t, torch_reps=n, speedup_vs_torch=ms_t / ms,
                           max_abs_diff_vs_torch=float((t_img - r["image"][0]).abs().max()))
                del t_img
            else:
                row.update(identical_to_no_bricks=bool(torch.equal(r["image"], ref_img)),
                           speedup_vs_no_bricks=rows[-1]["hip_ms"] / ms)
            signal.alarm(0)
            rows.append(row)
            text = table(rows, args, (bms, blo, bhi))
            print(text.splitlines()[-1], flush=True)
            for path, body in ((args.out, text), (args.json, json.dumps(
                    {"device": torch.cuda.get_device_name(0), "brick_ranges_ms": [bms, blo, bhi], "raycast": rows}, indent=1))):
                if path:
                    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                    with open(path, "w") as f:
                        f.write(body)
    print(table(rows, args, (bms, blo, bhi)))
    assert all(r["identical_to_no_bricks"] for r in rows if r["bricks"]), "the brick map changed the picture"


def table(rows, args, brick_ms):
    lines = ["%s, %d rounds after %d warm-up calls; median ms (p10 - p90); %d^3 -> %d^2, iso:%g; ops.brick_ranges %.3f ms "
             "(%.3f - %.3f), once per volume" % ((torch.cuda.get_device_name(0), args.reps, args.warmup, args.size, args.image,
                                                  args.iso) + tuple(brick_ms)),
             "%-4s %-6s %26s %12s %9s %30s %3s %8s  %s" % ("mode", "bricks", "HIP ms", "samples", "gather TB/s", "torch ms", "n",
                                                         "x", "note")]
    for r in rows:
        if r["bricks"]:
            tail = "%30s %3s %8s  same bits as without: %s, %.2fx its time" % ("", "", "", r["identical_to_no_bricks"],
                                                                               1.0 / r["speedup_vs_no_bricks"])
        else:
            tail = "%10.1f (%8.1f - %8.1f) %3d %8.1f  max |d| vs torch %.1e" % (
                r["torch_ms"], r["torch_ms_p10"], r["torch_ms_p90"], r["torch_reps"], r["speedup_vs_torch"],
                r["max_abs_diff_vs_torch"])
        lines.append("%-4s %-6s %8.3f (%7.3f - %7.3f) %12d %9.3f   %s" % (
            r["mode"], "yes" if r["bricks"] else "no", r["hip_ms"], r["hip_ms_p10"], r["hip_ms_p90"], r["samples"],
            r["gather_TBps"], tail))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
