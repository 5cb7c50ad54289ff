"""Streamlines on the GPU: ops.streamlines (fs_streamlines{2,3}d, one lane per line, every vertex kept) against the same
lines composed from stock torch ops on the same device in the same process, in fp32: per step one grid_sample (bilinear,
align_corners=True, border padding) of the field per integrator stage, a normalisation, the position update, a masked
termination and a store of the slot.  The stock form is the comparator for speed only: its fp32 coordinates cannot
reproduce the kernel's bits; the table gives how far the two forms' lines are apart after a quarter of the steps.

Cases: a 64^3 lattice of seeds in a 256^3 field and a 512^2 lattice in a 2048^2 field, M = 256 steps of h = 0.5, each
method; and a skeleton-sized call -- S = 4096 lines in the 256^3 field with the capture plane of its critical points --
next to the ops.critical_points call it follows.

Per case: `warmup` calls of each form, then `reps` rounds that time the forms in turn, each between two HIP events; the
table gives the median and the 10th / 90th percentile.  `Gsample/s` counts the field samples the lines really took
(length x stages; a line that leaves or stagnates takes fewer than M), `len` is the mean length in steps; the share of the
fp64 vector peak (78.6 TFLOP/s, AMD's MI355X spec) prices those samples by ops.streamlines_cost's flop count.

    python scripts/streamlinebench.py [--out profiles/streamlines.txt] [--json streamlines.json]

One process, the cases one after another, each under its own time limit (SIGALRM): a case that overruns ends the run."""
import argparse
import json
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from opticalflowscivis_amd import ops  # noqa: E402
from advectbench import smooth_flows  # noqa: E402
from licbench import timed  # noqa: E402

FP64_FLOPS = 78.6e12
CASE_LIMIT_S = 240
STAGES = {"euler": 1, "rk2": 2, "rk4": 4}
LIC_GSAMPLES = 196.0  # fs_lic3d, RK2, 256^3: profiles/lic.txt


def lattice(sp, n, dev="cuda"):
    """fp64 [n^C, C] cell-centred lattice of seeds over a grid of spatial shape sp, x first."""
    C = len(sp)
    ax = [(torch.arange(n, dtype=torch.float64, device=dev) + 0.5) * ((sp[C - 1 - c] - 1) / n) for c in range(C)]
    mesh = torch.meshgrid(*ax[::-1], indexing="ij")[::-1]
    return torch.stack([m.reshape(-1) for m in mesh], 1).contiguous()


def torch_lines(flows, seeds, M, h, method):
    """flows [1,C,*sp], seeds fp32 [C,S] -> (verts fp32 [M+1,C,S], length int32 [S]) from stock ops in fp32; a line that
    has ended keeps its last position in the remaining slots."""
    C = flows.shape[1]
    sp = tuple(flows.shape[2:])
    dev = flows.device
    S = [sp[C - 1 - c] for c in range(C)]
    scale = torch.tensor([2.0 / max(s - 1, 1) for s in S], device=dev).view(C, 1)
    hi = torch.tensor([float(s - 1) for s in S], device=dev).view(C, 1)

    def unit(q):
        g = (q * scale - 1.0).t().reshape((1,) + (1,) * (C - 1) + (q.shape[1], C))
        v = torch.nn.functional.grid_sample(flows, g, mode="bilinear", padding_mode="border",
                                            align_corners=True).reshape(C, -1)
        return v / v.norm(dim=0, keepdim=True)

    verts = torch.empty((M + 1, C, seeds.shape[1]), dtype=torch.float32, device=dev)
    verts[0] = seeds
    p = seeds
    alive = torch.ones(seeds.shape[1], dtype=torch.bool, device=dev)
    length = torch.zeros(seeds.shape[1], dtype=torch.int32, device=dev)
    for i in range(1, M + 1):
        d1 = unit(p)
        if method == "euler":
            pn = p + h * d1
        elif method == "rk2":
            pn = p + h * unit(p + (0.5 * h) * d1)
        else:
            d2 = unit(p + (0.5 * h) * d1)
            d3 = unit(p + (0.5 * h) * d2)
            d4 = unit(p + h * d3)
            pn = p + (h / 6.0) * (d1 + 2.0 * d2 + 2.0 * d3 + d4)
        alive = alive & ((pn >= 0) & (pn <= hi)).all(0)  # (a NaN direction compares false)
        p = torch.where(alive, pn, p)
        verts[i] = p
        length = length + alive.to(torch.int32)
    return verts, length


def lattice_case(name, sp, n, M, h, method, warmup, reps):
    signal.alarm(CASE_LIMIT_S)
    flows = smooth_flows(1, sp)
    seeds = lattice(sp, n)
    S = seeds.shape[0]
    step = torch.zeros(S, dtype=torch.int32, device="cuda")
    sign = torch.ones(S, dtype=torch.int8, device="cuda")
    s32 = seeds.t().float().contiguous()
    (ms, lo, hi_), (ms_t, lo_t, hi_t) = timed([lambda: ops.streamlines(flows, seeds, step, sign, None, None, M, h, 0.0, method),
                                               lambda: torch_lines(flows, s32, M, h, method)], warmup, reps)
    r = ops.streamlines(flows, seeds, step, sign, None, None, M, h, 0.0, method)
    vt, lt = torch_lines(flows, s32, M, h, method)
    q = M // 4
    both = (r["length"] >= q) & (lt >= q)
    d = (r["verts"][q] - vt[q]).abs().amax(0)[both]
    taken = int(r["length"].sum()) * STAGES[method]
    _, flops = ops.streamlines_cost(sp, S, M, method)
    signal.alarm(0)
    return {"case": name, "shape": list(sp), "S": S, "M": M, "h": h, "method": method, "reps": reps, "hip_ms": ms,
            "hip_ms_p10": lo, "hip_ms_p90": hi_, "torch_ms": ms_t, "torch_ms_p10": lo_t, "torch_ms_p90": hi_t,
            "speedup_vs_torch": ms_t / ms, "samples": taken, "samples_per_s": taken / ms * 1e3,
            "mean_length": float(r["length"].double().mean()), "full_frac": float((r["end"] == 0).float().mean()),
            "share_of_fp64_roof": flops * (taken / float(S * M * STAGES[method])) / FP64_FLOPS * 1e3 / ms,
            "max_abs_dpos_vs_torch_at_quarter": float(d.max()) if d.numel() else float("nan")}


def skeleton_case(sp, S, M, h, warmup, reps):
    signal.alarm(CASE_LIMIT_S)
    flows = smooth_flows(1, sp)
    cp = ops.critical_points(flows)
    N = int(cp["cell"].numel())
    capture = torch.zeros(flows[0, 0].numel(), dtype=torch.uint8, device="cuda")
    capture[cp["cell"].to(torch.int64)] = 1
    capture = capture.view((1,) + tuple(sp))
    g = torch.Generator(device="cuda").manual_seed(2)
    hi = torch.tensor([float(s - 1) for s in sp[::-1]], dtype=torch.float64, device="cuda")
    seeds = torch.rand((S, len(sp)), dtype=torch.float64, device="cuda", generator=g) * hi
    step = torch.zeros(S, dtype=torch.int32, device="cuda")
    sign = (2 * (torch.arange(S, device="cuda") % 2) - 1).to(torch.int8)
    run = lambda: ops.streamlines(flows, seeds, step, sign, None, capture, M, h, 0.0, "rk4")
    (ms, lo, hi_), (ms_c, lo_c, hi_c) = timed([run, lambda: ops.critical_points(flows)], warmup, reps)
    r = run()
    taken = int(r["length"].sum()) * 4
    signal.alarm(0)
    return {"case": "skeleton", "shape": list(sp), "S": S, "M": M, "h": h, "method": "rk4", "hip_ms": ms, "hip_ms_p10": lo,
            "hip_ms_p90": hi_, "critical_ms": ms_c, "critical_ms_p10": lo_c, "critical_ms_p90": hi_c, "critical_points": N,
            "samples": taken, "samples_per_s": taken / ms * 1e3, "mean_length": float(r["length"].double().mean()),
            "captured_frac": float((r["end"] == ops.SL_CAPTURED).float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--h", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "streamlinebench needs a GPU"
    assert args.reps >= 20
    dev = torch.cuda.get_device_name(0)
    lines = ["%s, %d rounds (every form once per round, in turn) after %d warm-up calls; median ms (p10 - p90); K = 1, "
             "M = %d, h = %g, band-limited flows, lattice seeds run with the field" % (dev, args.reps, args.warmup, args.steps, args.h)]
    rows = []
    for name, sp, n in (("256^3 / 64^3", (256,) * 3, 64), ("2048^2 / 512^2", (2048, 2048), 512)):
        for method in ("euler", "rk2", "rk4"):
            rows.append(lattice_case(name, sp, n, args.steps, args.h, method, args.warmup, args.reps))
    lines.append("%-15s %-6s %8s %28s %10s %8s %7s %6s %32s %7s  %s" % (
        "field / seeds", "method", "lines", "HIP ms", "Gsample/s", "x LIC", "of fp64", "len", "torch ms", "x", "full   max |d pos| at M/4"))
    for r in rows:
        lines.append("%-15s %-6s %8d %8.3f (%8.3f - %8.3f) %10.2f %8.4f %7.4f %6.1f %10.3f (%9.3f - %9.3f) %7.1f  %.3f  %.1e" % (
            r["case"], r["method"], r["S"], r["hip_ms"], r["hip_ms_p10"], r["hip_ms_p90"], r["samples_per_s"] / 1e9,
            r["samples_per_s"] / 1e9 / LIC_GSAMPLES, r["share_of_fp64_roof"], r["mean_length"], r["torch_ms"], r["torch_ms_p10"],
            r["torch_ms_p90"], r["speedup_vs_torch"], r["full_frac"], r["max_abs_dpos_vs_torch_at_quarter"]))
    lines.append("x LIC: the rate over fs_lic3d's %.0f Gsample/s (RK2, 256^3, every node a seed, packed image: profiles/lic.txt)" %
                 LIC_GSAMPLES)
    k = skeleton_case((256,) * 3, 4096, args.steps, args.h, args.warmup, args.reps)
    rows.append(k)
    lines.append("skeleton-sized call, 256^3, S = %d random seeds, both directions, RK4, capture plane of the field's %d critical "
                 "points: %.3f (%.3f - %.3f) ms, %.2f Gsample/s, mean length %.1f, %.0f %% captured; the ops.critical_points call "
                 "it follows: %.3f (%.3f - %.3f) ms" % (
                     k["S"], k["critical_points"], k["hip_ms"], k["hip_ms_p10"], k["hip_ms_p90"], k["samples_per_s"] / 1e9,
                     k["mean_length"], 100 * k["captured_frac"], k["critical_ms"], k["critical_ms_p10"], k["critical_ms_p90"]))
    lines.append("packed-image form (lic.hip's pre-pass, then 16-byte corner loads): not measured (not built)")
    print("\n".join(lines))
    for path, text in ((args.out, "\n".join(lines) + "\n"), (args.json, json.dumps({"device": dev, "streamlines": rows}, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
