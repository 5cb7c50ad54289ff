"""Pathline advection on the GPU: ops.advect (fs_advect{2,3}d, one launch for K steps) against the same motion composed
from stock torch ops on the same device in the same process: one grid_sample (bilinear, align_corners=True, border
padding, fp32) per integrator stage on a normalised grid, fp32 position updates, no status.  The stock form is the
comparator for speed only: its fp32 coordinates cannot reproduce the kernel's positions bit for bit, and it keeps
moving particles that have left the box along the clamped border values.

Per case: `warmup` calls of each, then `reps` rounds that time one HIP call and one torch call in turn, each between two
HIP events; the table gives the median and the 10th / 90th percentile.  Bytes and flops are the algorithm's
(ops.advect_cost: every reachable field element once, positions in and out, status and steps), set against the 8 TB/s
HBM peak and the 78.6 TFLOP/s fp64 vector peak (AMD's MI355X spec); `Ggather/s` counts the 2^C x C corner loads per
sample.  Euler and RK4 of one case move the same bytes and differ fourfold in samples: a time ratio near 1 would mean
the memory system sets the period, one near 4 that the per-sample work (fp64 chain or gather issue) does.

    python scripts/advectbench.py [--out profiles/advect.txt] [--json advect.json]

One process, the cases one after another, each under its own time limit (SIGALRM): a case that overruns ends the run."""
import argparse
import json
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402

HBM_BPS = 8.0e12
FP64_FLOPS = 78.6e12
CASE_LIMIT_S = 150
STAGES = {"euler": 1, "rk2": 2, "rk4": 4}


def torch_advect(pos, flows, method="euler"):
    """pos [C,P], flows [K,C,*sp] -> the last positions [C,P], from stock ops in fp32, one grid_sample per stage."""
    K, C = flows.shape[:2]
    sp = flows.shape[2:]
    S = [sp[C - 1 - c] for c in range(C)]
    scale = torch.tensor([2.0 / max(s - 1, 1) for s in S], device=pos.device).view(C, 1)
    p = pos

    def sample(k, q):
        g = (q * scale - 1.0).t().reshape((1,) + (1,) * (C - 1) + (q.shape[1], C))
        return torch.nn.functional.grid_sample(flows[k:k + 1], g, mode="bilinear", padding_mode="border",
                                               align_corners=True).reshape(C, -1)

    for k in range(K):
        k1 = sample(k, p)
        if method == "euler":
            p = p + k1
        elif method == "rk2":
            p = p + sample(k, p + 0.5 * k1)
        else:
            k2 = sample(k, p + 0.5 * k1)
            k3 = sample(k, p + 0.5 * k2)
            k4 = sample(k, p + k3)
            p = p + (1.0 / 6.0) * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
    return p


def timed_pair(fa, fb, warmup, reps):
    """Median, p10, p90 (ms) of fa and of fb, timed in turn."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    for a0, a1, b0, b1 in ev:
        a0.record()
        fa()
        a1.record()
        b0.record()
        fb()
        b1.record()
    torch.cuda.synchronize()
    out = []
    for i in (0, 2):
        ms = sorted(e[i].elapsed_time(e[i + 1]) for e in ev)
        out.append((ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]))
    return out


def smooth_flows(K, sp, amp=1.5):
    """Band-limited fields: coarse noise up-sampled to the grid, a few elements of motion per step."""
    g = torch.Generator(device="cuda").manual_seed(1)
    C = len(sp)
    coarse = torch.randn((K, C) + (6,) * C, device="cuda", generator=g)
    return (amp * torch.nn.functional.interpolate(coarse, size=sp, mode="trilinear" if C == 3 else "bilinear",
                                                  align_corners=True)).contiguous()


def case(name, sp, K, seeds, method, warmup, reps):
    signal.alarm(CASE_LIMIT_S)
    flows = smooth_flows(K, sp)
    if seeds == "dense":
        pos = ops.grid_seeds(sp, 1, 0, "cuda")
    else:
        g = torch.Generator(device="cuda").manual_seed(2)
        hi = torch.tensor([s - 1 for s in sp[::-1]], device="cuda", dtype=torch.float32).view(-1, 1)
        pos = torch.rand((len(sp), seeds), device="cuda", generator=g) * hi
    P, C = pos.shape[1], len(sp)
    nbytes, flops = ops.advect_cost(sp, P, K, method, 1)
    (ms, lo, hi_), (ms_t, lo_t, hi_t) = timed_pair(lambda: ops.advect(pos, flows, method=method),
                                                   lambda: torch_advect(pos, flows, method), warmup, reps)
    out, st, n = ops.advect(pos, flows, method=method)
    ref = torch_advect(pos, flows, method)
    alive = st == ops.ADV_ALIVE
    d = (out - ref).abs().amax(0)[alive]
    signal.alarm(0)
    gathers = P * K * STAGES[method] * (1 << C) * C
    return {"case": name, "shape": list(sp), "K": K, "P": P, "method": method, "reps": reps, "hip_ms": ms,
            "hip_ms_p10": lo, "hip_ms_p90": hi_, "torch_ms": ms_t, "torch_ms_p10": lo_t, "torch_ms_p90": hi_t,
            "speedup_vs_torch": ms_t / ms, "algo_bytes": nbytes, "algo_flops": flops, "hip_TBps": nbytes / ms / 1e9,
            "share_of_hbm_roof": nbytes / HBM_BPS * 1e3 / ms, "share_of_fp64_roof": flops / FP64_FLOPS * 1e3 / ms,
            "gathers_per_s": gathers / ms * 1e3, "alive_frac": float(alive.float().mean()),
            "max_abs_dpos_vs_torch_alive": float(d.max()) if d.numel() else float("nan")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "advectbench needs a GPU"
    assert args.reps >= 20
    rows = []
    for name, sp, K, seeds in (("dense 128^3, K = 4", (128,) * 3, 4, "dense"), ("dense 256^3, K = 4", (256,) * 3, 4, "dense"),
                               ("1e4 seeds 256^3, K = 16", (256,) * 3, 16, 10000)):
        for method in ("euler", "rk4"):
            rows.append(case(name, sp, K, seeds, method, args.warmup, args.reps))
    lines = ["%s, %d rounds (one HIP call, one torch call in turn) after %d warm-up calls; median ms (p10 - p90); one "
             "launch per HIP call, substeps = 1" % (torch.cuda.get_device_name(0), args.reps, args.warmup),
             "%-24s %-6s %28s %7s %9s %9s %10s %30s %7s  %s" % ("case", "method", "HIP ms", "TB/s", "of 8 TB/s", "of fp64",
                                                              "Ggather/s", "torch ms", "x", "alive   max |d pos| vs torch (alive)")]
    for r in rows:
        lines.append("%-24s %-6s %8.3f (%8.3f - %8.3f) %7.3f %9.3f %9.3f %10.1f %9.3f (%8.3f - %8.3f) %7.1f  %.4f  %.1e"
                     % (r["case"], r["method"], r["hip_ms"], r["hip_ms_p10"], r["hip_ms_p90"], r["hip_TBps"],
                        r["share_of_hbm_roof"], r["share_of_fp64_roof"], r["gathers_per_s"] / 1e9, r["torch_ms"],
                        r["torch_ms_p10"], r["torch_ms_p90"], r["speedup_vs_torch"], r["alive_frac"],
                        r["max_abs_dpos_vs_torch_alive"]))
    for i in range(0, len(rows), 2):
        lines.append("%s: RK4 / Euler time %.2f (same bytes, 4 x the samples)" % (rows[i]["case"], rows[i + 1]["hip_ms"] / rows[i]["hip_ms"]))
    print("\n".join(lines))
    for path, text in ((args.out, "\n".join(lines) + "\n"),
                       (args.json, json.dumps({"device": torch.cuda.get_device_name(0), "advect": rows}, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
