"""FTLE on the GPU: ops.ftle (fs_ftle{2,3}d: one launch for the field and its class map, one more for the summary)
against the same computation composed from stock torch ops on the same device in the same process: torch.gradient of every
map component along every axis in fp64 (central inside, one-sided at the border), einsum to the Cauchy-Green tensor,
torch.linalg.eigvalsh, 0.5 log(lambda_max) / T, rounded to fp32.  The stock form knows no status, so the maps here are
all ALIVE: identity plus a smooth displacement on dense lattices of 128^3, 256^3 and 2048^2 nodes.

Per case: `warmup` calls of each, then `reps` rounds that time one HIP call and one torch call in turn, each between two
HIP events; the table gives the median and the 10th / 90th percentile.  Where one torch call takes seconds, only the first
rounds time it (column n: at least 3, as many as fit 20 s), the HIP call is timed in every round.  Bytes are the
algorithm's (ops.ftle_cost: the map planes and the status read once, exponent and class written), set against the
8 TB/s HBM peak (AMD's MI355X spec); flops are ops.ftle_cost's nominal count against the 78.6 TFLOP/s fp64 vector peak.

    python scripts/ftlebench.py [--out profiles/ftle.txt] [--json ftle.json]

One process, the cases one after another, each under its own time limit (SIGALRM): a case that overruns ends the run."""
import argparse
import json
import os
import signal
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402

HBM_BPS = 8.0e12
FP64_FLOPS = 78.6e12
CASE_LIMIT_S = 280
TORCH_BUDGET_S = 20.0


def torch_ftle(pos, lattice, spacing, T):
    """pos [C,P] fp32 -> ftle fp32 [*lattice] from stock ops; every node is taken as usable."""
    C = len(lattice)
    phi = pos.view((C,) + tuple(lattice)).double()
    # J[..., r, c]: component r along axis c; axis c is tensor dim C - 1 - c
    cols = []
    for c in range(C):
        cols.append(torch.stack([torch.gradient(phi[r], spacing=float(spacing), dim=C - 1 - c)[0] for r in range(C)], -1))
    J = torch.stack(cols, -1)
    G = torch.einsum("...ra,...rb->...ab", J, J)
    lam = torch.linalg.eigvalsh(G)[..., -1]
    return ((0.5 * torch.log(lam)) / abs(float(T))).float()


def pct(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


def timed_pair(fa, fb, warmup, reps):
    """(median, p10, p90) ms of fa over `reps` rounds and of fb over the first n of them, timed in turn; n."""
    fa()
    fb()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fb()
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    n = min(reps, max(3, int(TORCH_BUDGET_S / max(one, 1e-6))))
    for _ in range(warmup):
        fa()
        if one < 1.0:
            fb()
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
    return pct([e[0].elapsed_time(e[1]) for e in ev]), pct([e[2].elapsed_time(e[3]) for e in ev[:n]]), n


def smooth_map(lattice, amp=0.8):
    """[C,P] fp32: the identity plus a sine displacement of a few elements' wavelength."""
    seeds = ops.grid_seeds(lattice, 1, 0, "cuda").double()
    C = seeds.shape[0]
    g = torch.Generator(device="cuda").manual_seed(1)
    k = 0.05 + 0.1 * torch.rand((C, C), device="cuda", generator=g, dtype=torch.float64)
    ph = 6.28 * torch.rand((C, 1), device="cuda", generator=g, dtype=torch.float64)
    return (seeds + amp * torch.sin(k @ seeds + ph)).float().contiguous()


def case(name, lattice, warmup, reps):
    signal.alarm(CASE_LIMIT_S)
    pos = smooth_map(lattice)
    P = pos.shape[1]
    status = torch.zeros(P, dtype=torch.uint8, device="cuda")
    T = 4.0
    nbytes, flops = ops.ftle_cost(lattice)
    (ms, lo, hi), (ms_t, lo_t, hi_t), n = timed_pair(lambda: ops.ftle(pos, status, lattice, 1.0, T),
                                                     lambda: torch_ftle(pos, lattice, 1.0, T), warmup, reps)
    got = ops.ftle(pos, status, lattice, 1.0, T)
    ref = torch_ftle(pos, lattice, 1.0, T)
    stats = ops.ftle_stats(got["summary"])
    d = float((got["ftle"] - ref).abs().max())
    signal.alarm(0)
    return {"case": name, "lattice": list(lattice), "nodes": P, "reps": reps, "torch_reps": n, "hip_ms": ms,
            "hip_ms_p10": lo, "hip_ms_p90": hi, "torch_ms": ms_t, "torch_ms_p10": lo_t, "torch_ms_p90": hi_t,
            "speedup_vs_torch": ms_t / ms, "algo_bytes": nbytes, "algo_flops": flops, "hip_TBps": nbytes / ms / 1e9,
            "share_of_hbm_roof": nbytes / HBM_BPS * 1e3 / ms, "share_of_fp64_roof": flops / FP64_FLOPS * 1e3 / ms,
            "ok_frac": stats["counts"]["ok"] / P, "ftle_mean": stats["mean"], "ftle_max": stats["max"],
            "max_abs_diff_vs_torch": d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ftlebench needs a GPU"
    assert args.reps >= 20
    rows = []
    for name, lattice in (("dense 128^3", (128,) * 3), ("dense 256^3", (256,) * 3), ("dense 2048^2", (2048,) * 2)):
        rows.append(case(name, lattice, args.warmup, args.reps))
        text = table(rows, args)
        print(text.splitlines()[-1], flush=True)
        for path, body in ((args.out, text),  # rewritten after every case: a case that overruns leaves the earlier rows
                           (args.json, json.dumps({"device": torch.cuda.get_device_name(0), "ftle": rows}, indent=1))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
    print(table(rows, args))


def table(rows, args):
    lines = ["%s, %d rounds (one HIP call, one torch call in turn; torch in the first n rounds) after %d warm-up calls; "
             "median ms (p10 - p90); two launches per HIP call (field, summary)" % (
                 torch.cuda.get_device_name(0), args.reps, args.warmup),
             "%-14s %28s %7s %9s %9s %34s %3s %8s  %s" % ("case", "HIP ms", "TB/s", "of 8 TB/s", "of fp64", "torch ms", "n",
                                                        "x", "ok      max |d ftle| vs torch")]
    for r in rows:
        lines.append("%-14s %8.3f (%8.3f - %8.3f) %7.3f %9.3f %9.3f %10.3f (%10.3f - %10.3f) %3d %8.1f  %.4f  %.1e"
                     % (r["case"], r["hip_ms"], r["hip_ms_p10"], r["hip_ms_p90"], r["hip_TBps"], r["share_of_hbm_roof"],
                        r["share_of_fp64_roof"], r["torch_ms"], r["torch_ms_p10"], r["torch_ms_p90"], r["torch_reps"],
                        r["speedup_vs_torch"], r["ok_frac"], r["max_abs_diff_vs_torch"]))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
