"""Velocity-gradient fields on the GPU: ops.velgrad (fs_velgrad{2,3}d: one launch for the planes and the flag map, one
more for the summary) against the same quantities composed from stock torch ops on the same device in the same process:
torch.gradient of every component along every axis in fp64 (central inside, one-sided at the border), S and Omega,
einsum for q and for M = S^2 + Omega^2, torch.linalg.eigvalsh for lambda2 (only where the field set asks for it), rounded
to fp32.  One step flow (a smooth displacement) on dense grids of 256^3, 128^3 and 2048^2 nodes, for the field sets
div,vort,q (no eigenvalues) and div,vmag,q,l2 (the default).

Per case: `warmup` calls of each, then `reps` rounds that time one HIP call and one torch call in turn, each between two
HIP events; the table gives the median and the 10th / 90th percentile.  Where one torch call takes seconds, only the first
rounds time it (column n: at least 3, as many as fit 20 s), the HIP call is timed in every round.  Bytes are the
algorithm's (ops.velgrad_cost: the C planes read once, the selected planes and the flag byte written), set against the
8 TB/s HBM peak (AMD's MI355X spec).  The run fails if a case is not faster than the stock composition timed beside it.

    python scripts/velgradbench.py [--out profiles/velgrad.txt] [--json velgrad.json]

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
CASE_LIMIT_S = 280
TORCH_BUDGET_S = 20.0


def torch_velgrad(flow, fields):
    """flow [C,*sp] fp32 -> {name: fp32 planes} from stock ops, spacing 1 and scale 1."""
    C = flow.shape[0]
    u = flow.double()
    # J[..., r, c]: component r along axis c; axis c is tensor dim C - 1 - c
    cols = [torch.stack([torch.gradient(u[r], dim=C - 1 - c)[0] for r in range(C)], -1) for c in range(C)]
    J = torch.stack(cols, -1)
    Jt = J.transpose(-1, -2)
    S, O = 0.5 * (J + Jt), 0.5 * (J - Jt)
    out = {}
    if "div" in fields:
        out["div"] = torch.einsum("...aa->...", J).float()
    if "vort" in fields or "vmag" in fields:
        w = (torch.stack([J[..., 2, 1] - J[..., 1, 2], J[..., 0, 2] - J[..., 2, 0], J[..., 1, 0] - J[..., 0, 1]]) if C == 3
             else (J[..., 1, 0] - J[..., 0, 1])[None])
        if "vort" in fields:
            out["vort"] = w.float()
        if "vmag" in fields:
            out["vmag"] = torch.linalg.vector_norm(w, dim=0).float()
    if "q" in fields:
        out["q"] = (0.5 * (torch.einsum("...ab,...ab->...", O, O) - torch.einsum("...ab,...ab->...", S, S))).float()
    if "l2" in fields:
        M = torch.einsum("...ab,...bc->...ac", S, S) + torch.einsum("...ab,...bc->...ac", O, O)
        ev = torch.linalg.eigvalsh(M)
        if C == 2:
            ev = torch.sort(torch.cat([ev, torch.zeros_like(ev[..., :1])], -1), -1)[0]
        out["l2"] = ev[..., 1].float()
    return out


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


def smooth_flow(sp, amp=0.8):
    """[1,C,*sp] fp32: a sine displacement of a few tens of elements' wavelength."""
    x = ops.grid_seeds(sp, 1, 0, "cuda").double()
    C = x.shape[0]
    g = torch.Generator(device="cuda").manual_seed(1)
    k = 0.05 + 0.1 * torch.rand((C, C), device="cuda", generator=g, dtype=torch.float64)
    ph = 6.28 * torch.rand((C, 1), device="cuda", generator=g, dtype=torch.float64)
    return (amp * torch.sin(k @ x + ph)).float().view((1, C) + tuple(sp)).contiguous()


def case(name, sp, fields, warmup, reps):
    signal.alarm(CASE_LIMIT_S)
    flows = smooth_flow(sp)
    names = fields.split(",")
    nbytes, flops = ops.velgrad_cost(sp, 1, fields)
    (ms, lo, hi), (ms_t, lo_t, hi_t), n = timed_pair(lambda: ops.velgrad(flows, fields),
                                                     lambda: torch_velgrad(flows[0], names), warmup, reps)
    got = ops.velgrad(flows, fields)
    ref = torch_velgrad(flows[0], names)
    d = max(float((got["out"][0, got["planes"][k]].reshape(ref[k].shape) - ref[k]).abs().max()) for k in names)
    st = ops.velgrad_stats(got["summary"], flows[0, 0].numel())[0]
    del ref
    signal.alarm(0)
    return {"case": name, "grid": list(sp), "fields": fields, "nodes": flows[0, 0].numel(), "reps": reps, "torch_reps": n,
            "hip_ms": ms, "hip_ms_p10": lo, "hip_ms_p90": hi, "torch_ms": ms_t, "torch_ms_p10": lo_t, "torch_ms_p90": hi_t,
            "speedup_vs_torch": ms_t / ms, "algo_bytes": nbytes, "algo_flops": flops, "hip_TBps": nbytes / ms / 1e9,
            "share_of_hbm_roof": nbytes / HBM_BPS * 1e3 / ms, "rms_div": st["rms_div"], "frac_q_pos": st["frac_q_pos"],
            "max_abs_diff_vs_torch": d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "velgradbench needs a GPU"
    assert args.reps >= 20
    rows = []
    for name, sp in (("256^3", (256,) * 3), ("128^3", (128,) * 3), ("2048^2", (2048,) * 2)):
        for fields in ("div,vort,q", ",".join(ops.VG_DEFAULT)):
            rows.append(case(name, sp, fields, args.warmup, args.reps))
            text = table(rows, args)
            print(text.splitlines()[-1], flush=True)
            for path, body in ((args.out, text),  # rewritten after every case: a case that overruns leaves the earlier rows
                               (args.json, json.dumps({"device": torch.cuda.get_device_name(0), "velgrad": rows}, indent=1))):
                if path:
                    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                    with open(path, "w") as f:
                        f.write(body)
    print(table(rows, args))
    slow = [(r["case"], r["fields"]) for r in rows if not r["hip_ms"] < r["torch_ms"]]
    assert not slow, "not faster than the stock composition: %r" % (slow,)


def table(rows, args):
    lines = ["%s, %d rounds (one HIP call, one torch call in turn; torch in the first n rounds) after %d warm-up calls; "
             "median ms (p10 - p90); two launches per HIP call (planes and flags, summary)" % (
                 torch.cuda.get_device_name(0), args.reps, args.warmup),
             "%-7s %-14s %28s %7s %7s %9s %34s %3s %8s  %s" % ("grid", "fields", "HIP ms", "GB", "TB/s", "of 8 TB/s",
                                                              "torch ms", "n", "x", "max |d| vs torch")]
    for r in rows:
        lines.append("%-7s %-14s %8.3f (%8.3f - %8.3f) %7.3f %7.3f %9.3f %10.3f (%10.3f - %10.3f) %3d %8.1f  %.1e"
                     % (r["case"], r["fields"], r["hip_ms"], r["hip_ms_p10"], r["hip_ms_p90"], r["algo_bytes"] / 1e9,
                        r["hip_TBps"], r["share_of_hbm_roof"], r["torch_ms"], r["torch_ms_p10"], r["torch_ms_p90"],
                        r["torch_reps"], r["speedup_vs_torch"], r["max_abs_diff_vs_torch"]))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
