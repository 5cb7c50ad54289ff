"""Forward-backward consistency on the GPU: ops.flow_consistency (fs_flow_consistency{2,3}d) against the same measures
composed from stock torch ops on the same device in the same process (grid_sample with align_corners=True on a
normalised grid for the samples of flow_b and img1, fp32 element-wise ops, masked sums).  The stock form is the
comparator for speed only: its fp32 samples cannot reproduce the kernel's counts exactly.

Per case: `warmup` calls, then `reps` calls each between two HIP events; the table gives the median and the
10th / 90th percentile.  Bytes are the algorithm's compulsory traffic (ops.flow_consistency_cost: both flows and both
frames once, the maps if written), set against the 8 TB/s HBM peak (AMD's MI355X spec).

    python scripts/flowconsistbench.py [--out profiles/flow_consistency.txt] [--json flow_consistency.json]

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
CASE_LIMIT_S = 120


def torch_flow_consistency(ff, fb, img0, img1, alpha=(0.01, 0.5), maps=False):
    """The same measures from stock torch ops, fp32."""
    N, C = ff.shape[:2]
    sp = ff.shape[2:]
    ax = [torch.arange(s, device=ff.device, dtype=torch.float32) for s in sp]
    grid = torch.meshgrid(*ax, indexing="ij")[::-1]  # channel 0 along W
    p = [grid[c].unsqueeze(0) + ff[:, c] for c in range(C)]
    S = [sp[C - 1 - c] for c in range(C)]
    inside = torch.ones_like(p[0], dtype=torch.bool)
    for c in range(C):
        inside &= (p[c] >= 0) & (p[c] <= S[c] - 1)
    g = torch.stack([p[c] * (2.0 / max(S[c] - 1, 1)) - 1.0 for c in range(C)], -1)
    src = torch.cat([fb, img1.unsqueeze(1)], 1)
    smp = torch.nn.functional.grid_sample(src, g, mode="bilinear", padding_mode="border", align_corners=True)
    fbw, i1w = smp[:, :C], smp[:, C]
    r2 = ((ff + fbw) ** 2).sum(1)
    m2 = (ff ** 2).sum(1) + (fbw ** 2).sum(1)
    r = torch.sqrt(r2)
    occ = inside & (r2 > alpha[0] * m2 + alpha[1])
    noc = inside & ~occ
    e = (i1w - img0).abs()
    zero = r.new_zeros(())
    dims = tuple(range(1, r.dim()))
    n_in = torch.count_nonzero(inside, dims).double()
    n_noc = torch.count_nonzero(noc, dims).double()
    res = {"fb_mean": torch.where(inside, r, zero).sum(dims, dtype=torch.float64) / n_in,
           "fb_mean_noc": torch.where(noc, r, zero).sum(dims, dtype=torch.float64) / n_noc,
           "fb_max": torch.where(inside, r, zero).amax(dims),
           "occ_frac": torch.count_nonzero(occ, dims).double() / n_in,
           "out_frac": 1.0 - n_in / float(r[0].numel()),
           "warp_l1": torch.where(inside, e, zero).sum(dims, dtype=torch.float64) / n_in,
           "warp_l1_noc": torch.where(noc, e, zero).sum(dims, dtype=torch.float64) / n_noc,
           "warp_mse": torch.where(inside, e * e, zero).sum(dims, dtype=torch.float64) / n_in}
    if maps:
        res["class_map"] = torch.where(inside, torch.where(occ, 2, 1), 3).to(torch.uint8)
        res["res_map"] = torch.where(inside, r, r.new_full((), float("nan")))
    return res


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


def flows(shape, kind):
    N, C = shape[:2]
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    if kind == "smooth":  # the tests' mixed recipe: a near-constant flow and its negative, 40 % of flow_b perturbed
        const = (torch.rand((1, C) + (1,) * C, device="cuda", generator=g) * 1.6 - 0.8)
        ff = const + 0.15 * rnd(shape)
        fb = -const + 0.15 * rnd(shape)
        fb = fb + rnd(shape) * (torch.rand((N, 1) + tuple(shape[2:]), device="cuda", generator=g) < 0.4)
    else:  # white noise x 1.5 (the tests' noise kind): neighbouring lanes sample unrelated points a few elements apart
        ff, fb = 1.5 * rnd(shape), 1.5 * rnd(shape)
    sp = (N,) + tuple(shape[2:])
    return ff, fb, torch.rand(sp, device="cuda", generator=g), torch.rand(sp, device="cuda", generator=g)


def case(name, shape, kind, maps, warmup, reps):
    signal.alarm(CASE_LIMIT_S)
    ff, fb, img0, img1 = flows(shape, kind)
    nbytes, _ = ops.flow_consistency_cost(shape, True, maps)
    ms, lo, hi = timed(lambda: ops.flow_consistency(ff, fb, img0, img1, return_maps=maps), warmup, reps)
    ms_t, lo_t, hi_t = timed(lambda: torch_flow_consistency(ff, fb, img0, img1, maps=maps), warmup, reps)
    r = ops.flow_consistency(ff, fb, img0, img1)
    rt = torch_flow_consistency(ff, fb, img0, img1)
    signal.alarm(0)
    return {"case": name, "shape": list(shape), "flows": kind, "maps": maps, "reps": reps, "hip_ms": ms,
            "hip_ms_p10": lo, "hip_ms_p90": hi, "torch_ms": ms_t, "torch_ms_p10": lo_t, "torch_ms_p90": hi_t,
            "speedup_vs_torch": ms_t / ms, "algo_bytes": nbytes, "hip_GBps": nbytes / ms / 1e6,
            "share_of_hbm_roof": nbytes / HBM_BPS * 1e3 / ms,
            "fb_mean": float(r["fb_mean"].mean()), "occ_frac": float(r["occ_frac"].mean()),
            "out_frac": float(r["out_frac"].mean()),
            "max_rel_dfb_mean_vs_torch": float(((r["fb_mean"] - rt["fb_mean"]) / rt["fb_mean"]).abs().max()),
            "max_docc_frac_vs_torch": float((r["occ_frac"] - rt["occ_frac"]).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "flowconsistbench needs a GPU"
    assert args.reps >= 20
    rows = []
    for name, shape in (("3d 2 x 3 x 256^3", (2, 3, 256, 256, 256)), ("2d 32 x 2 x 150 x 450", (32, 2, 150, 450))):
        for kind in ("smooth", "noise"):
            for maps in (False, True):
                rows.append(case(name, shape, kind, maps, args.warmup, args.reps))
    lines = ["%s, %d repetitions after %d warm-up calls; median ms (p10 - p90); images given in every case" %
             (torch.cuda.get_device_name(0), args.reps, args.warmup),
             "%-22s %-6s %-4s %28s %9s %9s %30s %7s  %s" % ("case", "flows", "maps", "HIP ms", "GB/s", "of 8 TB/s",
                                                              "torch ms", "x", "fb_mean / occ / out   |d occ| vs torch")]
    for r in rows:
        lines.append("%-22s %-6s %-4s %8.3f (%8.3f - %8.3f) %9.0f %9.3f %9.3f (%8.3f - %8.3f) %7.1f  %.4f / %.4f / %.4f   %.1e"
                     % (r["case"], r["flows"], "yes" if r["maps"] else "no", r["hip_ms"], r["hip_ms_p10"],
                        r["hip_ms_p90"], r["hip_GBps"], r["share_of_hbm_roof"], r["torch_ms"], r["torch_ms_p10"],
                        r["torch_ms_p90"], r["speedup_vs_torch"], r["fb_mean"], r["occ_frac"], r["out_frac"],
                        r["max_docc_frac_vs_torch"]))
    print("\n".join(lines))
    for path, text in ((args.out, "\n".join(lines) + "\n"),
                       (args.json, json.dumps({"device": torch.cuda.get_device_name(0), "flow_consistency": rows},
                                              indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
