"""Line integral convolution on the GPU: ops.lic (fs_lic{2,3}d, one launch for both sides of every line) against the
same picture composed from stock torch ops on the same device in the same process, in fp32: per step one grid_sample
(bilinear, align_corners=True, border padding) of the field per integrator stage, a normalisation, the position update,
one grid_sample of the texture and a masked accumulate.  The stock form is the comparator for speed only: its fp32
coordinates cannot reproduce the kernel's bits; the table gives the largest difference over the nodes whose two sides
ran to full length.

Per case: `warmup` calls of each, then `reps` rounds that time one HIP call and one torch call in turn, each between two
HIP events; the table gives the median and the 10th / 90th percentile.  Bytes and flops are the algorithm's
(ops.lic_cost, every line at full length), set against the 8 TB/s HBM peak and the 78.6 TFLOP/s fp64 vector peak (AMD's
MI355X spec); `Gsample/s` counts the field samples (2 L per node and integrator stage) and the texture samples
(2 L + 1) of full-length lines, `count` is the mean number of texture samples the lines really took.

    python scripts/licbench.py [--out profiles/lic.txt] [--json lic.json]
    FLOWSCI_HIP_LIBRARY=opticalflowscivis_amd/csrc/ablation/libflowsci_hip_ab.so python scripts/licbench.py --variants

--variants (ablation build only) times the kernel's four forms in turn within each round -- 64 consecutive x of a row
per wave or a compact 4 x 4 x 4 / 8 x 8 tile per wave, the field and texture planes as they are or a 16-byte
(v_x, v_y[, v_z], tex) element per node written by a streaming pre-pass that is part of the timed call (the product
is tiles, packed in 3-D and rows, packed in 2-D) -- and checks that all four give the same bits.

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
from opticalflowscivis_amd import _lib, ops  # noqa: E402
from advectbench import smooth_flows  # noqa: E402

HBM_BPS = 8.0e12
FP64_FLOPS = 78.6e12
CASE_LIMIT_S = 240
STAGES = {"euler": 1, "rk2": 2}
CASES = (("2048^2", (2048, 2048)), ("128^3", (128,) * 3), ("256^3", (256,) * 3))
VARIANTS = ((1, "rows, planes"), (2, "tiles, planes"), (3, "rows, packed"), (4, "tiles, packed"))  # FLOWSCI_LIC_VARIANT


def torch_lic(flows, tex, w, L, h, method="rk2"):
    """flows [1,C,*sp], tex [*sp], w: L + 1 floats -> (out [*sp], both sides at full length [*sp]) from stock ops in fp32."""
    C = flows.shape[1]
    sp = tuple(flows.shape[2:])
    dev = flows.device
    S = [sp[C - 1 - c] for c in range(C)]
    scale = torch.tensor([2.0 / max(s - 1, 1) for s in S], device=dev).view(C, 1)
    hi = torch.tensor([float(s - 1) for s in S], device=dev).view(C, 1)
    node = ops.grid_seeds(sp, 1, 0, dev)
    tex4 = tex.reshape((1, 1) + sp)

    def sample(img, q):
        g = (q * scale - 1.0).t().reshape((1,) + (1,) * (C - 1) + (q.shape[1], C))
        return torch.nn.functional.grid_sample(img, g, mode="bilinear", padding_mode="border",
                                               align_corners=True).reshape(img.shape[1], -1)

    def unit(q):
        v = sample(flows, q)
        return v / v.norm(dim=0, keepdim=True)

    acc = w[0] * tex.reshape(-1)
    wsum = torch.full_like(acc, w[0])
    full = torch.ones_like(acc, dtype=torch.bool)
    for s in (1.0, -1.0):
        p = node
        alive = torch.ones_like(full)
        for i in range(1, L + 1):
            d = unit(p)
            if method == "rk2":
                d = unit(p + (0.5 * s * h) * d)
            pn = p + (s * h) * d
            alive = alive & ((pn >= 0) & (pn <= hi)).all(0)  # (a NaN direction compares false)
            p = torch.where(alive, pn, p)
            m = alive.to(acc.dtype)
            acc = acc + (w[i] * m) * sample(tex4, p)[0]
            wsum = wsum + w[i] * m
        full = full & alive
    return (acc / wsum).reshape(sp), full.reshape(sp)


def timed(fns, warmup, reps):
    """[(median, p10, p90) ms] of every function of fns, timed in turn within each round."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(fns))] for _ in range(reps)]
    for row in ev:
        for i, f in enumerate(fns):
            row[2 * i].record()
            f()
            row[2 * i + 1].record()
    torch.cuda.synchronize()
    out = []
    for i in range(len(fns)):
        ms = sorted(e[2 * i].elapsed_time(e[2 * i + 1]) for e in ev)
        out.append((ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]))
    return out


def _operands(sp):
    return smooth_flows(1, sp), ops.lic_noise(sp, 0, "cuda")


def case(name, sp, L, h, method, warmup, reps):
    signal.alarm(CASE_LIMIT_S)
    flows, tex = _operands(sp)
    w = ops.lic_weights(L, "box", "cuda")
    wl = [1.0] * (L + 1)
    nodes = tex.numel()
    nbytes, flops = ops.lic_cost(sp, 1, L, method, shared_tex=True)
    (ms, lo, hi_), (ms_t, lo_t, hi_t) = timed([lambda: ops.lic(flows, tex, L, h, method, w),
                                               lambda: torch_lic(flows, tex, wl, L, h, method)], warmup, reps)
    r = ops.lic(flows, tex, L, h, method, w)
    ref, full_t = torch_lic(flows, tex, wl, L, h, method)
    full = (r["ends"][0] == 0) & full_t
    d = (r["out"][0] - ref).abs()[full]
    signal.alarm(0)
    samples = nodes * (2 * L * STAGES[method] + 2 * L + 1)
    return {"case": name, "shape": list(sp), "L": L, "h": h, "method": method, "reps": reps, "hip_ms": ms,
            "hip_ms_p10": lo, "hip_ms_p90": hi_, "torch_ms": ms_t, "torch_ms_p10": lo_t, "torch_ms_p90": hi_t,
            "speedup_vs_torch": ms_t / ms, "algo_bytes": nbytes, "algo_flops": flops,
            "share_of_hbm_roof": nbytes / HBM_BPS * 1e3 / ms, "share_of_fp64_roof": flops / FP64_FLOPS * 1e3 / ms,
            "samples_per_s": samples / ms * 1e3, "mean_count": float(r["count"].double().mean()),
            "full_frac": float(full.float().mean()), "max_abs_dout_vs_torch_full": float(d.max()) if d.numel() else float("nan")}


def variant_case(name, sp, L, h, method, warmup, reps):
    signal.alarm(CASE_LIMIT_S)
    flows, tex = _operands(sp)
    w = ops.lic_weights(L, "box", "cuda")

    def run(v):
        os.environ["FLOWSCI_LIC_VARIANT"] = str(v)  # read by the ablation build at every call
        return ops.lic(flows, tex, L, h, method, w)

    res = [run(v) for v, _ in VARIANTS]
    same = all(torch.equal(res[0][k].view(torch.uint8), r[k].view(torch.uint8)) for r in res[1:] for k in ("out", "ends", "count"))
    del res
    times = timed([(lambda v=v: run(v)) for v, _ in VARIANTS], warmup, reps)
    del os.environ["FLOWSCI_LIC_VARIANT"]
    signal.alarm(0)
    return {"case": name, "method": method, "same_bits": same,
            "variants": [{"variant": label, "ms": t[0], "ms_p10": t[1], "ms_p90": t[2]} for (_, label), t in zip(VARIANTS, times)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--h", type=float, default=0.5)
    ap.add_argument("--variants", action="store_true", help="the kernel's four forms against each other (ablation build)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "licbench needs a GPU"
    assert args.reps >= 20
    dev = torch.cuda.get_device_name(0)
    head = "%s, %d rounds (every form once per round, in turn) after %d warm-up calls; median ms (p10 - p90); K = 1, " \
           "L = %d, h = %g, box weights, band-limited flows" % (dev, args.reps, args.warmup, args.length, args.h)
    rows, lines = [], [head]
    if args.variants:
        assert _lib.ABLATION, "--variants needs FLOWSCI_HIP_LIBRARY=<the ablation build>"
        for name, sp in CASES:
            for method in ("euler", "rk2"):
                rows.append(variant_case(name, sp, args.length, args.h, method, args.warmup, args.reps))
        lines.append("%-8s %-6s %s  same bits" % ("case", "method", " ".join("%32s" % label for _, label in VARIANTS)))
        for r in rows:
            lines.append("%-8s %-6s %s  %s" % (r["case"], r["method"], " ".join(
                "%8.3f (%8.3f - %8.3f) ms" % (v["ms"], v["ms_p10"], v["ms_p90"]) for v in r["variants"]), r["same_bits"]))
    else:
        for name, sp in CASES:
            for method in ("euler", "rk2"):
                rows.append(case(name, sp, args.length, args.h, method, args.warmup, args.reps))
        lines.append("%-8s %-6s %28s %10s %9s %9s %6s %32s %7s  %s" % (
            "case", "method", "HIP ms", "Gsample/s", "of 8 TB/s", "of fp64", "count", "torch ms", "x",
            "full   max |d out| vs torch (full)"))
        for r in rows:
            lines.append("%-8s %-6s %8.3f (%8.3f - %8.3f) %10.1f %9.4f %9.3f %6.2f %10.3f (%9.3f - %9.3f) %7.1f  %.4f  %.1e" % (
                r["case"], r["method"], r["hip_ms"], r["hip_ms_p10"], r["hip_ms_p90"], r["samples_per_s"] / 1e9,
                r["share_of_hbm_roof"], r["share_of_fp64_roof"], r["mean_count"], r["torch_ms"], r["torch_ms_p10"],
                r["torch_ms_p90"], r["speedup_vs_torch"], r["full_frac"], r["max_abs_dout_vs_torch_full"]))
        for i in range(0, len(rows), 2):
            lines.append("%s: RK2 / Euler time %.2f (same bytes, %d against %d samples per node)" % (
                rows[i]["case"], rows[i + 1]["hip_ms"] / rows[i]["hip_ms"], 6 * args.length + 1, 4 * args.length + 1))
    print("\n".join(lines))
    for path, text in ((args.out, "\n".join(lines) + "\n"),
                       (args.json, json.dumps({"device": dev, "variants" if args.variants else "lic": rows}, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
