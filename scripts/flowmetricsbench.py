"""Flow accuracy on the GPU: ops.flow_metrics (fs_flow_metrics{2,3}d) against the same statistics as torch ops (fp32
element-wise math, fp64 reductions) on the same device.  Times are HIP events around `iters` calls after `warmup`
calls; bytes are the algorithm's compulsory traffic (ops.flow_metrics_cost: both flows, the masks, the map if written),
set against the 8 TB/s HBM peak (AMD's MI355X spec; ~6.3 TB/s is what a float4 copy reaches).

    python scripts/flowmetricsbench.py [--out profiles/flowmetricsbench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402

HBM_BPS = 8.0e12


def torch_flow_metrics(pred, gt, valid, noc, convention, tau=(3.0, 0.05)):
    """The same statistics as torch ops, written to be fast: fp32 element-wise math, masked values selected with
    torch.where and summed straight into fp64 accumulators (sum(dtype=float64) reads the fp32 values), counts by
    count_nonzero."""
    if convention == "rife3d":
        pred = ops.rife3d_to_disp(pred)
    d = pred - gt
    epe = torch.linalg.vector_norm(d, dim=1).flatten(1)
    gm = torch.linalg.vector_norm(gt, dim=1).flatten(1)
    C = pred.shape[1]
    cross = [pred[:, i] * gt[:, j] - pred[:, j] * gt[:, i] for i in range(C) for j in range(i + 1, C)]
    c2 = (d * d).sum(1) + sum(t * t for t in cross)
    ae = torch.atan2(torch.sqrt(c2), (pred * gt).sum(1) + 1).flatten(1)
    out = (epe > tau[0]) & (epe > tau[1] * gm)
    res = {}
    zero = epe.new_zeros(())
    for name, m in (("", valid.flatten(1)), ("_noc", (valid & noc).flatten(1))):
        n = torch.count_nonzero(m, 1).double()
        res["epe" + name] = torch.where(m, epe, zero).sum(1, dtype=torch.float64) / n
        res["fl" + name] = torch.count_nonzero(out & m, 1).double() / n
        if not name:
            res["rmse"] = torch.sqrt(torch.where(m, epe * epe, zero).sum(1, dtype=torch.float64) / n)
            res["ae_deg"] = torch.rad2deg(torch.where(m, ae, zero).sum(1, dtype=torch.float64) / n)
    return res


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


def case(name, shape, convention, warmup, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    gt = torch.randn(shape, device="cuda", generator=g) * 2
    pred = gt + torch.randn(shape, device="cuda", generator=g)
    sp = (shape[0],) + tuple(shape[2:])
    valid = torch.rand(sp, device="cuda", generator=g) < 0.9
    noc = torch.rand(sp, device="cuda", generator=g) < 0.7
    nbytes, _ = ops.flow_metrics_cost(shape, 2, False)
    ms = timed(lambda: ops.flow_metrics(pred, gt, valid, noc, convention), warmup, iters)
    ms_t = timed(lambda: torch_flow_metrics(pred, gt, valid, noc, convention), warmup, iters)
    r = ops.flow_metrics(pred, gt, valid, noc, convention)
    rt = torch_flow_metrics(pred, gt, valid, noc, convention)
    t_hbm = nbytes / HBM_BPS * 1e3
    return {"case": name, "shape": list(shape), "convention": convention, "hip_ms": ms, "torch_ms": ms_t,
            "speedup_vs_torch": ms_t / ms, "algo_bytes": nbytes, "hip_TBps": nbytes / ms / 1e9,
            "bound_hbm_ms": t_hbm, "share_of_hbm_roof": t_hbm / ms,
            "max_rel_depe_vs_torch": float(((r["epe"] - rt["epe"]) / rt["epe"]).abs().max()),
            "max_dfl_vs_torch": float((r["fl"] - rt["fl"]).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "flowmetricsbench needs a GPU"
    rows = [case("3d 2 x 3 x 256^3 disp", (2, 3, 256, 256, 256), "disp", args.warmup, args.iters),
            case("3d 2 x 3 x 256^3 rife3d", (2, 3, 256, 256, 256), "rife3d", args.warmup, args.iters),
            case("2d 64 x 2 x 150 x 450", (64, 2, 150, 450), "disp", args.warmup, args.iters),
            case("2d 64 x 2 x 160 x 224", (64, 2, 160, 224), "disp", args.warmup, args.iters)]
    for r in rows:
        print("%-26s HIP %7.3f ms  torch %8.3f ms  x%5.1f  %5.2f TB/s  %.2f of the 8 TB/s roof (%.3f ms)"
              "  |rel dEPE| vs torch %.1e" % (r["case"], r["hip_ms"], r["torch_ms"], r["speedup_vs_torch"],
                                               r["hip_TBps"], r["share_of_hbm_roof"], r["bound_hbm_ms"],
                                               r["max_rel_depe_vs_torch"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "flow_metrics": rows}, f, indent=1)


if __name__ == "__main__":
    main()
