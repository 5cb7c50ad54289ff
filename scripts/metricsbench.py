"""Per-frame PSNR / SSIM on the GPU: ops.frame_metrics (fs_frame_metrics{2,3}d) against a torch composition of the
same metric (separable grouped F.conv passes and elementwise ops, fp32) on the same device, plus one end-to-end
`flow3d.evaluate` run.  Times are HIP events around `iters` calls after `warmup` calls; bytes and flops are the
algorithm's, computed from shapes (ops.frame_metrics_cost).  Bounds: 8 TB/s HBM; the kernels filter in fp64, so the
VALU bound takes the flops at the fp64 vector peak (78.6 TFLOP/s, AMD's MI355X spec; 157.3 for fp32).

    python scripts/metricsbench.py [--out profiles/metricsbench.json] [--no-evaluate]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402

HBM_BPS, VALU_FLOPS = 8.0e12, 78.6e12


def torch_metrics(x, y, L, nd):
    """The same metric as torch ops: five maps through 11-tap grouped convolutions along each axis."""
    i = torch.arange(11, dtype=torch.float64, device=x.device)
    g = torch.exp(-((i - 5) ** 2) / 4.5)
    g = (g / g.sum()).float()
    N, C = x.shape[:2]
    maps = torch.cat([x, y, x * x, y * y, x * y], 1)
    conv = F.conv2d if nd == 2 else F.conv3d
    for ax in range(nd):
        shape = [1] * nd
        shape[ax] = 11
        maps = conv(maps, g.view(1, 1, *shape).expand(5 * C, 1, *shape), groups=5 * C)
    mx, my, exx, eyy, exy = maps.split(C, 1)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    s = ((2 * mx * my + c1) * (2 * (exy - mx * my) + c2)) / ((mx * mx + my * my + c1) * (exx - mx * mx + eyy - my * my + c2))
    mse = ((x.double() - y.double()) ** 2).flatten(1).mean(1)
    return 10 * torch.log10(L * L / mse), s.flatten(1).double().mean(1)


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


def case(name, shape, window, warmup, iters):
    nd = 2 if window == "2d" else 3
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(shape, device="cuda", generator=g)
    y = (x + 0.05 * torch.rand(shape, device="cuda", generator=g)).clamp(0, 1)
    nbytes, flops = ops.frame_metrics_cost(shape, window)
    ms = timed(lambda: ops.frame_metrics(x, y, 1.0, window), warmup, iters)
    ms_t = timed(lambda: torch_metrics(x, y, 1.0, nd), warmup, iters)
    p, s = ops.frame_metrics(x, y, 1.0, window)
    pt, st = torch_metrics(x, y, 1.0, nd)
    t_hbm, t_valu = nbytes / HBM_BPS * 1e3, flops / VALU_FLOPS * 1e3
    return {"case": name, "shape": list(shape), "window": window, "hip_ms": ms, "torch_ms": ms_t,
            "speedup_vs_torch": ms_t / ms, "algo_bytes": nbytes, "algo_flops": flops,
            "hip_GBps": nbytes / ms / 1e6, "hip_TFLOPs": flops / ms / 1e9,
            "bound_hbm_ms": t_hbm, "bound_valu_ms": t_valu,
            "share_of_bound": max(t_hbm, t_valu) / ms, "bound": "VALU" if t_valu > t_hbm else "HBM",
            "max_dssim_vs_torch": float((s - st).abs().max()), "max_dpsnr_vs_torch": float((p - pt).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-evaluate", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metricsbench needs a GPU"
    rows = [case("3d 2 x 256^3", (2, 1, 256, 256, 256), "3d", args.warmup, args.iters),
            case("2d 64 x 1 x 160 x 224", (64, 1, 160, 224), "2d", args.warmup, args.iters),
            case("2d 64 x 3 x 160 x 224", (64, 3, 160, 224), "2d", args.warmup, args.iters)]
    for r in rows:
        print("%-24s HIP %8.3f ms  torch %8.3f ms  x%.1f  %7.1f GB/s  %6.1f TFLOP/s  %.2f of the %s bound (%.3f ms)"
              "  |dSSIM| vs torch %.1e" % (r["case"], r["hip_ms"], r["torch_ms"], r["speedup_vs_torch"], r["hip_GBps"],
                                            r["hip_TFLOPs"], r["share_of_bound"], r["bound"],
                                            max(r["bound_hbm_ms"], r["bound_valu_ms"]), r["max_dssim_vs_torch"]))
    doc = {"device": torch.cuda.get_device_name(0), "frame_metrics": rows}
    if not args.no_evaluate:
        from opticalflowscivis_amd.evaluate import main as evaluate_main
        from opticalflowscivis_amd.flow3d.model.RIFE import Model
        torch.manual_seed(0)
        t0 = time.perf_counter()
        ev = evaluate_main(Model, 3, ["--dataset", "jets3d", "--size", "128", "--frames", "17", "--exp", "1", "2", "3",
                                      "--baseline", "--model", os.path.join(ROOT, "nonexistent_model_dir")])
        doc["evaluate_jets3d_128_17_frames"] = {"wall_s": time.perf_counter() - t0, "results": [
            {k: r[k] for k in ("factor", "time_inference_s", "time_metrics_s", "threshold", "selected")} |
            {"psnr_mean": r["model"]["psnr_mean"], "ssim_mean": r["model"]["ssim_mean"],
             "baseline_psnr_mean": r["baseline"]["psnr_mean"], "baseline_ssim_mean": r["baseline"]["ssim_mean"]}
            for r in ev["results"]]}
        print("flow3d.evaluate jets3d 128^3 x 17, exp 1 2 3: %.2f s" % doc["evaluate_jets3d_128_17_frames"]["wall_s"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
