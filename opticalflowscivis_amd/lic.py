"""Line integral convolution: a dense picture of a series' estimated step flows.  Every node's grey value is a noise
texture averaged along the streamline of the step flow through that node (ops.lic: one launch per `--chunk` of steps,
both directions of every line), so the picture is correlated along the flow and uncorrelated across it.  Shared by the
flow2d / flow3d / upflow `lic` entry points:

    python -m opticalflowscivis_amd.flow2d.lic --dataset rectangle2d --png-dir shots --json r.json
    python -m opticalflowscivis_amd.flow3d.lic --flows flows.npy --length 16 --kernel hann --passes 2 --out lic.npy
    python -m opticalflowscivis_amd.upflow.lic --seq frames.npy --texture t.npy --out lic.npy --ends e.npy

The step flows are those of `trace` and `vortex` (stepflows.step_chain over the flows flow_eval extracts, or --flows);
each is taken as a steady field.  --out holds [K, *sp] fp32: it goes into the `render` entry points as --field as it is
(`flow3d.render --field lic.npy` ray-casts a 3-D LIC volume, `flow2d.render --field lic.npy` colour-maps a 2-D one);
--ends holds the end codes [K, *sp] uint8, the forward side's ops.LIC_* in bits 0-1 and the backward side's in bits
2-3 (of the last pass).  --passes 2 feeds a pass's output back as the per-step texture of the next, which sharpens the
lines.  The texture is white noise from --noise-seed (the same on every device) or --texture, [*sp] or [K, *sp].

Each chunk of step flows is estimated once, handed to one launch per pass and dropped: device memory is one chunk of
flows and of results.

Out of scope: output finer than the grid; RK4; unsteady streaklines, including the unsteady-flow variant of LIC;
contrast equalisation; modulating the grey value by speed (`render`'s transfer function on a `vortex` vmag plane does
that); autograd through the op."""
import argparse
import os
import time

import numpy as np
import torch

from . import ops, stepflows

_SIDES = ("full", "out", "stagnant", "nonfinite")  # ops.LIC_*


def lic_stats(out, ends, count):
    """One dict per step of ops.lic's results: mean_count, the share of each end code per side (ends_fwd / ends_bwd),
    min / mean / max of the finite outputs (None when there is none) and n_nonfinite.  Synchronises."""
    rows = []
    for k in range(out.shape[0]):
        o, e = out[k].reshape(-1), ends[k].reshape(-1).to(torch.int64)
        fin = torch.isfinite(o)
        nf = int(fin.sum())
        row = {"mean_count": float(count[k].to(torch.float64).mean())}
        for name, codes in (("ends_fwd", e & 3), ("ends_bwd", e >> 2)):
            share = torch.bincount(codes, minlength=4).to(torch.float64) / codes.numel()
            row[name] = {s: float(share[i]) for i, s in enumerate(_SIDES)}
        sel = o[fin].to(torch.float64)
        row.update(min=float(sel.min()) if nf else None, mean=float(sel.mean()) if nf else None,
                   max=float(sel.max()) if nf else None, n_nonfinite=o.numel() - nf)
        rows.append(row)
    return rows


def lic_series(step_flows, n_steps, sp, length=16, h=0.5, method="rk2", kernel="box", passes=1, vmin=0.0, texture=None,
               noise_seed=0, chunk=4, frames=None, keep_out=True, keep_ends=True, keep_flows=False, device="cuda"):
    """The LIC fields of the n_steps step flows that step_flows(j0, j1) -> [j1 - j0, C, *sp] hands out `chunk` at a
    time (each exactly once, one ops.lic launch per chunk and pass).  texture: [*sp] or [n_steps, *sp] (array or
    tensor), default ops.lic_noise(sp, noise_seed); from the second pass on a step's texture is its previous output.
    frames: the n_steps + 1 frames the chain visits (default 0..n_steps).

    Returns a dict: out (fp32 [n_steps, *sp]) and ends (uint8 [n_steps, *sp], of the last pass) in host memory (keep_out
    / keep_ends; keep_flows: flows, the step flows themselves), steps (one dict per step: step, t_from, t_to and
    lic_stats' numbers for the last pass) and the totals time_flows_s, time_kernel_s."""
    chunk, passes = max(1, int(chunk)), int(passes)
    if passes < 1:
        raise ValueError("passes must be >= 1, got %d" % passes)
    n_steps = int(n_steps)
    sp = tuple(int(s) for s in sp)
    nd = len(sp)
    frames = list(range(n_steps + 1)) if frames is None else list(frames)
    if len(frames) != n_steps + 1:
        raise ValueError("frames must name the %d frames the chain visits, got %d" % (n_steps + 1, len(frames)))
    if texture is None:
        texture = ops.lic_noise(sp, noise_seed, device)
    else:
        texture = torch.as_tensor(texture).to(device=device, dtype=torch.float32)
        if tuple(texture.shape) not in (sp, (n_steps,) + sp):
            raise ValueError("the texture must be %s or %s, got %s" % (sp, (n_steps,) + sp, tuple(texture.shape)))
    per_step = texture.dim() == nd + 1
    res = {}
    if keep_out:
        res["out"] = torch.empty((n_steps,) + sp, dtype=torch.float32)
    if keep_ends:
        res["ends"] = torch.empty((n_steps,) + sp, dtype=torch.uint8)
    if keep_flows:
        res["flows"] = torch.empty((n_steps, nd) + sp, dtype=torch.float32)
    rows = [{"step": j, "t_from": frames[j], "t_to": frames[j + 1]} for j in range(n_steps)]
    t_flows = t_kernel = 0.0
    for j0 in range(0, n_steps, chunk):
        j1 = min(n_steps, j0 + chunk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = step_flows(j0, j1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tex = texture[j0:j1] if per_step else texture
        for _ in range(passes):
            r = ops.lic(f, tex, length, h, method, kernel, vmin)
            tex = r["out"]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_flows += t1 - t0
        t_kernel += t2 - t1
        for j, row in zip(range(j0, j1), lic_stats(r["out"], r["ends"], r["count"])):
            rows[j].update(row)
        if keep_out:
            res["out"][j0:j1].copy_(r["out"])
        if keep_ends:
            res["ends"][j0:j1].copy_(r["ends"])
        if keep_flows:
            res["flows"][j0:j1].copy_(f)
        del f, r, tex
    res.update(steps=rows, time_flows_s=t_flows, time_kernel_s=t_kernel)
    return res


def _args(nd, desc, model):
    sp = ",".join("DHW"[3 - nd:])
    ap = argparse.ArgumentParser(description=desc)
    stepflows.add_source_args(ap, nd, model, direction="fwd: the flows t -> t+1; bwd: the model's own backward flows, from "
                              "the last frame down", chunk="step flows estimated at a time and handed to one launch per pass")
    ap.add_argument("--length", type=int, default=16, help="steps each way (0..%d)" % ops.LIC_MAX_L)
    ap.add_argument("--h", type=float, default=0.5, help="step length in elements")
    ap.add_argument("--method", choices=sorted(ops._LIC_METHODS), default="rk2", help="integrator of the unit direction field")
    ap.add_argument("--kernel", choices=ops._LIC_KERNELS, default="box", help="weights along the line")
    ap.add_argument("--passes", type=int, default=1, help="LIC passes: each takes the previous output as its texture")
    ap.add_argument("--vmin", type=float, default=0.0, help="a line ends where the speed is not above this")
    ap.add_argument("--noise-seed", type=int, default=0, help="seed of the generated white noise")
    ap.add_argument("--texture", default=None, metavar="T.npy", help="instead of generated noise: [%s] or [K,%s]" % (sp, sp))
    ap.add_argument("--out", default=None, metavar="LIC.npy", help="write the LIC fields [K,%s] (fp32) here; `render --field` reads them" % sp)
    ap.add_argument("--ends", default=None, metavar="E.npy", help="write the end codes [K,%s] (uint8) here" % sp)
    ap.add_argument("--save-flows", default=None, metavar="FLOWS.npy", help="write the step flows [K,%d,%s] here (--flows reads them)" % (nd, sp))
    if nd == 2:
        ap.add_argument("--png-dir", default=None, help="write one grey picture per step, lic_%%03d_to_%%03d.png, here")
    ap.set_defaults(nd=nd)
    return ap


def check_args(args):
    """What the parser cannot express."""
    stepflows.check_source_args(args)
    if not 0 <= args.length <= ops.LIC_MAX_L:
        raise SystemExit("--length must be in 0..%d" % ops.LIC_MAX_L)
    if not (0 < args.h < float("inf")):
        raise SystemExit("--h must be finite and > 0")
    if not (0 <= args.vmin < float("inf")):
        raise SystemExit("--vmin must be finite and >= 0")
    if args.passes < 1:
        raise SystemExit("--passes must be >= 1")
    return args


def run(args, nd, model, make_model):
    """The LIC fields of one parsed command line.  make_model() -> flows(frames, pairs) -> [2P, C, *sp]."""
    from . import render
    dev = torch.device("cuda")
    sf = stepflows.open_step_flows(args, nd, model, make_model, dev)
    name, sp, visited, K = sf.name, sf.sp, sf.visited, sf.n_steps
    texture = None
    if args.texture:
        texture = np.load(args.texture)
        if tuple(texture.shape) not in (tuple(sp), (K,) + tuple(sp)):
            raise SystemExit("--texture must be %s or %s, got %s" % (tuple(sp), (K,) + tuple(sp), texture.shape))
    png_dir = getattr(args, "png_dir", None)
    res = lic_series(sf.source, K, sp, args.length, args.h, args.method, args.kernel, args.passes, args.vmin, texture,
                     args.noise_seed, args.chunk, frames=visited or [0], keep_out=bool(args.out or png_dir),
                     keep_ends=bool(args.ends), keep_flows=bool(args.save_flows), device=dev)
    doc = {"sequence": name, "shape": list(sp), "model": None if args.flows else args.model, "direction": args.direction,
           "chunk": args.chunk, "gap": args.gap, "length": args.length, "h": args.h, "method": args.method,
           "kernel": args.kernel, "passes": args.passes, "vmin": args.vmin,
           "texture": args.texture or "noise:%d" % args.noise_seed, "frames": visited, "steps": res["steps"],
           "time_inference_s": res["time_flows_s"], "time_kernel_s": res["time_kernel_s"]}
    if not res["steps"]:
        print("%s: the chain has no step" % name)
    for w in res["steps"]:
        print("%s %s frames %d -> %d: mean count %.2f  full %.3f / %.3f  out %.3f / %.3f  stagnant %.3f / %.3f  "
              "nonfinite %d" % (name, args.direction, w["t_from"], w["t_to"], w["mean_count"], w["ends_fwd"]["full"],
                                w["ends_bwd"]["full"], w["ends_fwd"]["out"], w["ends_bwd"]["out"],
                                w["ends_fwd"]["stagnant"], w["ends_bwd"]["stagnant"], w["n_nonfinite"]))
    if res["steps"]:
        print("flows %.3f s  kernel %.4f s" % (res["time_flows_s"], res["time_kernel_s"]))
    if png_dir and res["steps"]:
        os.makedirs(png_dir, exist_ok=True)
        tf = render.tf_preset("grey")
        doc["pngs"] = []
        for j, w in enumerate(res["steps"]):
            lo, hi = (w["min"], w["max"]) if w["min"] is not None and w["max"] > w["min"] else (0.0, 1.0)
            rgba = render.colormap(res["out"][j], tf, lo, hi)
            path = os.path.join(png_dir, "lic_%03d_to_%03d.png" % (w["t_from"], w["t_to"]))
            render.write_png(path, render.to_uint8(rgba[..., 0].numpy()))
            doc["pngs"].append(path)
    stepflows.write_report(doc, args.json, {args.out: lambda: res["out"].numpy(), args.ends: lambda: res["ends"].numpy(),
                                            args.save_flows: lambda: res["flows"].numpy()})
    return doc


def main_rife(Model, nd, argv=None):
    """flow2d / flow3d: the steps m -> m+h (or back) of the final IFNet flows."""
    args = check_args(_args(nd, "Line integral convolution of the flows of a RIFE model", "rife").parse_args(argv))
    return run(args, nd, "rife", stepflows.rife_model(Model, args))


def main_upflow(make_net, argv=None):
    """upflow: the steps t -> t+gap through flow_f_out, or back through flow_b_out."""
    args = check_args(_args(2, "Line integral convolution of UPFlow's flows", "upflow").parse_args(argv))
    return run(args, 2, "upflow", stepflows.upflow_model(make_net, args))
