"""Vortex and divergence fields: the Eulerian quantities of a series' estimated step flows.  Every step flow is turned
into a velocity (displacement / the time the step spans), differentiated, and reduced on the device to divergence,
vorticity, the Q criterion and lambda2 (ops.velgrad: one launch per `--chunk` of steps).  Shared by the flow2d / flow3d
/ upflow `vortex` entry points:

    python -m opticalflowscivis_amd.flow3d.vortex --seq frames.npy --fields div,vmag,q,l2 --out vg.npy --mask m.npy --json r.json
    python -m opticalflowscivis_amd.flow2d.vortex --flows flows.npy --fields vort,q --spacing 0.5 1.0 --out vg.npy
    python -m opticalflowscivis_amd.upflow.vortex --dataset rectangle2d --json r.json

The step flows are those of `trace` (trace.step_chain over the flows flow_eval extracts, or --flows).  --out holds
[K, NP, *sp] fp32 with the selected fields' planes in the order div, vort (1 plane in 2-D, 3 in 3-D), vmag, q, l2, grad
(C * C planes, d u_r / d x_c at r * C + c); --mask holds the flags [K, *sp] uint8: bit 0 q > 0, bit 1 l2 < 0 (the two
vortex criteria), bit 7 a value was not finite (every plane is NaN there).  For data from incompressible simulations the
rms divergence of the report is a plausibility score of the estimated flow that needs no ground truth.

Each chunk of step flows is estimated once, handed to one launch and dropped: device memory is one chunk of flows and
of results.  A step's scale is 1 / (frames it spans * --dt); --spacing is the node spacing, one value or one per axis
((D,)H,W).

Connected regions of the flag maps, their sizes and strengths, and their tracks through the series are
opticalflowscivis_amd/regions.py (the `regions` entry points; --mask's file goes in there as it is).  Out of scope:
swirling strength and the Delta criterion; eigenvectors; vortex core lines; a validity mask; autograd through the op.
Pictures of --out: opticalflowscivis_amd/render.py (the `render` entry points take the file as --field, --plane picks the
field)."""
import argparse
import json
import os
import time

import numpy as np
import torch

from . import flow_eval, ops, trace


def step_scales(frames, dt):
    """1 / (frames spanned * dt) for every step of a chain that visits `frames`."""
    dt = float(dt)
    if not (0 < dt < float("inf")):
        raise ValueError("dt must be finite and positive, got %r" % (dt,))
    spans = [abs(b - a) for a, b in zip(frames[:-1], frames[1:])]
    if any(s == 0 for s in spans):
        raise ValueError("every step must span at least one frame, got the frames %r" % (list(frames),))
    return [1.0 / (s * dt) for s in spans]


def vortex_series(step_flows, n_steps, sp, fields=ops.VG_DEFAULT, spacing=1.0, chunk=4, frames=None, dt=1.0,
                  keep_out=True, keep_flags=True, keep_flows=False):
    """The velocity-gradient fields of the n_steps step flows that step_flows(j0, j1) -> [j1 - j0, C, *sp] hands out
    `chunk` at a time (each exactly once, one ops.velgrad launch per chunk).  frames: the n_steps + 1 frames the chain
    visits (default 0..n_steps); step j's scale is 1 / (frames it spans * dt).

    Returns a dict: planes (name -> slice of the NP planes), out (fp32 [n_steps, NP, *sp]) and flags (uint8
    [n_steps, *sp]) in host memory (keep_out / keep_flags; keep_flows: flows, the step flows themselves), steps (one
    dict per step: step, t_from, t_to, frames_spanned, scale and ops.velgrad_stats' numbers) and the totals
    time_flows_s, time_kernel_s."""
    chunk = max(1, int(chunk))
    n_steps = int(n_steps)
    sp = tuple(int(s) for s in sp)
    nd = len(sp)
    frames = list(range(n_steps + 1)) if frames is None else list(frames)
    if len(frames) != n_steps + 1:
        raise ValueError("frames must name the %d frames the chain visits, got %d" % (n_steps + 1, len(frames)))
    scales = step_scales(frames, dt)
    planes = ops.velgrad_planes(fields, nd)
    NP = max(s.stop for s in planes.values())
    nodes = int(np.prod(sp))
    res = {"planes": planes}
    if keep_out:
        res["out"] = torch.empty((n_steps, NP) + sp, dtype=torch.float32)
    if keep_flags:
        res["flags"] = torch.empty((n_steps,) + sp, dtype=torch.uint8)
    if keep_flows:
        res["flows"] = torch.empty((n_steps, nd) + sp, dtype=torch.float32)
    rows = [{"step": j, "t_from": frames[j], "t_to": frames[j + 1], "frames_spanned": abs(frames[j + 1] - frames[j]),
             "scale": scales[j]} for j in range(n_steps)]
    t_flows = t_kernel = 0.0
    for j0 in range(0, n_steps, chunk):
        j1 = min(n_steps, j0 + chunk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = step_flows(j0, j1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r = ops.velgrad(f, fields, spacing, scales[j0:j1], with_flags=True, summary=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_flows += t1 - t0
        t_kernel += t2 - t1
        for j, row in zip(range(j0, j1), ops.velgrad_stats(r["summary"], nodes)):
            rows[j].update(row)
        if keep_out:
            res["out"][j0:j1].copy_(r["out"])
        if keep_flags:
            res["flags"][j0:j1].copy_(r["flags"])
        if keep_flows:
            res["flows"][j0:j1].copy_(f)
        del f, r
    res.update(steps=rows, time_flows_s=t_flows, time_kernel_s=t_kernel)
    return res


def _args(nd, desc, model):
    sp = ",".join("DHW"[3 - nd:])
    ap = argparse.ArgumentParser(description=desc)
    ap.add_argument("--dataset", choices=flow_eval.DATASETS[nd], help="synthetic sequence with known motion")
    ap.add_argument("--seq", help=".npy sequence [T,%s] in [0,1]" % sp)
    ap.add_argument("--flows", metavar="PATH", help="skip the model: a [K,%d,%s] .npy of consecutive step flows, or a "
                    "directory of flow_%%03d_to_%%03d.npy files chained from --start" % (nd, sp))
    ap.add_argument("--start", type=int, default=0, help="first frame of a --flows chain")
    ap.add_argument("--frames", type=int, default=9, help="frames of a synthetic sequence")
    ap.add_argument("--size", type=int, nargs="+", default=None, help="synthetic extent (S, or H W in 2-D)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--gap", type=int, default=1 if model == "upflow" else 2,
                    help="the model runs on pairs (t, t+gap)" + ("" if model == "upflow" else ": a step spans gap / 2 frames"))
    ap.add_argument("--model", default="train_log", help="directory holding the weights")
    ap.add_argument("--batch", type=int, default=1, help="pairs per model call")
    ap.add_argument("--direction", choices=("fwd", "bwd"), default="fwd",
                    help="fwd: the flows t -> t+1; bwd: the model's own backward flows, from the last frame down")
    ap.add_argument("--chunk", type=int, default=4, help="step flows estimated at a time and handed to one launch")
    ap.add_argument("--fields", default=",".join(ops.VG_DEFAULT),
                    help="comma-separated, out of %s" % ",".join(ops.VG_FIELDS))
    ap.add_argument("--spacing", type=float, nargs="+", default=[1.0], help="node spacing: one value or one per axis (%s)" % sp)
    ap.add_argument("--dt", type=float, default=1.0, help="the time one frame spans: velocity = displacement / (frames spanned * dt)")
    ap.add_argument("--out", default=None, metavar="F.npy", help="write the planes [K, NP, %s] (fp32) here" % sp)
    ap.add_argument("--mask", default=None, metavar="M.npy", help="write the flags [K, %s] (uint8) here" % sp)
    ap.add_argument("--save-flows", default=None, metavar="FLOWS.npy", help="write the step flows [K, %d, %s] here (--flows reads them)" % (nd, sp))
    ap.add_argument("--json", default=None, help="write the report as JSON here")
    ap.set_defaults(nd=nd)
    return ap


def check_args(args):
    """What the parser cannot express."""
    if sum(x is not None for x in (args.dataset, args.seq, args.flows)) == 0:
        raise SystemExit("one of --dataset, --seq and --flows is needed")
    if args.dataset and args.seq:
        raise SystemExit("--dataset and --seq exclude each other")
    for name in ("chunk", "batch"):
        if getattr(args, name) < 1:
            raise SystemExit("--%s must be >= 1" % name)
    if args.start < 0:
        raise SystemExit("--start must be >= 0")
    if not (0 < args.dt < float("inf")):
        raise SystemExit("--dt must be finite and positive")
    if len(args.spacing) not in (1, args.nd) or not all(0 < h < float("inf") for h in args.spacing):
        raise SystemExit("--spacing takes one or %d finite positive values" % args.nd)
    try:
        ops.velgrad_planes(args.fields, args.nd)
    except ValueError as e:
        raise SystemExit("--fields: %s" % e)
    return args


def run(args, nd, model, make_model):
    """The fields of one parsed command line.  make_model() -> flows(frames, pairs) -> [2P, C, *sp]."""
    dev = torch.device("cuda")
    frames = None
    name = args.dataset or os.path.basename(args.seq or args.flows.rstrip("/"))
    if args.dataset:
        frames, _ = flow_eval.motion(args.dataset, args.frames, args.size, args.seed, dev)
    elif args.seq:
        frames = torch.from_numpy(np.load(args.seq).astype(np.float32)).to(dev)
        if frames.dim() != nd + 1:
            raise SystemExit("--seq must be [T,%s], got %s" % (",".join("DHW"[3 - nd:]), tuple(frames.shape)))
    if args.flows:
        visited, load, sp = trace._given_flows(args, nd)
        source = lambda j0, j1: torch.from_numpy(load(j0, j1)).to(dev)
    else:
        sp = tuple(int(s) for s in frames.shape[1:])
        chain = trace.step_chain(frames.shape[0], args.gap, args.direction, model)
        visited = ([chain[0][0]] + [c[1] for c in chain]) if chain else []
        if model == "rife":
            pairs = flow_eval.rife_pairs(frames.shape[0], args.gap)
        else:
            pairs = [(t, t + args.gap) for t in range(0, frames.shape[0] - args.gap)]
        flows_of = make_model() if chain else None

        def source(j0, j1):
            # the chain's flows of one direction share their parity in the model's (first, second) flow stack: the
            # strided view goes to the kernel as it is
            part = chain[j0:j1]
            stack = flows_of(frames, [pairs[c[2] // 2] for c in part])
            return stack[part[0][2] % 2::2]
    K = max(0, len(visited) - 1)
    spacing = args.spacing[0] if len(args.spacing) == 1 else tuple(args.spacing)
    res = vortex_series(source, K, sp, args.fields, spacing, args.chunk, frames=visited or [0], dt=args.dt,
                        keep_out=bool(args.out), keep_flags=bool(args.mask), keep_flows=bool(args.save_flows))
    planes = {n: [s.start, s.stop] for n, s in res["planes"].items()}
    doc = {"sequence": name, "shape": list(sp), "model": None if args.flows else args.model, "direction": args.direction,
           "chunk": args.chunk, "gap": args.gap, "fields": list(planes), "planes": planes, "spacing": list(args.spacing),
           "dt": args.dt, "frames": visited, "steps": res["steps"], "time_inference_s": res["time_flows_s"],
           "time_kernel_s": res["time_kernel_s"]}
    if not res["steps"]:
        print("%s: the chain has no step" % name)
    for w in res["steps"]:
        print("%s %s frames %d -> %d: rms div %.4g  enstrophy %.4g  q > 0 %.3f  l2 < 0 %.3f  both %.3f  nonfinite %d" % (
            name, args.direction, w["t_from"], w["t_to"], w["rms_div"], w["enstrophy"], w["frac_q_pos"],
            w["frac_l2_neg"], w["frac_both"], w["n_nonfinite"]))
    if res["steps"]:
        print("flows %.3f s  kernel %.4f s" % (res["time_flows_s"], res["time_kernel_s"]))
    for path in (args.out, args.mask, args.save_flows, args.json):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if args.out:
        np.save(args.out, res["out"].numpy())
    if args.mask:
        np.save(args.mask, res["flags"].numpy())
    if args.save_flows:
        np.save(args.save_flows, res["flows"].numpy())
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
    return doc


def main_rife(Model, nd, argv=None):
    """flow2d / flow3d: the steps m -> m+h (or back) of the final IFNet flows."""
    args = check_args(_args(nd, "Vortex and divergence fields of the flows of a RIFE model", "rife").parse_args(argv))

    def make_model():
        m = Model(-1, device=torch.device("cuda"))
        try:
            m.load_model("flownet.pkl", args.model)
        except FileNotFoundError:
            print("no flownet.pkl under %s: using random-init weights" % args.model)
        m.eval()
        return lambda frames, pairs: flow_eval.rife_flows(m, frames, pairs, args.batch)

    return run(args, nd, "rife", make_model)


def main_upflow(make_net, argv=None):
    """upflow: the steps t -> t+gap through flow_f_out, or back through flow_b_out."""
    args = check_args(_args(2, "Vortex and divergence fields of UPFlow's flows", "upflow").parse_args(argv))

    def make_model():
        net = make_net(args.model)
        return lambda frames, pairs: flow_eval.upflow_flows(net, frames, pairs, args.batch)

    return run(args, 2, "upflow", make_model)
