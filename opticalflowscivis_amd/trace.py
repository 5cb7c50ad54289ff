"""Pathlines: follow seeded particles through the flows a model estimates on a time series (ops.advect: one launch
moves every particle through a chunk of consecutive step flows).  Shared by the flow2d / flow3d / upflow `trace`
entry points:

    python -m opticalflowscivis_amd.flow3d.trace --seq frames.npy --seed-grid 4 --out traj.npy --json r.json
    python -m opticalflowscivis_amd.flow3d.trace --dataset droplet3d --size 64 --seed-grid 1 --map-out map.npy
    python -m opticalflowscivis_amd.flow2d.trace --flows flows/ --start 1 --seeds seeds.npy --method rk4 --out traj.npy
    python -m opticalflowscivis_amd.upflow.trace --dataset rectangle2d --direction bwd --seed-grid 8 --json r.json

The step flows come from the flows flow_eval already extracts (stepflows.step_chain is pure index arithmetic over them;
opticalflowscivis_amd/stepflows.py opens them for this tool, `ftle`, `vortex` and `regions` alike, and says which
frames a RIFE and a UPFlow chain visit).  Tracing backward uses the model's own backward flows with scale +1, not
negated forward ones.  --flows skips the model: a [K,C,*sp] .npy of consecutive step flows, or a directory of
flow_%03d_to_%03d.npy files as --save-flows writes them, chained from --start.

Positions are (x, y[, z]) in elements (x along W), kept as fp32 and advanced in fp64; a particle ends when it leaves the
box (status 1, it keeps its exit point), or meets a non-finite value (status 2, it keeps its last finite position);
status 0 is alive.  The flows of `--chunk` steps are estimated at a time and consumed by one launch, so device memory
does not grow with the number of frames (the recorded trajectories aside); chunking does not change a bit of the result.
With a known motion (--dataset or --gt) the same seeds are also advected through gt(m_j, m_j+1) by the same kernel and
the report gains the per-step drift between the two trajectories: what the per-pair errors add up to (--map-out
without --out records nothing per step: the drift after the last step only).

FTLE fields, the derivative of the flow map reduced to Lyapunov exponents, are opticalflowscivis_amd/ftle.py (the `ftle`
entry points).  Out of scope: batches of several series in one launch; interleaved ([*sp, C]) flow layouts; autograd
through the op."""
import argparse
import time

import numpy as np
import torch

from . import flow_eval, ops, stepflows


def trace_series(step_flows, n_steps, seeds, chunk=4, method="euler", substeps=1, scale=1.0, record=True):
    """Advect `seeds` [C,P] through the n_steps step flows that step_flows(j0, j1) -> [j1 - j0, C, *sp] hands out
    `chunk` at a time, one ops.advect launch per chunk.  Returns a dict: traj ([n_steps + 1, C, P], or None without
    record), pos [C,P] (the last positions), status, steps, time_flows_s, time_advect_s."""
    chunk = max(1, int(chunk))
    C, P = seeds.shape
    dev = seeds.device
    pos = seeds.to(torch.float32)
    traj = None
    if record:
        traj = torch.empty(n_steps + 1, C, P, dtype=torch.float32, device=dev)
        traj[0].copy_(pos)
    status = steps = None
    t_flows = t_adv = 0.0
    for j0 in range(0, n_steps, chunk):
        j1 = min(n_steps, j0 + chunk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = step_flows(j0, j1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out, status, steps = ops.advect(pos, f, status, steps, method, substeps, scale, record=record)
        if record:
            traj[j0 + 1:j1 + 1].copy_(out[1:])
            pos = traj[j1]
        else:
            pos = out
        torch.cuda.synchronize()
        t_flows += t1 - t0
        t_adv += time.perf_counter() - t1
    if status is None:  # no step at all
        status = torch.zeros(P, dtype=torch.uint8, device=dev)
        steps = torch.zeros(P, dtype=torch.int32, device=dev)
    return {"traj": traj, "pos": pos, "status": status, "steps": steps, "time_flows_s": t_flows,
            "time_advect_s": t_adv}


def step_counts(status, steps, n_steps):
    """Per step j (after step j + 1 steps were taken) the (alive, out, nonfinite) counts, from the final status and the
    per-particle count of steps survived: a particle is alive after step j when steps > j and has ended, in the class
    its final status names, otherwise."""
    st, n = status.cpu().numpy(), steps.cpu().numpy()
    rows = []
    for j in range(n_steps):
        ended = n <= j
        rows.append((int((~ended).sum()), int((ended & (st == ops.ADV_OUT)).sum()),
                     int((ended & (st == ops.ADV_NONFINITE)).sum())))
    return rows


def drift(a, b, frames):
    """Per step the mean and maximum distance between the trajectories of two trace_series results over the particles
    alive in both after that step (with unrecorded trajectories: after the last step only)."""
    K = len(frames) - 1
    rows = []
    for j in (range(1, K + 1) if a["traj"] is not None and b["traj"] is not None else [K] if K else []):
        pa = a["traj"][j] if a["traj"] is not None else a["pos"]
        pb = b["traj"][j] if b["traj"] is not None else b["pos"]
        both = (a["steps"] >= j) & (b["steps"] >= j)
        d = torch.sqrt(((pa.double() - pb.double()) ** 2).sum(0))[both]
        n = int(d.numel())
        rows.append({"step": j, "t": frames[j], "n": n, "mean": float(d.mean()) if n else float("nan"),
                     "max": float(d.max()) if n else float("nan")})
    return rows


def _args(nd, desc, model):
    sp = ",".join("DHW"[3 - nd:])
    ap = argparse.ArgumentParser(description=desc)
    stepflows.add_source_args(ap, nd, model, direction="trace forward or backward in time",
                              chunk="step flows estimated at a time and advected in one launch")
    ap.add_argument("--gt", help=".npy per-frame velocities [T,%d,%s]: also trace the known motion, report the drift" % (nd, sp))
    seeds = ap.add_mutually_exclusive_group(required=True)
    seeds.add_argument("--seeds", metavar="FILE", help=".npy seed positions [P,%d] as (x, y%s), in elements" % (nd, ", z" if nd == 3 else ""))
    seeds.add_argument("--seed-grid", type=int, metavar="STRIDE", help="seed every STRIDE-th element (1: the dense flow map)")
    ap.add_argument("--method", choices=sorted(ops._ADV_METHODS), default="euler")
    ap.add_argument("--substeps", type=int, default=1)
    ap.add_argument("--out", default=None, metavar="TRAJ.npy", help="write the trajectories [K+1,P,%d] (fp32) here" % nd)
    ap.add_argument("--map-out", default=None, metavar="MAP.npy",
                    help="write last position minus seed as a displacement [%d,%s] (needs --seed-grid 1)" % (nd, sp))
    return ap


def check_args(args):
    """What the parser cannot express."""
    stepflows.check_source_args(args)
    if args.dataset and args.gt:
        raise SystemExit("--gt goes with --seq or --flows: a --dataset carries its own known motion")
    if args.map_out and args.seed_grid != 1:
        raise SystemExit("--map-out needs --seed-grid 1 (one particle per element)")
    if args.seed_grid is not None and args.seed_grid < 1:
        raise SystemExit("--seed-grid must be >= 1")
    if args.substeps < 1:
        raise SystemExit("--substeps must be >= 1")
    return args


def run(args, nd, model, make_model):
    """The trace of one parsed command line.  make_model() -> flows(frames, pairs) -> [2P, C, *sp]."""
    dev = torch.device("cuda")
    sf = stepflows.open_step_flows(args, nd, model, make_model, dev)
    name, gt, sp, visited, K = sf.name, sf.gt, sf.sp, sf.visited, sf.n_steps
    if args.gt:
        vel = torch.from_numpy(np.load(args.gt).astype(np.float32)).to(dev)
        if vel.dim() != nd + 2 or tuple(vel.shape[1:]) != (nd,) + sp or (visited and vel.shape[0] <= max(visited[:-1] or [0])):
            raise SystemExit("--gt must be [T,%d,%s] with the traced extent %s and a frame for every step, got %s" % (
                nd, ",".join("DHW"[3 - nd:]), sp, tuple(vel.shape)))
        gt = flow_eval.velocity_gt(vel)
    if args.seeds:
        s = np.load(args.seeds)
        if s.ndim != 2 or s.shape[1] != nd:
            raise SystemExit("--seeds must be [P,%d], got %s" % (nd, s.shape))
        seeds = torch.from_numpy(np.ascontiguousarray(s.astype(np.float32).T)).to(dev)
    else:
        seeds = ops.grid_seeds(sp, args.seed_grid, 0, dev)
    record = args.out is not None or (gt is not None and not args.map_out)
    kw = dict(chunk=args.chunk, method=args.method, substeps=args.substeps, record=record)
    res = trace_series(sf.source, K, seeds, **kw)
    doc = {"sequence": name, "shape": list(sp), "model": None if args.flows else args.model, "direction": args.direction,
           "method": args.method, "substeps": args.substeps, "chunk": args.chunk, "gap": args.gap,
           "frames": visited, "n_particles": int(seeds.shape[1]),
           "steps": [{"step": j + 1, "t_from": visited[j], "t_to": visited[j + 1], "alive": c[0], "out": c[1],
                      "nonfinite": c[2]} for j, c in enumerate(step_counts(res["status"], res["steps"], K))],
           "time_inference_s": res["time_flows_s"], "time_advect_s": res["time_advect_s"]}
    if gt is not None and K:
        ref = trace_series(lambda j0, j1: torch.stack([gt(visited[j], visited[j + 1])[0] for j in range(j0, j1)]).float(),
                           K, seeds, **kw)
        doc["drift"] = {"steps": drift(res, ref, visited), "time_advect_s": ref["time_advect_s"]}
    if not K:
        print("%s: the series is too short for a step of the chain (gap %d)" % (name, args.gap))
    else:
        last = doc["steps"][-1]
        line = "%s %s %s x%d: %d particles through frames %s: alive %d  out %d  nonfinite %d" % (
            name, args.direction, args.method, args.substeps, doc["n_particles"],
            "%d..%d" % (visited[0], visited[-1]), last["alive"], last["out"], last["nonfinite"])
        if "drift" in doc and doc["drift"]["steps"]:
            d = doc["drift"]["steps"][-1]
            line += "  | drift mean %.4f max %.4f over %d" % (d["mean"], d["max"], d["n"])
        print(line + "  | flows %.3f s  advection %.4f s" % (res["time_flows_s"], res["time_advect_s"]))
    stepflows.write_report(doc, args.json, {
        args.out: lambda: res["traj"].permute(0, 2, 1).contiguous().cpu().numpy(),
        args.map_out: lambda: (res["pos"] - seeds).view((nd,) + sp).cpu().numpy()})
    return doc


def main_rife(Model, nd, argv=None):
    """flow2d / flow3d: the steps m -> m+h (or back) of the final IFNet flows."""
    args = check_args(_args(nd, "trace particles through the flows of a RIFE model", "rife").parse_args(argv))
    return run(args, nd, "rife", stepflows.rife_model(Model, args))


def main_upflow(make_net, argv=None):
    """upflow: the steps t -> t+gap through flow_f_out, or back through flow_b_out."""
    args = check_args(_args(2, "trace particles through UPFlow's flows", "upflow").parse_args(argv))
    return run(args, 2, "upflow", stepflows.upflow_model(make_net, args))
