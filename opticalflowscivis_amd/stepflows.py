"""The step flows of a series: what the `trace`, `ftle`, `vortex` and `regions` tools walk.  One place for the chain
arithmetic (step_chain, chain_flow_files, step_scales), the source options of their command lines and the checks on
them, the opening of a parsed command line into `source(j0, j1)` (open_step_flows), the two model factories and the
writing of a report with its arrays.  Imports without a GPU; the device is a parameter.

A RIFE model run on the pairs (t, t+g), g = 2h, yields flows that start at each pair's mid frame, so the chain visits the
frames h, 2h, 3h, ... for which both rife_consistency_pairs flows exist: forward in time through the flows m -> m+h
(F_mid->1 of pair m-h, on frame m's grid), backward through m+h -> m (F_mid->0 of pair m, on frame m+h's grid).  UPFlow
gives t -> t+g and t+g -> t directly.  A backward chain therefore uses the model's own backward flows, not negated forward
ones.  --flows skips the model: a [K,C,*sp] .npy of consecutive step flows, or a directory of flow_%03d_to_%03d.npy files
as --save-flows writes them, chained from --start."""
import collections
import json
import os
import re

import numpy as np
import torch

from . import flow_eval
from .rife import load_pretrained


def step_chain(T, gap, direction="fwd", model="rife"):
    """[(t_from, t_to, index)] of the consecutive steps a trace takes through a series of T frames; `index` is the row
    of the step's flow in the [2P, C, *sp] stack that flow_eval.rife_flows gives for rife_pairs(T, gap) (model="rife":
    pair index // 2, flow index % 2) or flow_eval.upflow_flows for the pairs (t, t+gap) (model="upflow").  Forward:
    ascending frames; backward: the same frames from the last one down, through the opposite flows.  Empty when the
    series is too short."""
    if direction not in ("fwd", "bwd"):
        raise ValueError("direction must be 'fwd' or 'bwd', got %r" % (direction,))
    if model == "rife":
        by_start = {a: (b, i_f, i_b) for a, b, i_f, i_b in flow_eval.rife_consistency_pairs(T, gap)}
        m = gap // 2
    elif model == "upflow":
        if gap < 1:
            raise ValueError("gap must be >= 1, got %d" % gap)
        by_start = {t: (t + gap, 2 * i, 2 * i + 1) for i, t in enumerate(range(0, T - gap))}
        m = 0
    else:
        raise ValueError("model must be 'rife' or 'upflow', got %r" % (model,))
    fwd, bwd = [], []
    while m in by_start:
        b, i_f, i_b = by_start[m]
        fwd.append((m, b, i_f))
        bwd.append((b, m, i_b))
        m = b
    return fwd if direction == "fwd" else bwd[::-1]


_FLOW_FILE = re.compile(r"^flow_(\d+)_to_(\d+)\.npy$")


def chain_flow_files(dirname, start, direction="fwd"):
    """[(t_from, t_to, path)]: the flow_%03d_to_%03d.npy files of `dirname` chained from frame `start`: from each frame
    the file that leads to the nearest later (fwd) / earlier (bwd) frame, until none does."""
    if direction not in ("fwd", "bwd"):
        raise ValueError("direction must be 'fwd' or 'bwd', got %r" % (direction,))
    nxt = {}
    for name in sorted(os.listdir(dirname)):
        m = _FLOW_FILE.match(name)
        if not m:
            continue
        a, b = int(m.group(1)), int(m.group(2))
        if (b > a) != (direction == "fwd") or a == b:
            continue
        if a not in nxt or abs(b - a) < abs(nxt[a][0] - a):
            nxt[a] = (b, os.path.join(dirname, name))
    chain, t = [], int(start)
    while t in nxt:
        b, path = nxt[t]
        chain.append((t, b, path))
        t = b
    return chain


def step_scales(frames, dt):
    """1 / (frames spanned * dt) for every step of a chain that visits `frames`."""
    dt = float(dt)
    if not (0 < dt < float("inf")):
        raise ValueError("dt must be finite and positive, got %r" % (dt,))
    spans = [abs(b - a) for a, b in zip(frames[:-1], frames[1:])]
    if any(s == 0 for s in spans):
        raise ValueError("every step must span at least one frame, got the frames %r" % (list(frames),))
    return [1.0 / (s * dt) for s in spans]


def add_source_args(ap, nd, model, direction, chunk, dt=None, spacing=False):
    """The options that name a series' step flows, and --json.  model ("rife" / "upflow") sets --gap's default and help;
    direction and chunk are the tool's help strings for --direction and --chunk; dt: the help string of --dt, for a tool
    that has one; spacing: the tool takes --spacing."""
    sp = ",".join("DHW"[3 - nd:])
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
    ap.add_argument("--direction", choices=("fwd", "bwd"), default="fwd", help=direction)
    ap.add_argument("--chunk", type=int, default=4, help=chunk)
    if dt is not None:
        ap.add_argument("--dt", type=float, default=1.0, help=dt)
    if spacing:
        ap.add_argument("--spacing", type=float, nargs="+", default=[1.0], help="node spacing: one value or one per axis (%s)" % sp)
        ap.set_defaults(nd=nd)
    ap.add_argument("--json", default=None, help="write the report as JSON here")
    return ap


def check_source_args(args):
    """What the parser cannot express about the options of add_source_args."""
    if sum(x is not None for x in (args.dataset, args.seq, args.flows)) == 0:
        raise SystemExit("one of --dataset, --seq and --flows is needed")
    if args.dataset and args.seq:
        raise SystemExit("--dataset and --seq exclude each other")
    for name in ("chunk", "batch"):
        if getattr(args, name) < 1:
            raise SystemExit("--%s must be >= 1" % name)
    if args.start < 0:
        raise SystemExit("--start must be >= 0")
    if hasattr(args, "dt") and not (0 < args.dt < float("inf")):
        raise SystemExit("--dt must be finite and positive")
    if hasattr(args, "spacing") and (len(args.spacing) not in (1, args.nd) or
                                     not all(0 < h < float("inf") for h in args.spacing)):
        raise SystemExit("--spacing takes one or %d finite positive values" % args.nd)
    return args


def given_flows(args, nd):
    """(visited frames, load(j0, j1) -> fp32 array [j1 - j0, C, *sp], spatial shape) of --flows."""
    if os.path.isdir(args.flows):
        chain = chain_flow_files(args.flows, args.start, args.direction)
        if not chain:
            raise SystemExit("no flow_%03d_to_*.npy file in %s leads %s from frame %d" % (
                args.start, args.flows, "forward" if args.direction == "fwd" else "backward", args.start))
        frames = [chain[0][0]] + [c[1] for c in chain]
        first = np.load(chain[0][2])
        if first.ndim != nd + 1 or first.shape[0] != nd:
            raise SystemExit("%s must be [%d,%s], got %s" % (chain[0][2], nd, ",".join("DHW"[3 - nd:]), first.shape))
        load = lambda j0, j1: np.stack([np.load(c[2]).astype(np.float32) for c in chain[j0:j1]])
        return frames, load, tuple(first.shape[1:])
    arr = np.load(args.flows, mmap_mode="r")
    if arr.ndim != nd + 2 or arr.shape[1] != nd or arr.shape[0] < 1:
        raise SystemExit("--flows must be [K,%d,%s], got %s" % (nd, ",".join("DHW"[3 - nd:]), arr.shape))
    sgn = 1 if args.direction == "fwd" else -1
    frames = [args.start + sgn * j for j in range(arr.shape[0] + 1)]
    if min(frames) < 0:
        raise SystemExit("a backward trace through %d flows needs --start >= %d" % (arr.shape[0], arr.shape[0]))
    return frames, (lambda j0, j1: np.array(arr[j0:j1], dtype=np.float32)), tuple(arr.shape[2:])


StepFlows = collections.namedtuple("StepFlows", "name frames gt sp visited n_steps source")
StepFlows.__doc__ = """The step flows of one parsed command line.  name: of the series; frames: [T,*sp] on the device, or
None with --flows alone; gt: the known motion gt(t_from, t_to) of a --dataset, or None; sp: the spatial shape; visited:
the n_steps + 1 frames the chain visits ([] when the series is too short for a step); source(j0, j1) -> [j1 - j0, C, *sp]
on the device: the flows of the steps j0 .. j1 - 1."""


def open_step_flows(args, nd, model, make_model, device):
    """The StepFlows of a command line with the options of add_source_args.  make_model() -> flows(frames, pairs) ->
    [2P, C, *sp] is called once, and only when the model has a step to estimate (never with --flows)."""
    frames = gt = None
    name = args.dataset or os.path.basename(args.seq or args.flows.rstrip("/"))
    if args.dataset:
        frames, gt = flow_eval.motion(args.dataset, args.frames, args.size, args.seed, device)
    elif args.seq:
        frames = torch.from_numpy(np.load(args.seq).astype(np.float32)).to(device)
        if frames.dim() != nd + 1:
            raise SystemExit("--seq must be [T,%s], got %s" % (",".join("DHW"[3 - nd:]), tuple(frames.shape)))
    if args.flows:
        visited, load, sp = given_flows(args, nd)
        if frames is not None and tuple(frames.shape[1:]) != sp:
            raise SystemExit("the flows' extent %s is not the series' %s" % (sp, tuple(frames.shape[1:])))
        source = lambda j0, j1: torch.from_numpy(load(j0, j1)).to(device)
    else:
        sp = tuple(int(s) for s in frames.shape[1:])
        chain = step_chain(frames.shape[0], args.gap, args.direction, model)
        visited = ([chain[0][0]] + [c[1] for c in chain]) if chain else []
        if model == "rife":
            pairs = flow_eval.rife_pairs(frames.shape[0], args.gap)
        else:
            pairs = [(t, t + args.gap) for t in range(0, frames.shape[0] - args.gap)]
        flows_of = make_model() if chain else None

        def source(j0, j1):
            # the chain's flows of one direction share their parity in the model's (first, second) flow stack: the
            # strided view goes to the kernels as it is
            part = chain[j0:j1]
            stack = flows_of(frames, [pairs[c[2] // 2] for c in part])
            return stack[part[0][2] % 2::2]
    return StepFlows(name, frames, gt, sp, visited, max(0, len(visited) - 1), source)


def rife_model(Model, args):
    """make_model of a flow2d / flow3d tool: the final IFNet flows of `Model` with the weights under --model."""
    def make_model():
        m = load_pretrained(Model, args.model, torch.device("cuda"))
        return lambda frames, pairs: flow_eval.rife_flows(m, frames, pairs, args.batch)
    return make_model


def upflow_model(make_net, args):
    """make_model of an upflow tool: flow_f_out / flow_b_out of make_net(--model)."""
    def make_model():
        net = make_net(args.model)
        return lambda frames, pairs: flow_eval.upflow_flows(net, frames, pairs, args.batch)
    return make_model


def write_report(doc, json_path, arrays=None):
    """Save `arrays` ({path: array, or a function that makes it}; an entry without a path is skipped) as .npy files and
    dump `doc` as JSON to json_path (if any), creating the directories they go to."""
    arrays = {p: a for p, a in (arrays or {}).items() if p}
    for path in list(arrays) + [json_path] * bool(json_path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    for path, a in arrays.items():
        np.save(path, a() if callable(a) else a)
    if json_path:
        with open(json_path, "w") as f:
            json.dump(doc, f, indent=1)
