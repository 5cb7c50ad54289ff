"""Vortex regions of a series, labelled and tracked: the flag maps of the Eulerian vortex criteria (ops.velgrad: q > 0,
l2 < 0) are cut into connected regions (ops.label_regions), every region is measured (ops.region_table: size, centroid,
bounding box, sums and extrema of vortex planes), consecutive label maps are linked along the estimated flow
(ops.region_links: where the step flow carries each node of a region), and the links are read as a track graph with
birth, death, split, merge and exit events (link_tracks, host code).  Shared by the flow2d / flow3d / upflow `regions`
entry points:

    python -m opticalflowscivis_amd.flow3d.regions --seq frames.npy --criterion both --out labels.npy --track-ids t.npy --json r.json
    python -m opticalflowscivis_amd.flow2d.regions --flows flows.npy --connectivity full --min-size 8 --json r.json
    python -m opticalflowscivis_amd.flow2d.regions --flows flows.npy --mask m.npy --require 1 --reject 128 --json r.json
    python -m opticalflowscivis_amd.upflow.regions --dataset rectangle2d --json r.json

The step flows are those of `vortex` and `trace` (stepflows.step_chain over the flows flow_eval extracts, or --flows).  Step
flow j gives label map j: it lives on the grid of the frame the step starts at, and the same flow carries map j onto
map j + 1, so K step flows give K maps and K - 1 sets of links.  Each chunk of step flows is estimated once; the last
label map of a chunk stays on the device and is linked to the first of the next, so nothing but timing depends on
--chunk.  --mask labels a flag stack `vortex --mask` wrote (with --require / --reject) instead of recomputing it; it
then needs the K - 1 (or more) step flows between the maps and measures no weights.

--out holds int32 [K, *sp]: every node's region as its dense id 1 .. R_k within its step (the row of the table, plus
one), 0 on background and on regions below --min-size; --track-ids the same shape with the track id (from 1) instead.

Out of scope: edge-only (18) connectivity; periodic domains; components connected through time (4-D); vortex core lines;
sub-node region boundaries; autograd; several series in one launch.  Pictures of the fields the regions were cut from:
opticalflowscivis_amd/render.py (the `render` entry points)."""
import argparse
import math
import time

import numpy as np
import torch

from . import ops, stepflows

CRITERIA = {"q": (("q",), ops.VG_FLAG_Q), "l2": (("l2",), ops.VG_FLAG_L2),
            "both": (("q", "l2"), ops.VG_FLAG_Q | ops.VG_FLAG_L2), "mask": ((), None)}
WEIGHTS = ("div", "vmag", "q", "l2")  # the one-plane fields of ops.velgrad
EVENTS = ("birth", "merge", "split", "exit", "death")


def _weight_names(weights):
    names = [n.strip() for n in weights.split(",") if n.strip()] if isinstance(weights, str) else list(weights or ())
    bad = [n for n in names if n not in WEIGHTS]
    if bad or len(set(names)) != len(names):
        raise ValueError("weights are distinct names out of %s, got %r" % (", ".join(WEIGHTS), names))
    return names


def link_tracks(tables, links, min_size=1, min_overlap=0.25):
    """The track graph of a series' regions.  Pure host code.

    tables: a dict with count (int [R]) and offsets (int [K+1]: step k's regions are rows offsets[k] .. offsets[k+1], a
    region's dense id its row minus offsets[k]).  links: K - 1 dicts as ops.region_links returns them (src, dst, count,
    n_out, n_to_background).  min_size and min_overlap are the user's thresholds, not tolerances:
      regions with count < min_size are dropped, and every link that touches one;
      a link a -> b is kept iff count >= max(1, ceil(min_overlap * min(|a|, |b|)));
      b continues a's track iff a is b's kept predecessor with the largest count and b is a's kept successor with the
      largest count (ties: the lower dense id); otherwise b starts a new track.
    Events of a kept region: birth (no kept predecessor, not in the first map), death (no kept successor, not in the
    last map), split (more than one kept successor), merge (more than one kept predecessor), exit (not in the last map,
    n_out > 0 and no other destination -- background or any one region of the next map -- takes more of its nodes).

    Returns a dict: tracks (id from 1, regions [(step, dense id)], first, last), events ({step, region, track, event},
    by step, region, then in the order birth, merge, split, exit, death), track_of (per step an int array over the
    dense ids: the track id, 0 for a dropped region), kept (per step a bool array) and links (per step pair the kept
    links: src, dst, count)."""
    count = np.asarray(tables["count"], dtype=np.int64)
    off = np.asarray(tables["offsets"], dtype=np.int64)
    K = len(off) - 1
    if len(links) != max(0, K - 1):
        raise ValueError("%d label maps need %d sets of links, got %d" % (K, max(0, K - 1), len(links)))
    min_size = int(min_size)
    min_overlap = float(min_overlap)
    if min_size < 1 or not (0.0 <= min_overlap <= 1.0):
        raise ValueError("min_size must be >= 1 and min_overlap in [0, 1], got %r and %r" % (min_size, min_overlap))
    size = [count[off[k]:off[k + 1]] for k in range(K)]
    kept = [s >= min_size for s in size]
    succ = [[[] for _ in range(len(size[k]))] for k in range(K)]
    pred = [[[] for _ in range(len(size[k]))] for k in range(K)]
    kept_links = []
    for j, lk in enumerate(links):
        rows = []
        for a, b, c in zip(np.asarray(lk["src"]).tolist(), np.asarray(lk["dst"]).tolist(), np.asarray(lk["count"]).tolist()):
            if not (kept[j][a] and kept[j + 1][b]):
                continue
            if c >= max(1, math.ceil(min_overlap * min(int(size[j][a]), int(size[j + 1][b])))):
                succ[j][a].append((b, c))
                pred[j + 1][b].append((a, c))
                rows.append((a, b, c))
        kept_links.append({"src": [r[0] for r in rows], "dst": [r[1] for r in rows], "count": [r[2] for r in rows]})
    # per source region the largest number of its nodes that one region of the next map, or the background, receives
    rival = []
    for j, lk in enumerate(links):
        top = np.asarray(lk["n_to_background"], dtype=np.int64).copy()
        np.maximum.at(top, np.asarray(lk["src"], dtype=np.int64), np.asarray(lk["count"], dtype=np.int64))
        rival.append(top)
    best = lambda pairs: min(pairs, key=lambda p: (-p[1], p[0]))[0] if pairs else None
    track_of = [np.zeros(len(size[k]), dtype=np.int64) for k in range(K)]
    tracks, events = [], []
    for k in range(K):
        for i in range(len(size[k])):
            if not kept[k][i]:
                continue
            a = best(pred[k][i])
            if a is not None and best(succ[k - 1][a]) == i:
                tid = int(track_of[k - 1][a])
                tracks[tid - 1]["regions"].append((k, i))
                tracks[tid - 1]["last"] = k
            else:
                tid = len(tracks) + 1
                tracks.append({"id": tid, "regions": [(k, i)], "first": k, "last": k})
            track_of[k][i] = tid
            ev = []
            if k > 0 and not pred[k][i]:
                ev.append("birth")
            if len(pred[k][i]) > 1:
                ev.append("merge")
            if len(succ[k][i]) > 1:
                ev.append("split")
            if k < K - 1:
                n_out = int(links[k]["n_out"][i])
                if n_out > 0 and n_out >= int(rival[k][i]):
                    ev.append("exit")
                if not succ[k][i]:
                    ev.append("death")
            events += [{"step": k, "region": i, "track": tid, "event": e} for e in ev]
    return {"tracks": tracks, "events": events, "track_of": track_of, "kept": kept, "links": kept_links}


def regions_series(step_flows, n_steps, sp, criterion="q", connectivity="face", weights=("q", "vmag"), spacing=1.0,
                   chunk=4, frames=None, dt=1.0, min_size=1, min_overlap=0.25, keep_labels=True, masks=None,
                   require=ops.VG_FLAG_Q, reject=ops.VG_FLAG_NONFINITE, n_flows=None):
    """Label, measure, link and track the regions of n_steps maps.

    step_flows(j0, j1) -> [j1 - j0, C, *sp] hands out the step flows `chunk` at a time, each exactly once.  With a
    criterion of q, l2 or both, flag map j is ops.velgrad's of step flow j (scaled as in `vortex`: frames, dt, spacing)
    and the weights (names out of div, vmag, q, l2) are its planes.  criterion="mask": masks(j0, j1) -> uint8
    [j1 - j0, *sp] on the device hands out the flag maps, a node is foreground under require / reject, only the first
    n_flows (default n_steps - 1) step flows are asked for and no weights are measured.

    Returns a dict: table (the columns of ops.region_table over all R rows, offsets [n_steps + 1]; no rank), links (per
    step pair, ops.region_links), graph (link_tracks), steps (per step: regions, regions_kept, foreground_fraction,
    largest), keep_labels: labels (int32 [n_steps, *sp] host tensor of dense ids from 1, 0 on background and dropped
    regions) and track_ids, and the totals time_flows_s, time_kernel_s."""
    if criterion not in CRITERIA:
        raise ValueError("criterion must be one of %s, got %r" % (", ".join(CRITERIA), criterion))
    chunk = max(1, int(chunk))
    n_steps = int(n_steps)
    sp = tuple(int(s) for s in sp)
    nd = len(sp)
    nodes = int(np.prod(sp))
    names = _weight_names(weights)
    if criterion == "mask":
        if masks is None:
            raise ValueError("criterion 'mask' needs masks(j0, j1)")
        if names:
            raise ValueError("a given mask carries no planes: weights must be empty, got %r" % (names,))
        n_flows = max(0, n_steps - 1) if n_flows is None else int(n_flows)
        if n_flows < n_steps - 1:
            raise ValueError("%d maps need %d step flows between them, got %d" % (n_steps, n_steps - 1, n_flows))
        scales = None
    else:
        n_flows = n_steps
        frames = list(range(n_steps + 1)) if frames is None else list(frames)
        if len(frames) != n_steps + 1:
            raise ValueError("frames must name the %d frames the chain visits, got %d" % (n_steps + 1, len(frames)))
        scales = stepflows.step_scales(frames, dt)
        require, reject = CRITERIA[criterion][1], ops.VG_FLAG_NONFINITE
        fields = [n for n in ops.VG_FIELDS if n in CRITERIA[criterion][0] or n in names]
    cols, links, rows = [], [], []
    labels_host = torch.zeros((n_steps,) + sp, dtype=torch.int32) if keep_labels else None
    prev = None  # (labels [1,*sp], rank [1,*sp], regions, flow [1,C,*sp]) of the last map so far
    t_flows = t_kernel = 0.0
    for j0 in range(0, n_steps, chunk):
        j1 = min(n_steps, j0 + chunk)
        nf = min(j1, n_flows) - j0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = step_flows(j0, j0 + nf) if nf > 0 else None
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        w = None
        if criterion == "mask":
            flags = masks(j0, j1)
        else:
            vg = ops.velgrad(f, fields, spacing, scales[j0:j1], with_flags=True, summary=False)
            flags = vg["flags"]
            if names:
                idx = [vg["planes"][n].start for n in names]
                w = vg["out"] if idx == list(range(vg["out"].shape[1])) else vg["out"][:, idx].contiguous()
        lab = ops.label_regions(flags, require, reject, connectivity)
        tab = ops.region_table(lab, w, names)
        L, rank = lab["labels"], tab["rank"]
        off = tab["offsets"]
        if prev is not None:  # the seam: the last map of the chunk before onto this chunk's first
            seam = {"offsets": np.array([0, prev[2], prev[2] + int(off[1])], dtype=np.int64),
                    "rank": torch.cat([prev[1], rank[:1]])}
            links += ops.region_links(torch.cat([prev[0], L[:1]]), prev[3], seam)
        if j1 - j0 > 1:
            links += ops.region_links(L, f, tab)
        if j1 < n_steps:
            prev = (L[-1:].clone(), rank[-1:].clone(), int(off[-1] - off[-2]), f[j1 - j0 - 1:j1 - j0].clone())
        if keep_labels:  # dense ids from 1 by a lookup in the rank map; regions below min_size -> 0
            P = nodes
            flat = L.view(j1 - j0, P)
            dense = torch.gather(rank.view(j1 - j0, P), 1, (flat - 1).clamp(min=0).long()) + 1
            small = torch.from_numpy(np.asarray(tab["count"]) < int(min_size)).to(L.device)
            base = torch.from_numpy(off[:-1]).to(L.device).view(-1, 1)
            drop = small[(base + dense.long() - 1).clamp(0, len(tab["count"]) - 1)] if len(tab["count"]) else (flat < 0)
            labels_host[j0:j1].copy_(torch.where((flat > 0) & ~drop, dense, torch.zeros_like(dense)).view(L.shape))
        torch.cuda.synchronize()
        t_flows += t1 - t0
        t_kernel += time.perf_counter() - t1
        tab["step"] = tab["step"] + j0
        cols.append(tab)
        for k in range(j1 - j0):
            c = tab["count"][off[k]:off[k + 1]]
            rows.append({"step": j0 + k, "regions": int(len(c)), "regions_kept": int((c >= int(min_size)).sum()),
                         "foreground_fraction": float(c.sum()) / nodes, "largest": int(c.max()) if len(c) else 0})
        del f, lab, tab, L, rank
    keys = [k for k in (cols[0] if cols else {}) if k not in ("rank", "offsets")]
    table = {k: np.concatenate([c[k] for c in cols]) for k in keys}
    sizes = [int(r["regions"]) for r in rows]
    table["offsets"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if not cols:
        table["count"] = np.zeros(0, dtype=np.int64)
    graph = link_tracks(table, links, min_size, min_overlap)
    res = {"table": table, "links": links, "graph": graph, "steps": rows, "weights": names, "time_flows_s": t_flows,
           "time_kernel_s": t_kernel}
    if keep_labels:
        res["labels"] = labels_host
        tid = np.zeros((n_steps,) + sp, dtype=np.int32)
        lab_np = labels_host.numpy()
        for k in range(n_steps):
            lut = np.concatenate([[0], graph["track_of"][k]]).astype(np.int32)
            tid[k] = lut[lab_np[k]]
        res["track_ids"] = torch.from_numpy(tid)
    return res


def _args(nd, desc, model):
    sp = ",".join("DHW"[3 - nd:])
    ap = argparse.ArgumentParser(description=desc)
    stepflows.add_source_args(ap, nd, model, direction="fwd: the flows t -> t+1; bwd: the model's own backward flows, from "
                              "the last frame down", chunk="step flows estimated, labelled and linked at a time",
                              dt="the time one frame spans: velocity = displacement / (frames spanned * dt)", spacing=True)
    ap.add_argument("--criterion", choices=("q", "l2", "both"), default="q",
                    help="foreground: q > 0, l2 < 0, or both (and every value finite)")
    ap.add_argument("--connectivity", choices=("face", "full"), default="face", help="face: 4 / 6 neighbours; full: 8 / 26")
    ap.add_argument("--min-size", type=int, default=1, help="regions with fewer nodes are dropped")
    ap.add_argument("--min-overlap", type=float, default=0.25,
                    help="a link is kept when it carries at least this share of the smaller region's nodes")
    ap.add_argument("--weights", default=None, help="comma-separated planes measured per region, out of %s (default "
                    "q,vmag; none with --mask)" % ",".join(WEIGHTS))
    ap.add_argument("--mask", default=None, metavar="M.npy", help="label this flag stack [K, %s] (uint8, as `vortex --mask` "
                    "writes it) instead of computing the criterion; needs --flows" % sp)
    ap.add_argument("--require", type=int, default=None, help="with --mask: bits a foreground node has (default 1)")
    ap.add_argument("--reject", type=int, default=None, help="with --mask: bits a foreground node has not (default 128)")
    ap.add_argument("--out", default=None, metavar="L.npy", help="write the dense labels [K, %s] (int32) here" % sp)
    ap.add_argument("--track-ids", default=None, metavar="T.npy", help="write every node's track id [K, %s] (int32) here" % sp)
    ap.add_argument("--save-flows", default=None, metavar="FLOWS.npy", help="write the step flows [K, %d, %s] here (--flows reads them)" % (nd, sp))
    return ap


def check_args(args):
    """What the parser cannot express."""
    stepflows.check_source_args(args)
    if args.min_size < 1:
        raise SystemExit("--min-size must be >= 1")
    if not (0.0 <= args.min_overlap <= 1.0):
        raise SystemExit("--min-overlap must lie in [0, 1]")
    if args.mask:
        if not args.flows or args.dataset or args.seq:
            raise SystemExit("--mask needs --flows (the step flows between its maps) and no --dataset / --seq")
        if args.weights:
            raise SystemExit("--mask carries no planes: --weights cannot be measured")
        if args.save_flows:
            raise SystemExit("--save-flows with --mask: the flows are the ones --flows names")
        args.require = 1 if args.require is None else args.require
        args.reject = 128 if args.reject is None else args.reject
        if not (0 <= args.require <= 255 and 0 <= args.reject <= 255) or args.require & args.reject:
            raise SystemExit("--require and --reject are disjoint bytes")
        args.weights = ""
    else:
        if args.require is not None or args.reject is not None:
            raise SystemExit("--require / --reject select bits of a --mask")
        args.weights = "q,vmag" if args.weights is None else args.weights
    try:
        _weight_names(args.weights)
    except ValueError as e:
        raise SystemExit("--weights: %s" % e)
    return args


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


def run(args, nd, model, make_model):
    """The regions of one parsed command line.  make_model() -> flows(frames, pairs) -> [2P, C, *sp]."""
    dev = torch.device("cuda")
    sf = stepflows.open_step_flows(args, nd, model, make_model, dev)
    name, sp, visited, source = sf.name, sf.sp, sf.visited, sf.source
    K = n_flows = sf.n_steps
    masks = None
    if args.mask:
        m = np.load(args.mask, mmap_mode="r")
        if m.dtype != np.uint8 or tuple(m.shape[1:]) != sp or not 1 <= m.shape[0] <= n_flows + 1 or m.shape[0] < n_flows:
            raise SystemExit("--mask must be uint8 [K,%s] with K the number of step flows (%d) or one more, got %s %s" %
                             (",".join(str(s) for s in sp), n_flows, m.dtype, m.shape))
        K = int(m.shape[0])
        masks = lambda j0, j1: torch.from_numpy(np.array(m[j0:j1])).to(dev)
    saved = []
    if args.save_flows:
        inner = source

        def source(j0, j1):
            f = inner(j0, j1)
            saved.append(f.cpu())
            return f
    spacing = args.spacing[0] if len(args.spacing) == 1 else tuple(args.spacing)
    keep = bool(args.out or args.track_ids)
    res = regions_series(source, K, sp, "mask" if args.mask else args.criterion, args.connectivity, args.weights, spacing,
                         args.chunk, frames=None if args.mask else (visited or [0]), dt=args.dt, min_size=args.min_size,
                         min_overlap=args.min_overlap, keep_labels=keep, masks=masks,
                         require=args.require if args.mask else ops.VG_FLAG_Q,
                         reject=args.reject if args.mask else ops.VG_FLAG_NONFINITE, n_flows=n_flows if args.mask else None)
    g = res["graph"]
    doc = {"sequence": name, "shape": list(sp), "model": None if args.flows else args.model, "direction": args.direction,
           "chunk": args.chunk, "gap": args.gap, "criterion": "mask" if args.mask else args.criterion,
           "connectivity": args.connectivity, "min_size": args.min_size, "min_overlap": args.min_overlap,
           "weights": res["weights"], "spacing": list(args.spacing), "dt": args.dt, "frames": visited[:K + 1],
           "steps": res["steps"], "table": _jsonable(res["table"]), "links": _jsonable(res["links"]),
           "kept_links": _jsonable(g["links"]), "tracks": _jsonable(g["tracks"]), "events": _jsonable(g["events"]),
           "track_of": _jsonable(g["track_of"]), "time_inference_s": res["time_flows_s"],
           "time_kernel_s": res["time_kernel_s"]}
    if not res["steps"]:
        print("%s: the chain has no step" % name)
    for r in res["steps"]:
        print("%s %s step %d: %d regions (%d kept)  foreground %.3f  largest %d" % (
            name, args.direction, r["step"], r["regions"], r["regions_kept"], r["foreground_fraction"], r["largest"]))
    if res["steps"]:
        n_ev = {e: sum(1 for x in g["events"] if x["event"] == e) for e in EVENTS}
        print("%d tracks  %s" % (len(g["tracks"]), "  ".join("%s %d" % (e, n_ev[e]) for e in EVENTS)))
        print("flows %.3f s  kernel %.4f s" % (res["time_flows_s"], res["time_kernel_s"]))
    stepflows.write_report(doc, args.json, {
        args.out: lambda: res["labels"].numpy(), args.track_ids: lambda: res["track_ids"].numpy(),
        args.save_flows: lambda: torch.cat(saved).numpy() if saved else np.zeros((0, nd) + sp, np.float32)})
    return doc


def main_rife(Model, nd, argv=None):
    """flow2d / flow3d: the steps m -> m+h (or back) of the final IFNet flows."""
    args = check_args(_args(nd, "Vortex regions of the flows of a RIFE model, labelled and tracked", "rife").parse_args(argv))
    return run(args, nd, "rife", stepflows.rife_model(Model, args))


def main_upflow(make_net, argv=None):
    """upflow: the steps t -> t+gap through flow_f_out, or back through flow_b_out."""
    args = check_args(_args(2, "Vortex regions of UPFlow's flows, labelled and tracked", "upflow").parse_args(argv))
    return run(args, 2, "upflow", stepflows.upflow_model(make_net, args))
