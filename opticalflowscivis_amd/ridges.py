"""Ridge surfaces: the transport barriers an FTLE field exists to find, as geometry.  Every frame of a stack of scalar
volumes -- the FTLE fields of a series' estimated flows, or any stored field -- becomes one indexed triangle mesh of its
height ridges (Eberly: the gradient is orthogonal to the eigenvector of the Hessian's smallest eigenvalue, and that
eigenvalue is below -strength), extracted on the device by Marching Ridges on the Kuhn split of every cell
(ops.ridge_surfaces: a node launch, a count launch and an emit launch per `--chunk` of frames).  An isosurface of the
same field is no substitute: it wraps the ridge in a tube whose thickness depends on the isovalue.  The flow3d `ridges`
entry point:

    python -m opticalflowscivis_amd.flow3d.ridges --seq frames.npy --window 4 --direction bwd --refine 2 --sigma 1 \\
        --strength 0.05 --fmin 0.2 --min-faces 32 --mesh-dir meshes --format ply --out ridges.npz --json r.json
    python -m opticalflowscivis_amd.flow3d.ridges --field vg.npy --plane 4 --valley --strength 0.01 --mesh-dir meshes

The first form runs ftle.ftle_series (all of the `ftle` entry point's options) and extracts the ridges of every window's
field on the lattice spacing the FTLE returns: the repelling structures of a forward field, the attracting ones with
--direction bwd.  The second takes [K, D,H,W] or [K, NP, D,H,W] (--plane) as flow3d.isosurface does; --valley extracts
the valley surfaces instead (of lambda2, of a density), which are by construction the ridges of -f.

Second differences amplify noise, so --sigma smooths every volume first with a separable Gaussian (plumbing: torch),
normalised over the finite nodes under the kernel; a node that is not finite stays so, and the ridge stops one node
short of it, as it does one node inside the border.  --strength is the least -lambda of a ridge node (in units of
f / spacing^2), --fmin the least f (under --valley: of -f).  Where the eigenvector cannot be oriented consistently over
a tetrahedron (near degenerate eigenvalues) the tetrahedron is twisted and emits nothing: a hole, counted per frame
with its share of the tetrahedra that could have emitted.  --min-faces and --min-area drop the connected components
(faces that share a vertex index: numpy) below them, which is what removes the speckle of a noisy field.

--mesh-dir gets frame_%04d.ply (isosurface.write_ply: x y z nx ny nz value0 value1, with value0 = f, value1 = lambda
and the normal (0, 0, 0): a ridge surface need not be orientable, so neither normals nor the winding of the faces mean
anything) or frame_%04d.npz (vertices, values, faces).  --out gets one .npz of all frames: vertices, values, faces
(indices local to their frame), vertex_offsets, face_offsets.  The JSON holds per frame the class counts of its nodes,
vertices, faces, twisted tetrahedra and their share, area, boundary_edges, the components kept and dropped, and times.

3-D only: in 2-D ridges are curves, which need contour-line machinery.  Out of scope: ridge lines (co-dimension 2),
scale-space ridges, mesh smoothing or simplification, filtering by the flux across the surface, drawing the meshes in
the ray-caster."""
import argparse
import math
import os
import time

import numpy as np
import torch

from . import ops, stepflows
from .isosurface import mesh_stats, write_ply


def gaussian_smooth(volumes, sigma):
    """[K,D,H,W] smoothed along D, H and W with a Gaussian of standard deviation `sigma` nodes, truncated at 3 sigma and
    normalised over the finite nodes under it (so a border or a hole does not darken its neighbourhood); nodes that are
    not finite stay NaN.  sigma <= 0: the input.  Plumbing: shifted slices in torch, fp32."""
    sigma = float(sigma)
    if not sigma > 0:
        return volumes
    r = max(1, int(math.ceil(3.0 * sigma)))
    w = [math.exp(-0.5 * (i / sigma) ** 2) for i in range(-r, r + 1)]
    fin = torch.isfinite(volumes)
    num = torch.where(fin, volumes, torch.zeros_like(volumes))
    den = fin.to(volumes.dtype)
    for ax in (1, 2, 3):
        n = volumes.shape[ax]
        pad = [0, 0] * (3 - ax) + [r, r] + [0, 0] * (ax - 1)  # F.pad counts from the last axis
        pn, pd = torch.nn.functional.pad(num, pad), torch.nn.functional.pad(den, pad)
        num, den = torch.zeros_like(num), torch.zeros_like(den)
        for i, wi in enumerate(w):
            num += wi * pn.narrow(ax, i, n)
            den += wi * pd.narrow(ax, i, n)
    return torch.where(fin & (den > 0), num / den.clamp_min(1e-30), torch.full_like(num, float("nan")))


def face_components(faces, n_vertices):
    """Per face of an indexed mesh the label of its connected component (faces that share a vertex index are
    connected): the smallest vertex index of the component, by min-label propagation with pointer jumping (numpy)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lab = np.arange(int(n_vertices), dtype=np.int64)
    if f.shape[0] == 0:
        return np.zeros(0, np.int64)
    while True:
        m = lab[f].min(1)
        new = lab.copy()
        for c in range(3):
            np.minimum.at(new, f[:, c], m)
        new = new[new]
        if np.array_equal(new, lab):
            return lab[f[:, 0]]
        lab = new


def filter_components(vertices, faces, values=None, min_faces=0, min_area=0.0):
    """Drop the connected components with fewer than min_faces faces or less than min_area area and re-index the
    vertices.  Returns (vertices, faces, values, kept, dropped); the order of what stays is unchanged."""
    v = np.asarray(vertices).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    if f.shape[0] == 0:
        return v[:0], f, None if values is None else values[:0], 0, 0
    lab = face_components(f, v.shape[0])
    roots, inv, cnt = np.unique(lab, return_inverse=True, return_counts=True)
    p = v.astype(np.float64)
    tri = 0.5 * np.sqrt((np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]) ** 2).sum(1))
    area = np.bincount(inv, weights=tri, minlength=roots.size)
    keep = (cnt >= int(min_faces)) & (area >= float(min_area))
    fk = f[keep[inv]]
    used = np.zeros(v.shape[0], dtype=bool)
    used[fk.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return (v[used], remap[fk].astype(f.dtype), None if values is None else np.asarray(values)[used],
            int(keep.sum()), int((~keep).sum()))


def ridge_series(volumes_of, n_frames, spacing=1.0, strength=0.0, fmin=-float("inf"), valley=False, sigma=0.0,
                 min_faces=0, min_area=0.0, chunk=4, times=None, sink=None):
    """Ridge meshes of the n_frames volumes that volumes_of(j0, j1) -> fp32 [j1 - j0, D, H, W] on the device hands out
    `chunk` at a time (each exactly once; one ops.ridge_surfaces call -- three launches -- per chunk).  sigma: the
    pre-smoothing (gaussian_smooth); min_faces, min_area: the component filter (filter_components).  times: the time of
    every frame (default its index).  sink(j, mesh): called with every frame's filtered mesh, a dict of host arrays
    vertices [V,3], values [V,2] (f in the field's own sign, lam) and faces [T,3].

    Returns a dict: frames (one dict per frame: frame, time, classes, vertices, faces -- after the filter --
    vertices_extracted, faces_extracted, twisted, tetrahedra, twisted_share, area, boundary_edges, bbox, components_kept,
    components_dropped, status, time_smooth_s, time_kernel_s, time_filter_s) and the totals time_load_s, time_smooth_s,
    time_kernel_s, time_filter_s.  A frame's device times are its share of its chunk's.  FlowsciKernelError when a
    chunk's status is set."""
    chunk = max(1, int(chunk))
    n_frames = int(n_frames)
    times = list(range(n_frames)) if times is None else [float(t) for t in times]
    if len(times) != n_frames:
        raise ValueError("times must name the %d frames, got %d" % (n_frames, len(times)))
    rows = []
    tot = {"time_load_s": 0.0, "time_smooth_s": 0.0, "time_kernel_s": 0.0, "time_filter_s": 0.0}
    for j0 in range(0, n_frames, chunk):
        j1 = min(n_frames, j0 + chunk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = volumes_of(j0, j1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        v = gaussian_smooth(v, sigma)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        r = ops.ridge_surfaces(v, spacing, strength, fmin, valley)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        status = int(r["status"].cpu()[0])
        ops.ridge_surfaces_check({"status": status})
        vo, fo = r["vertex_offsets"].cpu().tolist(), r["face_offsets"].cpu().tolist()
        counts, classes = r["counts"].cpu().tolist(), r["classes"].cpu().tolist()
        vert, vals, faces = r["vertices"].cpu().numpy(), r["values"].cpu().numpy(), r["faces"].cpu().numpy()
        n = j1 - j0
        tot["time_load_s"] += t1 - t0
        tot["time_smooth_s"] += t2 - t1
        tot["time_kernel_s"] += t3 - t2
        for j in range(j0, j1):
            k = j - j0
            t4 = time.perf_counter()
            val = vals[vo[k]:vo[k + 1]].copy()
            if valley:
                val[:, 0] = -val[:, 0]
            pv, pf, pw, kept, dropped = filter_components(vert[vo[k]:vo[k + 1]], faces[fo[k]:fo[k + 1]], val, min_faces, min_area)
            st = mesh_stats(pv, pf)
            t5 = time.perf_counter()
            tot["time_filter_s"] += t5 - t4
            st.pop("volume")  # (meaningless without an orientation)
            nv, nf, tw, te = counts[k]
            rows.append(dict({"frame": j, "time": times[j], "classes": dict(zip(ops.RIDGE_CLASS_NAMES, classes[k])),
                              "vertices": int(pv.shape[0]), "faces": int(pf.shape[0]), "vertices_extracted": nv,
                              "faces_extracted": nf, "twisted": tw, "tetrahedra": te,
                              "twisted_share": tw / te if te else 0.0}, **st, components_kept=kept,
                             components_dropped=dropped, status=status, time_smooth_s=(t2 - t1) / n,
                             time_kernel_s=(t3 - t2) / n, time_filter_s=t5 - t4))
            if sink is not None:
                sink(j, {"vertices": pv, "values": pw, "faces": pf})
        del v, r
    return dict(tot, frames=rows)


def _args(nd, model):
    ap = argparse.ArgumentParser(description="Extract the ridge surfaces (LCS) of the FTLE fields of a series' flows, or the "
                                 "ridge / valley surfaces of a stored field")
    stepflows.add_source_args(ap, nd, model, direction="fwd: repelling structures; bwd: attracting ones",
                              chunk="step flows estimated, or frames of --field extracted, at a time",
                              dt="the time one frame spans: T = frames spanned * dt")
    ap.add_argument("--window", type=int, default=None, help="steps of the chain a flow map integrates over (FTLE)")
    ap.add_argument("--every", type=int, default=1, help="a window opens at every EVERY-th step of the chain")
    ap.add_argument("--refine", type=int, default=1, help="lattice nodes per grid element along every axis")
    ap.add_argument("--method", choices=sorted(ops._ADV_METHODS), default="euler")
    ap.add_argument("--substeps", type=int, default=1)
    ap.add_argument("--accept-out", action="store_true", help="a particle that left the box counts with its exit point")
    ap.add_argument("--field", default=None, help="skip the FTLE: a .npy field [K,D,H,W] or [K,NP,D,H,W]")
    ap.add_argument("--plane", type=int, default=0, help="the plane of a [K,NP,D,H,W] --field")
    ap.add_argument("--spacing", type=float, nargs="+", default=[1.0], help="node spacing of --field: one value or D H W")
    ap.set_defaults(nd=nd)  # (what stepflows.check_source_args measures --spacing against)
    ap.add_argument("--valley", action="store_true", help="valley surfaces: the ridges of -f")
    ap.add_argument("--sigma", type=float, default=0.0, help="pre-smoothing: a Gaussian of SIGMA nodes (0: none)")
    ap.add_argument("--strength", type=float, default=0.0, help="least -lambda of a ridge node, in f / spacing^2")
    ap.add_argument("--fmin", type=float, default=-float("inf"), help="least f of a ridge node (--valley: of -f)")
    ap.add_argument("--min-faces", type=int, default=0, help="drop connected components with fewer faces")
    ap.add_argument("--min-area", type=float, default=0.0, help="drop connected components with less area")
    ap.add_argument("--mesh-dir", default=None, metavar="DIR", help="write frame_%%04d.<format> here")
    ap.add_argument("--format", choices=("ply", "npz"), default="ply")
    ap.add_argument("--out", default=None, metavar="RIDGES.npz", help="write all frames' meshes here")
    ap.add_argument("--ftle-out", default=None, metavar="FTLE.npy", help="write the FTLE fields the ridges are of here")
    return ap


def check_args(args):
    """What the parser cannot express."""
    if args.field:
        if args.dataset or args.seq or args.flows or args.ftle_out:
            raise SystemExit("--field excludes --dataset, --seq, --flows and --ftle-out")
        if args.chunk < 1:
            raise SystemExit("--chunk must be >= 1")
        if len(args.spacing) not in (1, 3) or not all(0 < h < float("inf") for h in args.spacing):
            raise SystemExit("--spacing takes one or 3 finite positive values")
    else:
        stepflows.check_source_args(args)
        if args.window is None:
            raise SystemExit("--window is needed (or --field)")
        for name in ("window", "every", "refine", "substeps"):
            if getattr(args, name) < 1:
                raise SystemExit("--%s must be >= 1" % name)
    if not 0 <= args.strength < float("inf"):
        raise SystemExit("--strength must be finite and >= 0")
    if not args.fmin < float("inf"):
        raise SystemExit("--fmin must be a number below +inf")
    if not 0 <= args.sigma < float("inf") or args.min_faces < 0 or not 0 <= args.min_area < float("inf"):
        raise SystemExit("--sigma, --min-faces and --min-area must be finite and >= 0")
    return args


def run(args, model, make_model):
    """The ridge meshes of one parsed command line.  make_model() -> flows(frames, pairs) -> [2P, 3, *sp]."""
    from .ftle import ftle_series
    from .render import series_source
    dev = torch.device("cuda")
    doc = {}
    if args.field:
        a, take, name = series_source(args, 3)
        K = int(a.shape[0])
        sp = tuple(int(s) for s in take(0, 1).shape[1:])
        spacing = args.spacing[0] if len(args.spacing) == 1 else tuple(args.spacing)
        source = lambda j0, j1: torch.from_numpy(np.array(take(j0, j1), np.float32)).to(dev)
        times = [j * args.dt for j in range(K)]
        chunk = args.chunk
        doc.update(source=name, plane=args.plane if a.ndim == 5 else None, spacing=list(args.spacing))
        ftle_field = None
    else:
        sf = stepflows.open_step_flows(args, 3, model, make_model, dev)
        name = sf.name
        res = ftle_series(sf.source, sf.n_steps, sf.sp, args.window, args.every, args.refine, args.method, args.substeps,
                          args.chunk, accept_out=args.accept_out, frames=sf.visited or [0], dt=args.dt)
        ftle_field = res["ftle"]
        K, sp, spacing = int(ftle_field.shape[0]), tuple(res["lattice"]), res["spacing"]
        source = lambda j0, j1: ftle_field[j0:j1]
        times = [w["t_from"] * args.dt for w in res["windows"]]
        chunk = 1  # (a window's lattice is refine^3 times the grid)
        if not res["windows"]:
            print("%s: the chain has %d steps, too few for a window of %d" % (name, sf.n_steps, args.window))
        doc.update(source=name, model=None if args.flows else args.model, direction=args.direction, method=args.method,
                   substeps=args.substeps, gap=args.gap, window=args.window, every=args.every, refine=args.refine,
                   accept_out=bool(args.accept_out), dt=args.dt, visited=sf.visited, spacing=spacing,
                   windows=res["windows"], time_inference_s=res["time_flows_s"], time_advect_s=res["time_advect_s"],
                   time_ftle_s=res["time_ftle_s"])
    if args.mesh_dir:
        os.makedirs(args.mesh_dir, exist_ok=True)
    meshes = []

    def sink(j, m):
        if args.out:
            meshes.append(m)
        if not args.mesh_dir:
            return
        path = os.path.join(args.mesh_dir, "frame_%04d.%s" % (j, args.format))
        if args.format == "ply":
            write_ply(path, m["vertices"], np.zeros_like(m["vertices"]), m["faces"], m["values"])
        else:
            np.savez(path, vertices=m["vertices"], values=m["values"], faces=m["faces"])

    out = ridge_series(source, K, spacing, args.strength, args.fmin, args.valley, args.sigma, args.min_faces, args.min_area,
                       chunk, times, sink)
    doc.update(shape=list(sp), valley=bool(args.valley), sigma=args.sigma, strength=args.strength,
               fmin=args.fmin if args.fmin > -float("inf") else None, min_faces=args.min_faces, min_area=args.min_area,
               format=args.format, frames=out["frames"], time_load_s=out["time_load_s"], time_smooth_s=out["time_smooth_s"],
               time_kernel_s=out["time_kernel_s"], time_filter_s=out["time_filter_s"])
    for w in out["frames"]:
        print("%s frame %d t %.4g: eligible %d  | %d vertices  %d faces  area %.6g  boundary edges %d  | twisted %d of %d "
              "(%.1f %%)  components kept %d dropped %d" % (
                  name, w["frame"], w["time"], w["classes"]["eligible"], w["vertices"], w["faces"], w["area"],
                  w["boundary_edges"], w["twisted"], w["tetrahedra"], 100 * w["twisted_share"], w["components_kept"],
                  w["components_dropped"]))
    print("smoothing %.4f s  kernels %.4f s  filter %.3f s" % (out["time_smooth_s"], out["time_kernel_s"], out["time_filter_s"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        cat = lambda key, shape, dt: (np.concatenate([m[key] for m in meshes]) if meshes else np.zeros(shape, dt))
        np.savez(args.out, vertices=cat("vertices", (0, 3), np.float32), values=cat("values", (0, 2), np.float32),
                 faces=cat("faces", (0, 3), np.int32),
                 vertex_offsets=np.cumsum([0] + [len(m["vertices"]) for m in meshes]).astype(np.int64),
                 face_offsets=np.cumsum([0] + [len(m["faces"]) for m in meshes]).astype(np.int64))
    stepflows.write_report(doc, args.json, {args.ftle_out: (lambda: ftle_field.cpu().numpy()) if ftle_field is not None else None})
    return doc


def main_rife(Model, argv=None):
    """flow3d: the ridge surfaces of the FTLE fields of the final IFNet flows, or of --field."""
    args = check_args(_args(3, "rife").parse_args(argv))
    return run(args, "rife", stepflows.rife_model(Model, args))
