"""Ridge surfaces on the GPU: the three passes of ops.ridge_surfaces timed one by one (fs_ridge_nodes3d: 19-point
differences and the fp64 Jacobi eigen-solve of every node; fs_ridge_count3d: the stored operands of every cell's corners
to edge masks and per-row counts; fs_ridge_emit3d: vertices, values and faces) on one volume of 256^3 nodes, for three
fields -- band-limited, the Gaussian sphere shell of the tests tiled to that size, white noise -- next to two things in
the same run:
  * fs_iso_count3d and fs_iso_emit3d on the same volume (iso: the field's median), the marching passes' nearest
    neighbours: the same rows, chunks and table, one value per corner instead of four and a class;
  * the stock composition in torch, fp64: gradient and Hessian by slicing, torch.linalg.eigh, d = e . g, and the edge
    test on the seven owned edges (detection only: no tetrahedra, no positions).  It runs on a SLAB of --stock-slab
    z-layers and is extrapolated linearly in the interior layers to the whole volume; the table says so.  Where torch
    cannot run it on this device the table says "not measured" and why.

Per case: `warmup` rounds, then `reps` rounds that launch the five kernels in turn, each between two HIP events on
preallocated outputs (the prefix sums between count and emit are made once, outside the timed window); the table gives
the median and the 10th / 90th percentile.  Bytes are the algorithm's (ops.ridge_cost, ops.isosurface_cost), set against
the 8 TB/s HBM peak (AMD's MI355X spec): `share` is the time those bytes take at that rate over the measured time.  The
timings are WARM: the rounds repeat on one volume (67 MB) and its operands (336 MB), which together do not fit the 256 MB
last-level cache but are partly served from it.

    python scripts/ridgebench.py [--out profiles/ridges.txt] [--json ridges.json] [--size 256]

One process, the cases one after another, each under its own time limit (SIGALRM): a case that overruns ends the run."""
import argparse
import ctypes
import json
import math
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402

CASE_LIMIT_S = 280
HBM_BPS = 8.0e12
FIELDS = ("band", "shell", "noise")
EDGES = ((0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1))


def pct(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


def field(kind, S):
    """([1, S, S, S] fp32 on the GPU, strength, fmin)"""
    sp = (S, S, S)
    if kind == "noise":
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        return torch.randn((1,) + sp, generator=g, device="cuda"), 0.0, -float("inf")
    if kind == "shell":  # the shell of tests/ridge_fields.py (radius 6.3, sigma 1.5) on a 20 x 24 x 24 tile
        z, y, x = torch.meshgrid(*[torch.arange(s, dtype=torch.float64, device="cuda") for s in (20, 24, 24)], indexing="ij")
        r = torch.sqrt((x - 11.4) ** 2 + (y - 11.6) ** 2 + (z - 9.7) ** 2)
        u = torch.exp(-(r - 6.3) ** 2 / (2 * 1.5 ** 2)).float()
        return u.repeat(*[-(-S // n) for n in (20, 24, 24)])[None, :S, :S, :S].contiguous(), 0.1, 0.5
    grid = torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device="cuda") / s for s in sp], indexing="ij")
    cpu = torch.Generator().manual_seed(11)
    u = torch.zeros((1,) + sp, device="cuda")
    for _ in range(8):
        w = torch.randint(-4, 5, (3,), generator=cpu).tolist()
        a, ph = float(torch.randn((), generator=cpu)), float(torch.rand((), generator=cpu)) * 2 * math.pi
        u[0] += a * torch.cos(2 * math.pi * sum(wi * x for wi, x in zip(w, grid)) + ph)
    return u, 0.0, -float("inf")


def stock(vol, strength, slab):
    """The torch composition on the first `slab` z-layers: (ms differences, ms eigh, ms edge test, interior layers,
    active edges, note)."""
    f = vol[0, :slab].double()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    c = lambda dz, dy, dx: f[1 + dz:f.shape[0] - 1 + dz, 1 + dy:f.shape[1] - 1 + dy, 1 + dx:f.shape[2] - 1 + dx]
    try:
        ev[0].record()
        ax = ((0, 0, 1), (0, 1, 0), (1, 0, 0))
        g = torch.stack([(c(*a) - c(*[-v for v in a])) * 0.5 for a in ax], -1)
        H = torch.empty(g.shape[:-1] + (3, 3), dtype=torch.float64, device=f.device)
        for i, a in enumerate(ax):
            H[..., i, i] = (c(*a) - 2.0 * c(0, 0, 0)) + c(*[-v for v in a])
        for i, j in ((0, 1), (0, 2), (1, 2)):
            p = lambda si, sj: c(*[si * u + sj * v for u, v in zip(ax[i], ax[j])])
            H[..., i, j] = H[..., j, i] = ((p(1, 1) - p(1, -1)) - (p(-1, 1) - p(-1, -1))) * 0.25
        ev[1].record()
        lam, U = torch.linalg.eigh(H)
        ev[2].record()
        e, l0 = U[..., :, 0], lam[..., 0]
        d = (e * g).sum(-1)
        ok = l0 <= -strength
        D, Hh, W = d.shape
        active = 0
        for dz, dy, dx in EDGES:
            a = (slice(0, D - dz), slice(0, Hh - dy), slice(0, W - dx))
            b = (slice(dz, D), slice(dy, Hh), slice(dx, W))
            flip = (e[a] * e[b]).sum(-1) < 0
            active += int((ok[a] & ok[b] & (torch.signbit(d[a]) != (torch.signbit(d[b]) ^ flip))).sum())
        ev[3].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3]), slab - 2, active, "ok"
    except Exception as err:  # (a device without a batched symmetric eigensolver, or out of memory)
        return None, None, None, slab - 2, 0, "%s: %s" % (type(err).__name__, str(err).split("\n")[0][:120])


def bench(kind, S, warmup, reps, slab):
    vol, strength, fmin = field(kind, S)
    sp, P = (S, S, S), S ** 3
    stream = ops._stream(vol)
    iso = float(vol.median())
    operands, cls = ops.ridge_nodes(vol, 1.0, strength, fmin)
    ws, off = ops.ridge_count(operands, cls)
    V, T = int(off[0, -1]), int(off[1, -1])
    iws, ioff = ops.isosurface_count(vol, iso)
    iV, iT = int(ioff[0, -1]), int(ioff[1, -1])
    vert = torch.empty(max(V, iV, 1) * 3, device="cuda")
    vals = torch.empty(max(V, 1) * 2, device="cuda")
    faces = torch.empty(max(T, iT, 1) * 3, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    arr = lambda *v: (ctypes.c_double * 3)(*v)
    one = arr(1.0, 1.0, 1.0)
    runs = {
        "nodes": lambda: ops._call("fs_ridge_nodes3d", vol.data_ptr(), 1, *sp, P, 0, arr(.5, .5, .5), one, arr(.25, .25, .25),
                                   strength, fmin, operands.data_ptr(), cls.data_ptr(), stream),
        "count": lambda: ops._call("fs_ridge_count3d", operands.data_ptr(), cls.data_ptr(), 1, *sp, ws.data_ptr(), stream),
        "emit": lambda: ops._call("fs_ridge_emit3d", vol.data_ptr(), 1, *sp, P, 0, operands.data_ptr(), cls.data_ptr(), one,
                                  ws.data_ptr(), off.data_ptr(), V, T, vert.data_ptr(), vals.data_ptr(), faces.data_ptr(),
                                  status.data_ptr(), stream),
        "iso_count": lambda: ops._call("fs_iso_count3d", vol.data_ptr(), 1, *sp, P, iso, iws.data_ptr(), stream),
        "iso_emit": lambda: ops._call("fs_iso_emit3d", vol.data_ptr(), 1, *sp, P, iso, one, iws.data_ptr(), ioff.data_ptr(), iV,
                                      iT, None, 0, vert.data_ptr(), None, None, faces.data_ptr(), status.data_ptr(), stream),
    }
    for _ in range(warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    ev = [{k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in runs} for _ in range(reps)]
    for round_ in ev:
        for k, f in runs.items():
            round_[k][0].record()
            f()
            round_[k][1].record()
    torch.cuda.synchronize()
    ms = {k: pct([r[k][0].elapsed_time(r[k][1]) for r in ev]) for k in runs}
    assert int(status.cpu()[0]) == 0, "an emit pass set its status"
    runs["emit"]()
    r = ops.ridge_surfaces(vol, 1.0, strength, fmin)
    same = (bool(torch.equal(r["vertices"].reshape(-1).view(torch.int32), vert[:3 * V].view(torch.int32))) and
            bool(torch.equal(r["faces"].reshape(-1), faces[:3 * T])) and
            bool(torch.equal(r["values"].reshape(-1).view(torch.int32), vals[:2 * V].view(torch.int32))))
    counts, classes = r["counts"][0].tolist(), r["classes"][0].tolist()
    del r
    t_diff, t_eigh, t_edge, layers, active, note = stock(vol, strength, slab)
    scale = (S - 2) / layers
    bytes_ = {"nodes": ops.ridge_cost(sp, op="nodes")[0], "count": ops.ridge_cost(sp, op="count")[0],
              "emit": ops.ridge_cost(sp, 1, V, T, op="emit")[0], "iso_count": ops.isosurface_cost(sp, op="count")[0],
              "iso_emit": ops.isosurface_cost(sp, 1, iV, iT, 0, False, op="emit")[0]}
    row = {"field": kind, "shape": list(sp), "strength": strength, "fmin": fmin if fmin > -float("inf") else None,
           "vertices": V, "faces": T, "twisted": counts[2], "tetrahedra": counts[3], "classes": classes, "iso": iso,
           "iso_vertices": iV, "iso_faces": iT, "reps": reps, "same_as_op": same, "node_gflops": ops.ridge_cost(sp, op="nodes")[1] / 1e9,
           "stock_slab_layers": layers, "stock_note": note, "stock_diff_ms": t_diff, "stock_eigh_ms": t_eigh,
           "stock_edge_ms": t_edge, "stock_active_edges": active,
           "stock_ms_extrapolated": None if t_diff is None else (t_diff + t_eigh + t_edge) * scale}
    for k in ms:
        row[k + "_ms"], row[k + "_ms_p10"], row[k + "_ms_p90"] = ms[k]
        row[k + "_bytes"] = bytes_[k]
        row[k + "_share_of_roof"] = (bytes_[k] / HBM_BPS * 1e3) / ms[k][0] if ms[k][0] > 0 else None
    row["all_ms"] = ms["nodes"][0] + ms["count"][0] + ms["emit"][0]
    return row


def table(rows, args):
    lines = ["%s, %d rounds after %d warm-up rounds; median ms (p10 - p90); one volume, spacing 1; share = (algorithmic bytes / "
             "8 TB/s) over the time, warm; stock = torch fp64 differences + linalg.eigh + edge test on a slab, extrapolated "
             "linearly to the volume" % (torch.cuda.get_device_name(0), args.reps, args.warmup),
             "%-12s %-6s %-10s %28s %10s %7s  %s" % ("shape", "field", "pass", "HIP ms", "MB", "share", "note")]
    for r in rows:
        shape = "x".join(str(s) for s in r["shape"])
        notes = {"nodes": "%.1f fp64 Gflop by ops.ridge_cost: %.2f Tflop/s; classes border %d nonfinite %d weak %d low %d eligible %d" %
                          ((r["node_gflops"], r["node_gflops"] / r["nodes_ms"]) + tuple(r["classes"])),
                 "count": "%.1fx fs_iso_count3d" % (r["count_ms"] / r["iso_count_ms"]),
                 "emit": "%d vertices, %d faces, %d of %d tetrahedra twisted; %.1fx fs_iso_emit3d; same bits as ops.ridge_surfaces: %s" %
                         (r["vertices"], r["faces"], r["twisted"], r["tetrahedra"], r["emit_ms"] / r["iso_emit_ms"], r["same_as_op"]),
                 "iso_count": "fs_iso_count3d, iso = the median %.4g" % r["iso"],
                 "iso_emit": "fs_iso_emit3d without normals: %d vertices, %d faces" % (r["iso_vertices"], r["iso_faces"])}
        for k in ("nodes", "count", "emit", "iso_count", "iso_emit"):
            lines.append("%-12s %-6s %-10s %9.3f (%7.3f - %7.3f) %10.1f %7.4f  %s" % (
                shape, r["field"], k, r[k + "_ms"], r[k + "_ms_p10"], r[k + "_ms_p90"], r[k + "_bytes"] / 1e6,
                r[k + "_share_of_roof"], notes[k]))
        if r["stock_ms_extrapolated"] is None:
            stock_ = "not measured (%s)" % r["stock_note"]
        else:
            stock_ = ("differences %.1f + eigh %.1f + edge test %.1f ms on %d interior layers, EXTRAPOLATED to %.0f ms: %.0fx" %
                      (r["stock_diff_ms"], r["stock_eigh_ms"], r["stock_edge_ms"], r["stock_slab_layers"],
                       r["stock_ms_extrapolated"], r["stock_ms_extrapolated"] / r["all_ms"]))
        lines.append("%-12s %-6s %-10s %9.3f %19s %10s %7s  stock: %s" % (shape, r["field"], "all three", r["all_ms"], "", "", "", stock_))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--stock-slab", type=int, default=10, help="z-layers the torch composition runs on")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ridgebench needs a GPU"
    rows = []
    for kind in FIELDS:
        signal.alarm(CASE_LIMIT_S)
        rows.append(bench(kind, args.size, args.warmup, args.reps, min(args.stock_slab, args.size)))
        signal.alarm(0)
        torch.cuda.empty_cache()
        text = table(rows, args)
        for path, body in ((args.out, text), (args.json, json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows},
                                                                    indent=1))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        print(text, flush=True)
    assert all(r["same_as_op"] for r in rows)


if __name__ == "__main__":
    main()
