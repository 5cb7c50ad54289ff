"""Critical points on the GPU: the two passes of ops.critical_points timed one by one (fs_critical_count{2,3}d: stream
the field, test signs, form the minors of the surviving simplices; fs_critical_emit{2,3}d: gather the flagged cells and
write the table) on one step flow of 256^3, 128^3 and 2048^2 nodes, for three fields -- band-limited (few zeros), white
noise (a zero in every eighth tetrahedron, every fourth triangle) and a band-limited field that is exactly zero outside
a ball (most of the grid is quiet) -- next to fs_iso_count3d on one component of the same field in the same run: the
existing kernel with the same access pattern and a third of the bytes.

Per case: `warmup` rounds, then `reps` rounds that launch iso_count (3-D), count and emit in turn, each between two HIP
events on preallocated outputs (the prefix sum between the passes is made once, outside the timed window); the table
gives the median and the 10th / 90th percentile.  Bytes are the algorithm's (ops.critical_points_cost: count reads every
node's C components and writes a mask byte per node and two counts per row; emit reads the mask bytes and writes the
table; the corners it gathers around flagged cells come on top and are not counted), set against the 8 TB/s HBM peak
(AMD's MI355X spec): `share` is the time those bytes take at that rate over the measured time.  The timings are
WARM: the rounds repeat on one field, and a 256^3 field (201 MB) fits the 256 MB last-level cache, as every smaller one
does, so reads may be served from there and not from HBM; a first pass over a field fresh from HBM can take longer.

The stock composition on the same device, timed in turn (`--stock-reps` calls): torch slicing of a cell's 8 (4) corners,
all signed face minors of all simplices of all cells in fp64, the sign test on them, `nonzero` -- the detection alone,
without positions, Jacobians or classes.  The run FAILS if count + emit is not faster than that in a case.

    python scripts/criticalbench.py [--out profiles/critical.txt] [--json critical.json]

One process, the cases one after another, each under its own time limit (SIGALRM): a case that overruns ends the run."""
import argparse
import ctypes
import itertools
import json
import math
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402

CASE_LIMIT_S = 240
HBM_BPS = 8.0e12
SHAPES = ((256, 256, 256), (128, 128, 128), (2048, 2048))
FIELDS = ("band", "noise", "ball")


def pct(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


def field(kind, sp):
    """[1, C, *sp] fp32 on the GPU."""
    C = len(sp)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    if kind == "noise":
        return torch.randn((1, C) + sp, generator=g, device="cuda")
    grid = torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device="cuda") / s for s in sp], indexing="ij")
    cpu = torch.Generator().manual_seed(11)
    u = torch.zeros((1, C) + sp, device="cuda")
    for r in range(C):
        for _ in range(6):
            w = torch.randint(-4, 5, (C,), generator=cpu).tolist()
            a, ph = float(torch.randn((), generator=cpu)), float(torch.rand((), generator=cpu)) * 2 * math.pi
            u[0, r] += a * torch.cos(2 * math.pi * sum(wi * x for wi, x in zip(w, grid)) + ph)
    if kind == "ball":
        u *= (sum((x - 0.5) ** 2 for x in grid) <= 0.3 ** 2).to(u.dtype)
    return u


def _det(v):
    if len(v) == 3:
        a, b, c = v
        return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0])
    a, b = v
    return a[0] * b[1] - a[1] * b[0]


def stock(flows):
    """The detection in stock torch ops: [N, nd + 1] (cell coordinates, simplex) of the simplices whose signed minors all
    have one sign."""
    f = flows[0].double()
    nd = f.dim() - 1
    cs = tuple(s - 1 for s in f.shape[1:])
    hits = []
    for pi in itertools.permutations(range(nd)):
        offs = [[0] * nd]
        for a in pi:
            offs.append(list(offs[-1]))
            offs[-1][a] += 1
        v = [f[(slice(None),) + tuple(slice(o[nd - 1 - a], o[nd - 1 - a] + cs[a]) for a in range(nd))] for o in offs]
        s = [(-1.0) ** i * _det(v[:i] + v[i + 1:]) for i in range(nd + 1)]
        pos, neg = s[0] > 0, s[0] < 0
        for si in s[1:]:
            pos &= si > 0
            neg &= si < 0
        hits.append(pos | neg)
    return torch.stack(hits, -1).nonzero()


def bench(kind, sp, warmup, reps, stock_reps):
    u = field(kind, sp)
    nd, P = len(sp), math.prod(sp)
    stream = ops._stream(u)
    ws, off = ops.critical_points_count(u, 0.0)
    N = int(off[-1])
    out = {"cell": torch.empty(N, dtype=torch.int32, device="cuda"), "simplex": torch.empty(N, dtype=torch.uint8, device="cuda"),
           "pos": torch.empty((N, nd), device="cuda"), "jac": torch.empty((N, nd * nd), dtype=torch.float64, device="cuda"),
           "inv": torch.empty((N, 4), dtype=torch.float64, device="cuda"), "cls": torch.empty(N, dtype=torch.uint8, device="cuda"),
           "vmax": torch.empty(N, device="cuda")}
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    h, sc = (ctypes.c_double * nd)(*[1.0] * nd), (ctypes.c_double * 1)(1.0)
    runs = {}
    if nd == 3:
        iso_ws = torch.empty(ops._lib.lib().fs_iso3d_ws_bytes(1, *sp), dtype=torch.uint8, device="cuda")
        runs["iso_count"] = lambda: ops._call("fs_iso_count3d", u.data_ptr(), 1, *sp, P, 0.0, iso_ws.data_ptr(), stream)
    runs["count"] = lambda: ops._call("fs_critical_count%dd" % nd, u.data_ptr(), 1, nd, *sp, nd * P, 0.0, ws.data_ptr(), stream)
    if N:
        runs["emit"] = lambda: ops._call("fs_critical_emit%dd" % nd, u.data_ptr(), 1, nd, *sp, nd * P, h, sc, 0.0,
                                         ws.data_ptr(), off.data_ptr(), N, *[out[c].data_ptr() for c in
                                                                             ("cell", "simplex", "pos", "jac", "inv", "cls", "vmax")],
                                         status.data_ptr(), stream)
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
    ms.setdefault("emit", (0.0, 0.0, 0.0))
    assert int(status.cpu()[0]) == 0, "fs_critical_emit set its status"
    # the timed launches wrote what ops.critical_points returns
    r = ops.critical_points(u)
    same = all(bool(torch.equal(r[c], out[c])) for c in out)
    # the stock composition, in turn
    found = stock(u)
    torch.cuda.synchronize()
    st = []
    for _ in range(stock_reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        found = stock(u)
        e1.record()
        torch.cuda.synchronize()
        st.append(e0.elapsed_time(e1))
    bytes_ = {"count": ops.critical_points_cost(sp, 1, op="count")[0], "emit": ops.critical_points_cost(sp, 1, N, op="emit")[0],
              "iso_count": ops.isosurface_cost(sp, 1, op="count")[0] if nd == 3 else 0}
    counts = r["counts"][0].tolist()
    row = {"field": kind, "shape": list(sp), "points": N, "degenerate_simplices": counts[1], "flagged_cells": counts[3],
           "reps": reps, "same_as_op": same, "stock_ms": sorted(st)[len(st) // 2], "stock_reps": stock_reps,
           "stock_points": int(found.shape[0])}
    for k in ms:
        row[k + "_ms"], row[k + "_ms_p10"], row[k + "_ms_p90"] = ms[k]
        row[k + "_bytes"] = bytes_[k]
        row[k + "_share_of_roof"] = (bytes_[k] / HBM_BPS * 1e3) / ms[k][0] if ms[k][0] > 0 else None
    row["both_ms"] = ms["count"][0] + ms["emit"][0]
    row["speedup_over_stock"] = row["stock_ms"] / row["both_ms"]
    row["count_over_iso_count"] = ms["count"][0] / ms["iso_count"][0] if nd == 3 else None
    return row


def table(rows, args):
    lines = ["%s, %d rounds after %d warm-up rounds; median ms (p10 - p90); one step flow, spacing 1, vmin 0; share = "
             "(algorithmic bytes / 8 TB/s) over the time, warm (the rounds repeat on one field, which fits the 256 MB last-level "
             "cache); stock = torch slicing + all minors in fp64 + nonzero, median of %d" %
             (torch.cuda.get_device_name(0), args.reps, args.warmup, args.stock_reps),
             "%-12s %-6s %-10s %28s %10s %7s  %s" % ("shape", "field", "pass", "HIP ms", "MB", "share", "note")]
    for r in rows:
        shape = "x".join(str(s) for s in r["shape"])
        for k in ("iso_count", "count", "emit"):
            if k + "_ms" not in r or (k == "emit" and not r["points"]):
                continue
            note = {"iso_count": "fs_iso_count3d on component 0: the same access pattern, a third of the bytes",
                    "count": ("%.2fx fs_iso_count3d; " % r["count_over_iso_count"] if r["count_over_iso_count"] else "") +
                             "%d flagged cells, %d degenerate simplices" % (r["flagged_cells"], r["degenerate_simplices"]),
                    "emit": "%d points; same bits as ops.critical_points: %s" % (r["points"], r["same_as_op"])}[k]
            lines.append("%-12s %-6s %-10s %9.3f (%7.3f - %7.3f) %10.1f %7.3f  %s" % (
                shape, r["field"], k, r[k + "_ms"], r[k + "_ms_p10"], r[k + "_ms_p90"], r[k + "_bytes"] / 1e6,
                r[k + "_share_of_roof"], note))
        lines.append("%-12s %-6s %-10s %9.3f %19s %10s %7s  stock %.2f ms (%d simplices found): %.0fx" % (
            shape, r["field"], "both", r["both_ms"], "", "", "", r["stock_ms"], r["stock_points"], r["speedup_over_stock"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--stock-reps", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "criticalbench needs a GPU"
    rows = []
    for sp in SHAPES:
        for kind in FIELDS:
            signal.alarm(CASE_LIMIT_S)
            rows.append(bench(kind, sp, args.warmup, args.reps, args.stock_reps))
            signal.alarm(0)
            torch.cuda.empty_cache()
            text = table(rows, args)
            for path, body in ((args.out, text), (args.json, json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows},
                                                                        indent=1))):
                if path:
                    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                    with open(path, "w") as f:
                        f.write(body)
    print(table(rows, args))
    assert all(r["same_as_op"] for r in rows)
    slow = [(r["shape"], r["field"]) for r in rows if not r["both_ms"] < r["stock_ms"]]
    assert not slow, "not faster than the stock composition: %r" % (slow,)


if __name__ == "__main__":
    main()
