"""Isosurface extraction on the GPU: the two launches of ops.isosurface timed one by one (fs_iso_count3d: classify and
count; fs_iso_emit3d: gather and emit, with normals) on one 256^3 volume, for a sparse surface -- a sphere shell of radius
100 nodes, which cuts about 1 % of the cells -- and a dense one -- white noise at iso 0, which cuts every cell -- next to
fs_brick_range3d (ops.brick_ranges) on the same volume: the existing kernel with the same read traffic, untouched by the
isosurface work.

Per case: `warmup` rounds, then `reps` rounds that launch brick_range, count and emit in turn, each between two HIP events
on preallocated outputs (the prefix sum between the passes is made once, outside the timed window); the table gives the
median and the 10th / 90th percentile.  Bytes are the algorithm's (ops.isosurface_cost: count reads every node and writes
a mask byte per node and two counts per row; emit reads the mask bytes and writes the vertices, normals and faces; the
nodes it gathers around cut cells come on top and are not counted), set against the 8 TB/s HBM peak (AMD's MI355X
spec): `x roof` is the measured time over the time those bytes take at that rate.

    python scripts/isobench.py [--out profiles/isosurface.txt] [--json iso.json] [--size 256]

One process, the cases one after another, each under its own time limit (SIGALRM): a case that overruns ends the run."""
import argparse
import ctypes
import json
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import isosurface, ops  # noqa: E402

CASE_LIMIT_S = 240
HBM_BPS = 8.0e12


def pct(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


def volume(kind, S):
    if kind == "sphere":
        z, y, x = torch.meshgrid(*[torch.arange(S, dtype=torch.float32, device="cuda")] * 3, indexing="ij")
        c = 0.5 * (S - 1) + 0.3
        return ((100.0 * S / 256.0) - torch.sqrt((x - c) ** 2 + (y - c - 0.2) ** 2 + (z - c + 0.2) ** 2))[None].contiguous()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    return torch.randn((1, S, S, S), generator=g, device="cuda")


def bench(kind, S, warmup, reps):
    vol = volume(kind, S)
    sp, P = (S, S, S), S ** 3
    stream = ops._stream(vol)
    ws, off = ops.isosurface_count(vol, 0.0)
    host = off[:, -1].cpu()
    V, T = int(host[0]), int(host[1])
    vert = torch.empty((V, 3), dtype=torch.float32, device="cuda")
    nrm = torch.empty((V, 3), dtype=torch.float32, device="cuda")
    faces = torch.empty((T, 3), dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    nb = tuple((s - 1 + 7) // 8 for s in sp)
    rng = torch.empty((1,) + nb + (2,), dtype=torch.float32, device="cuda")
    flg = torch.empty((1,) + nb, dtype=torch.uint8, device="cuda")
    h = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    runs = {
        "brick_range": lambda: ops._call("fs_brick_range3d", vol.data_ptr(), 1, *sp, P, rng.data_ptr(), flg.data_ptr(), stream),
        "count": lambda: ops._call("fs_iso_count3d", vol.data_ptr(), 1, *sp, P, 0.0, ws.data_ptr(), stream),
        "emit": lambda: ops._call("fs_iso_emit3d", vol.data_ptr(), 1, *sp, P, 0.0, h, ws.data_ptr(), off.data_ptr(), V, T, 0,
                                  0, vert.data_ptr(), nrm.data_ptr(), 0, faces.data_ptr(), status.data_ptr(), stream),
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
    st = isosurface.mesh_stats(vert, faces) if kind == "sphere" else None
    assert int(status.cpu()[0]) == 0, "fs_iso_emit3d set its status"
    # the timed launches wrote what ops.isosurface returns
    r = ops.isosurface(vol, 0.0)
    same = bool(torch.equal(r["vertices"], vert) and torch.equal(r["faces"], faces) and torch.equal(r["normals"], nrm))
    bytes_ = {"brick_range": 4 * P + 9 * nb[0] * nb[1] * nb[2], "count": ops.isosurface_cost(sp, 1, op="count")[0],
              "emit": ops.isosurface_cost(sp, 1, V, T, 0, True, op="emit")[0]}
    row = {"case": kind, "volume": list(sp), "vertices": V, "faces": T, "reps": reps, "same_as_op": same,
           "boundary_edges": None if st is None else st["boundary_edges"]}
    for k in runs:
        row[k + "_ms"], row[k + "_ms_p10"], row[k + "_ms_p90"] = ms[k]
        row[k + "_bytes"] = bytes_[k]
        row[k + "_x_roof"] = ms[k][0] / (bytes_[k] / HBM_BPS * 1e3)
    row["both_ms"] = ms["count"][0] + ms["emit"][0]
    row["both_bytes"] = 4 * P + bytes_["emit"] - P  # the volume read once, the outputs written
    row["both_x_roof"] = row["both_ms"] / (row["both_bytes"] / HBM_BPS * 1e3)
    row["count_over_brick_range"] = ms["count"][0] / ms["brick_range"][0]
    return row


def table(rows, args):
    lines = ["%s, %d rounds after %d warm-up rounds; median ms (p10 - p90); one %d^3 volume, iso 0, normals on; x roof = time "
             "over (algorithmic bytes / 8 TB/s)" % (torch.cuda.get_device_name(0), args.reps, args.warmup, args.size),
             "%-7s %-12s %28s %12s %8s  %s" % ("case", "pass", "HIP ms", "MB", "x roof", "note")]
    for r in rows:
        for k in ("brick_range", "count", "emit"):
            note = {"brick_range": "fs_brick_range3d: the same read traffic",
                    "count": "%.2fx fs_brick_range3d" % r["count_over_brick_range"],
                    "emit": "%d vertices, %d faces%s; same bits as ops.isosurface: %s" % (
                        r["vertices"], r["faces"],
                        "" if r["boundary_edges"] is None else ", %d boundary edges" % r["boundary_edges"], r["same_as_op"])}[k]
            lines.append("%-7s %-12s %9.3f (%7.3f - %7.3f) %12.1f %8.2f  %s" % (
                r["case"], k, r[k + "_ms"], r[k + "_ms_p10"], r[k + "_ms_p90"], r[k + "_bytes"] / 1e6, r[k + "_x_roof"], note))
        lines.append("%-7s %-12s %9.3f %19s %12.1f %8.2f  volume read once + outputs written" % (
            r["case"], "count + emit", r["both_ms"], "", r["both_bytes"] / 1e6, r["both_x_roof"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "isobench needs a GPU"
    rows = []
    for kind in ("sphere", "noise"):
        signal.alarm(CASE_LIMIT_S)
        rows.append(bench(kind, args.size, args.warmup, args.reps))
        signal.alarm(0)
        text = table(rows, args)
        for path, body in ((args.out, text), (args.json, json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows},
                                                                    indent=1))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
    print(table(rows, args))
    assert all(r["same_as_op"] for r in rows)


if __name__ == "__main__":
    main()
