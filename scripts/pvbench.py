"""Parallel vectors on the GPU: the two passes of ops.parallel_vectors timed one by one (fs_pv_count3d: screen the 12
owned faces of every node, solve the survivors' pencils, add up the tetrahedra; fs_pv_emit3d: re-solve the faces of the
tetrahedra with two points and write the segments) on one step of 256^3 nodes, for three velocity fields -- band-limited,
the vortex ring of the tests tiled to that size, white noise -- with w = J v (--criterion levy: w = curl v) and aux = Q
from cores.core_fields, next to two things in the same run:
  * fs_critical_count3d on the same velocity field: its nearest neighbour in traffic (3 of the 6 planes, the same rows);
  * the stock composition in torch: the same Bernstein reject on every owned face of every cell (fp64 slicing, slot by
    slot, at full size -- it also gives the share of faces that survive step 2), then torch.linalg.solve and batched
    torch.linalg.eigvals on the survivors.  The eigenvalue stage is timed on a SAMPLE of at most --eig-sample surviving
    faces and extrapolated linearly to all of them; the table says so.  Detection only: no acceptance test, no
    positions.  Where torch cannot run it on this device the table says "not measured" and why.

Per case: `warmup` rounds, then `reps` rounds that launch critical_count, count and emit in turn, each between two HIP
events on preallocated outputs (the prefix sum between the passes is made once, outside the timed window); the table
gives the median and the 10th / 90th percentile.  Bytes are the algorithm's (ops.parallel_vectors_cost), set against the
8 TB/s HBM peak (AMD's MI355X spec): `share` is the time those bytes take at that rate over the measured time.  The
timings are WARM: the rounds repeat on one pair of fields (403 MB), which does not fit the 256 MB last-level cache whole
but is partly served from it.  The kernel is bound by fp64 VALU work, not by bytes: the share says how far from the roof
that leaves it.

    python scripts/pvbench.py [--out profiles/pv.txt] [--json pv.json] [--size 256]

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
from opticalflowscivis_amd import cores, ops  # noqa: E402

CASE_LIMIT_S = 280
HBM_BPS = 8.0e12
FIELDS = ("band", "ring", "noise")
MID = (1, 1, 2, 2, 4, 4, 3, 5, 6, 1, 2, 4)  # include/flowsci_hip.h: the corners 0 < mid < hi of a node's 12 slots
HI = (3, 5, 3, 6, 5, 6, 7, 7, 7, 7, 7, 7)


def pct(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


def field(kind, S):
    """[1, 3, S, S, S] fp32 on the GPU."""
    sp = (S, S, S)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    if kind == "noise":
        return torch.randn((1, 3) + sp, generator=g, device="cuda")
    if kind == "ring":  # the ring of tests/pv_fields.py on its 10 x 14 x 15 grid, tiled
        z, y, x = torch.meshgrid(*[torch.arange(s, dtype=torch.float64, device="cuda") for s in (10, 14, 15)], indexing="ij")
        rho = torch.sqrt((x - 7.2) ** 2 + (y - 6.6) ** 2)
        s, h = rho - 4.0, z - 4.4
        gs = torch.exp(-(s * s + h * h) / (2.0 * 1.5 ** 2))
        er, ephi = ((x - 7.2) / rho, (y - 6.6) / rho), (-(y - 6.6) / rho, (x - 7.2) / rho)
        u = torch.stack([gs * -h * er[0] + 0.3 * gs * ephi[0], gs * -h * er[1] + 0.3 * gs * ephi[1], gs * s + 0.2]).float()
        reps = [1] + [-(-S // n) for n in (10, 14, 15)]
        return u.repeat(*reps)[None, :, :S, :S, :S].contiguous()
    grid = torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device="cuda") / s for s in sp], indexing="ij")
    cpu = torch.Generator().manual_seed(11)
    u = torch.zeros((1, 3) + sp, device="cuda")
    for r in range(3):
        for _ in range(6):
            w = torch.randint(-4, 5, (3,), generator=cpu).tolist()
            a, ph = float(torch.randn((), generator=cpu)), float(torch.rand((), generator=cpu)) * 2 * math.pi
            u[0, r] += a * torch.cos(2 * math.pi * sum(wi * x for wi, x in zip(w, grid)) + ph)
    return u


def _corner(f, c):
    """The values at corner c of every cell: [3, D-1, H-1, W-1] fp64."""
    dz, dy, dx = c >> 2 & 1, c >> 1 & 1, c & 1
    D, H, W = f.shape[1:]
    return f[:, dz:dz + D - 1, dy:dy + H - 1, dx:dx + W - 1].double()


def _survivors(v, w, s):
    """Step 2 on slot s of every cell (the faces owned by border nodes that are no cell's origin are left out): the
    mask of the faces that are not rejected, and their corner values."""
    cs = (0, MID[s], HI[s])
    V, W = [_corner(v, c) for c in cs], [_corner(w, c) for c in cs]
    out = torch.zeros(V[0].shape[1:], dtype=torch.bool, device=v.device)
    for k in range(3):
        j, l = (k + 1) % 3, (k + 2) % 3
        x = lambda p, q: V[p][j] * W[q][l] - V[p][l] * W[q][j]
        six = torch.stack([x(0, 0), x(1, 1), x(2, 2), x(0, 1) + x(1, 0), x(0, 2) + x(2, 0), x(1, 2) + x(2, 1)])
        out |= (six > 0).all(0) | (six < 0).all(0)
    return ~out, V, W


def stock(v, w, eig_sample):
    """(faces, survivors, reject ms, eigenvalue ms on the sample, sample size, note)."""
    faces = surv = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sample = None
    for s in range(12):
        keep, V, W = _survivors(v[0], w[0], s)
        faces += keep.numel()
        surv += int(keep.sum())
        if s == 0:
            at = keep.reshape(-1).nonzero()[:eig_sample, 0]
            sample = [torch.stack([c.reshape(3, -1)[:, at] for c in X], -1).permute(1, 0, 2).contiguous() for X in (V, W)]
        del keep, V, W
    e1.record()
    torch.cuda.synchronize()
    t_reject = e0.elapsed_time(e1)
    n = int(sample[0].shape[0])
    if n == 0:
        return faces, surv, t_reject, None, 0, "no survivor in slot 0"
    try:
        e0.record()
        lam = torch.linalg.eigvals(torch.linalg.solve(sample[1], sample[0]))  # A = w, B = v: det(B - x A) = 0
        e1.record()
        torch.cuda.synchronize()
        return faces, surv, t_reject, e0.elapsed_time(e1), n, "%d real" % int((lam.imag == 0).sum())
    except Exception as e:  # (a device without a batched nonsymmetric eigensolver)
        return faces, surv, t_reject, None, n, "%s: %s" % (type(e).__name__, str(e).split("\n")[0][:120])


def bench(kind, S, criterion, warmup, reps, eig_sample):
    u = field(kind, S)
    sp, P = (S, S, S), S ** 3
    cf = cores.core_fields(u, criterion)
    v, w, aux = cf["v"], cf["w"].contiguous(), cf["q"].contiguous()
    del cf
    stream = ops._stream(v)
    ws, off = ops.parallel_vectors_count(v, w, aux)
    N = int(off[-1])
    cols = {"cell": (1, torch.int32), "simplex": (1, torch.uint8), "face": (2, torch.uint8), "key": (2, torch.int64),
            "pos": (6, torch.float32), "mu": (2, torch.float64), "vel": (6, torch.float32), "aux": (2, torch.float32)}
    out = {c: torch.empty(max(N, 1) * k, dtype=dt, device="cuda") for c, (k, dt) in cols.items()}
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    h = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    fields = (v.data_ptr(), 3 * P, w.data_ptr(), 3 * P, aux.data_ptr(), P)
    cws = torch.empty(ops._lib.lib().fs_critical3d_ws_bytes(1, *sp), dtype=torch.uint8, device="cuda")
    runs = {"critical_count": lambda: ops._call("fs_critical_count3d", v.data_ptr(), 1, 3, *sp, 3 * P, 0.0, cws.data_ptr(), stream),
            "count": lambda: ops._call("fs_pv_count3d", *fields, 1, *sp, 0.0, 0.0, ws.data_ptr(), stream)}
    if N:
        runs["emit"] = lambda: ops._call("fs_pv_emit3d", *fields, 1, *sp, h, 0.0, 0.0, ws.data_ptr(), off.data_ptr(), N,
                                         *[out[c].data_ptr() for c in cols], status.data_ptr(), stream)
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
    assert int(status.cpu()[0]) == 0, "fs_pv_emit3d set its status"
    r = ops.parallel_vectors(v, w, aux)
    same = all(bool(torch.equal(r[c].reshape(-1).view(torch.uint8), out[c][:N * cols[c][0]].view(torch.uint8))) for c in cols)
    counts = r["counts"][0].tolist()
    del r
    faces, surv, t_reject, t_eig, n_eig, note = stock(v, w, eig_sample)
    bytes_ = {"count": ops.parallel_vectors_cost(sp, 1, op="count", aux=True)[0],
              "emit": ops.parallel_vectors_cost(sp, 1, N, op="emit", aux=True)[0],
              "critical_count": ops.critical_points_cost(sp, 1, op="count")[0]}
    row = {"field": kind, "shape": list(sp), "criterion": criterion, "segments": N, "ambiguous_tets": counts[1],
           "degenerate_faces": counts[2], "reps": reps, "same_as_op": same, "faces": faces, "survivors": surv,
           "survivor_share": surv / faces, "stock_reject_ms": t_reject, "stock_eig_sample": n_eig,
           "stock_eig_sample_ms": t_eig, "stock_note": note,
           "stock_eig_ms_extrapolated": None if t_eig is None else t_eig * surv / n_eig}
    for k in ms:
        row[k + "_ms"], row[k + "_ms_p10"], row[k + "_ms_p90"] = ms[k]
        row[k + "_bytes"] = bytes_[k]
        row[k + "_share_of_roof"] = (bytes_[k] / HBM_BPS * 1e3) / ms[k][0] if ms[k][0] > 0 else None
    row["both_ms"] = ms["count"][0] + ms["emit"][0]
    row["count_over_critical_count"] = ms["count"][0] / ms["critical_count"][0]
    return row


def table(rows, args):
    lines = ["%s, %d rounds after %d warm-up rounds; median ms (p10 - p90); one step, spacing 1, vmin = wmin = 0, aux = Q, "
             "criterion %s; share = (algorithmic bytes / 8 TB/s) over the time, warm; stock = torch fp64 reject at full size + "
             "solve and linalg.eigvals on a sample of the survivors of slot 0, extrapolated to all survivors" %
             (torch.cuda.get_device_name(0), args.reps, args.warmup, args.criterion),
             "%-12s %-6s %-15s %28s %10s %7s  %s" % ("shape", "field", "pass", "HIP ms", "MB", "share", "note")]
    for r in rows:
        shape = "x".join(str(s) for s in r["shape"])
        for k in ("critical_count", "count", "emit"):
            if k == "emit" and not r["segments"]:
                continue
            note = {"critical_count": "fs_critical_count3d on v: the same rows, half the planes",
                    "count": "%.1fx fs_critical_count3d; %.1f %% of %d faces survive step 2" %
                             (r["count_over_critical_count"], 100 * r["survivor_share"], r["faces"]),
                    "emit": "%d segments, %d ambiguous tetrahedra, %d degenerate faces; same bits as ops.parallel_vectors: %s" %
                            (r["segments"], r["ambiguous_tets"], r["degenerate_faces"], r["same_as_op"])}[k]
            lines.append("%-12s %-6s %-15s %9.3f (%7.3f - %7.3f) %10.1f %7.4f  %s" % (
                shape, r["field"], k, r[k + "_ms"], r[k + "_ms_p10"], r[k + "_ms_p90"], r[k + "_bytes"] / 1e6,
                r[k + "_share_of_roof"], note))
        if r["stock_eig_ms_extrapolated"] is None:
            stock_ = "reject %.1f ms; eigenvalues not measured (%s)" % (r["stock_reject_ms"], r["stock_note"])
        else:
            total = r["stock_reject_ms"] + r["stock_eig_ms_extrapolated"]
            stock_ = "reject %.1f ms + eigvals %.1f ms (EXTRAPOLATED from %.1f ms for %d faces, %s) = %.0f ms: %.0fx" % (
                r["stock_reject_ms"], r["stock_eig_ms_extrapolated"], r["stock_eig_sample_ms"], r["stock_eig_sample"],
                r["stock_note"], total, total / r["both_ms"])
        lines.append("%-12s %-6s %-15s %9.3f %19s %10s %7s  stock: %s" % (shape, r["field"], "both", r["both_ms"], "", "", "",
                                                                          stock_))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table here")
    ap.add_argument("--json", default=None, help="write the rows as JSON here")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--criterion", choices=cores.CRITERIA, default="sujudi-haimes")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--eig-sample", type=int, default=1 << 16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pvbench needs a GPU"
    rows = []
    for kind in FIELDS:
        signal.alarm(CASE_LIMIT_S)
        rows.append(bench(kind, args.size, args.criterion, args.warmup, args.reps, args.eig_sample))
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
