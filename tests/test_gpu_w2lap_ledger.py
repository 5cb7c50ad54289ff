"""GPU (-m gpu): every row of the ledger of the 2-D warp, occlusion and Laplacian-pyramid kernels (tests/w2lap_ledger.py)
on the device.

Per row: one raw ctypes call of the C-ABI entry point with the row's inputs at the row's misalignments; the launched
kernels recorded with torch.profiler must be the row's compute kernels and no other kernel of warp2d.hip / laplacian.hip /
laplacian3d.hip; status 0; every output within the row's band of the fp64 reference, or equal to the exact expectation
(occlusion masks, sgn bit for bit, the loss and sgn of input == target), at EVERY element; every output, workspace and
zero-filled accumulator lives inside 4096-float guard bands of a NaN bit pattern that must be bitwise unchanged afterwards.
Fully overwritten outputs start as that pattern (an element a dropped second trip never writes fails the comparison),
grad_in / grad_img* start at zero as the ABI requires; an aliased pair passes one buffer twice and expects the sum of both
gradients in it.  Backward rows run twice into fresh buffers and require equal bits of grad_flow / grad_diff.  A summary
line per row (kernels, errors over band, time) is printed.

The argument errors these entry points define are refused with their status before anything is launched or written."""
import ctypes
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2lap_ledger as LG  # noqa: E402
from ledger_harness import DEV, Guarded, kernels_launched, load_lib, on_device, stream as _stream  # noqa: E402
import w2lap_ledger_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

FS_ERR_NULLPTR, FS_ERR_SHAPE, FS_ERR_ARG = 1, 2, 3
KNOWN = {k for r in LG.ROWS for k in LG.kernels_of(r)} | set(LG.UNREACHABLE) | LG.HELPERS


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _kernels_launched(fn):
    """(fn's return value, normalized names of the kernels of the three sources it launched); one the ledger does not know
    is an error."""
    return kernels_launched(fn, LG.normalize, lambda n: n in KNOWN or n.startswith(LG.PREFIXES), KNOWN)


class Call:
    """Device operands, guarded outputs and the launch of one row.  `a` holds the arguments the launch passes (the row's;
    the refusal test overrides some of them after the buffers are made)."""

    def __init__(self, lib, r, T):
        self.lib, self.r, self.a = lib, r, dict(r, drop_gin1=False)
        op, m, B, C = r["op"], r["mis"], r["B"], r["C"]
        self.D = {name: on_device(t, m.get(name, 0)) for name, t in T.items()}
        self.bufs = {}
        G = lambda name, n, zero=False: self.bufs.__setitem__(name, Guarded(n, zero=zero, mis=m.get(name, 0)))
        if op in LG.WARP_OPS:
            npair = 2 if op in LG.PAIR_OPS else 1
            nf, ni = I.numel(r["ext"]), I.numel(I.img_ext(r))
            if op in ("w_fwd", "wp_fwd"):
                for i in range(npair):
                    G("out%d" % i, B * C * nf)
            else:
                if r["gflow"]:
                    G("gflow", B * 2 * npair * nf)
                if r["gin"]:
                    for i in range(1 if r["alias"] else npair):
                        G("gin%d" % i, B * C * ni, zero=True)
        elif op == "occ":
            G("occ_f", B * I.numel(r["ext"]))
            G("occ_b", B * I.numel(r["ext"]))
        else:
            out = [ctypes.c_longlong(0) for _ in range(3)]
            fn = lib.fs_laploss2d_sizes if len(r["ext"]) == 2 else lib.fs_laploss3d_sizes
            assert fn(B, *r["ext"], r["levels"], *[ctypes.byref(o) for o in out]) == 0
            sgn_n, ws_fwd, ws_bwd = (o.value for o in out)
            assert (sgn_n, ws_fwd, ws_bwd) == I.lap_sizes(r)[1:]
            if op.endswith("fwd"):
                G("sgn", sgn_n)
                G("ws", ws_fwd)
                G("loss", 2)
            else:
                G("ws", ws_bwd)
                G("gdiff", B * I.numel(r["ext"]))

    def p(self, name):
        if name in self.bufs:
            return self.bufs[name].ptr()
        return self.D[name].data_ptr() if name in self.D else None

    def launch(self):
        lib, a, p, st = self.lib, self.a, self.p, _stream()
        op, B, C = a["op"], a["B"], a["C"]
        hw = (ctypes.c_int * 2)(*a["inp"]) if a["inp"] else None
        gflow = p("gflow") if a["gflow"] else None
        gin0 = p("gin0") if a["gin"] else None
        gin1 = None if (not a["gin"] or a["drop_gin1"]) else (p("gin0") if a["alias"] else p("gin1"))
        start = p("start") if a["start"] else None
        if op == "w_fwd":
            return lib.fs_warp2d_fwd(p("in0"), p("flow"), start, p("out0"), B, C, hw, *a["ext"], a["mode"], a["mask"], st)
        if op == "w_bwd":
            return lib.fs_warp2d_bwd(p("in0"), p("flow"), start, p("gout0"), gin0, gflow, B, C, hw, *a["ext"], a["mode"],
                                     a["mask"], st)
        if op == "wp_fwd":
            return lib.fs_warp2d_pair_fwd(p("in0"), p("in1"), p("flow"), p("out0"), p("out1"), B, C, hw, *a["ext"],
                                          a["mode"], st)
        if op == "wp_bwd":
            return lib.fs_warp2d_pair_bwd(p("in0"), p("in1"), p("flow"), p("gout0"), p("gout1"), gin0, gin1, gflow, B, C,
                                          hw, *a["ext"], a["mode"], st)
        if op == "occ":
            return lib.fs_occ_check2d(p("flow_f"), p("flow_b"), p("occ_f"), p("occ_b"), B, *a["ext"], I.ALPHA1, I.ALPHA2S,
                                      a["mode"], st)
        nd2 = len(a["ext"]) == 2
        if op.endswith("fwd"):
            fn = lib.fs_laploss2d_fwd if nd2 else lib.fs_laploss3d_fwd
            return fn(p("input"), p("target"), p("sgn"), p("ws"), p("loss"), B, *a["ext"], a["levels"], st)
        fn = lib.fs_laploss2d_bwd if nd2 else lib.fs_laploss3d_bwd
        return fn(p("sgn"), p("gl"), p("ws"), p("gdiff"), B, *a["ext"], a["levels"], st)

    def got(self, name):
        t = self.bufs[name].t
        return t[:1] if name == "loss" else t


RERUN = {"w_bwd": "gflow", "wp_bwd": "gflow", "l2_bwd": "gdiff", "l3_bwd": "gdiff"}


@pytest.mark.parametrize("r", LG.ROWS, ids=[LG.row_id(r) for r in LG.ROWS])
def test_ledger_row(lib, r):
    t0 = time.perf_counter()
    T = I.data(r)
    ref = I.results(r, T, torch.float64)
    call = Call(lib, r, T)
    rc, launched = _kernels_launched(call.launch)
    assert rc == 0, "status %d" % rc
    compute = [n for n in launched if n not in LG.HELPERS]
    want = LG.kernels_of(r)
    assert set(compute) == set(want), "expected %s, launched %s" % (want, launched)
    if r["op"] in LG.WARP_OPS or r["op"] == "occ":
        assert compute == list(want), "expected one launch each of %s in this order, launched %s" % (want, launched)
    else:  # a pyramid launches its two kernels once per level
        assert compute == list(want) * r["levels"], "expected %d x %s, launched %s" % (r["levels"], want, launched)
    errs = {}
    for name, (rf, tol) in ref.items():
        g = call.got(name).detach().cpu()
        if tol is None:
            same = torch.equal(g.view(torch.int32), rf.float().reshape(-1).view(torch.int32)) if name == "sgn" else \
                torch.equal(g, rf.float().reshape(-1))
            errs[name] = 0.0 if same else float("inf")
            if not same:
                print("EXACT %s differs at %d of %d elements" % (name, int((g != rf.float().reshape(-1)).sum()), g.numel()))
        else:
            g = g.double()
            errs[name] = float("inf") if not bool(torch.isfinite(g).all()) else \
                float((g - rf.reshape(-1)).abs().max()) / I.band(rf, tol)
    again = None
    if r["op"] in RERUN and RERUN[r["op"]] in call.bufs:
        twin = Call(lib, r, T)
        assert twin.launch() == 0
        torch.cuda.synchronize()
        name = RERUN[r["op"]]
        again = torch.equal(call.bufs[name].t.view(torch.int32), twin.bufs[name].t.view(torch.int32))
        assert all(b.intact() for b in twin.bufs.values()), "the second run wrote outside its buffers"
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("LEDGER %-7s %-66s err/band %s  %.2fs  %s" % (r["op"], "+".join(want), " ".join("%s=%.3f" % kv for kv in
                                                                                         sorted(errs.items())), dt, r["why"]))
    bad_guard = [name for name, b in call.bufs.items() if not b.intact()]
    assert not bad_guard, "writes outside %s" % bad_guard
    assert errs and all(e <= 1.0 for e in errs.values()), errs
    assert again is not False, "two runs of the same backward differ in the bits of %s" % RERUN[r["op"]]


# ---- argument errors are refused before anything is launched or written ---------------------------------------------
def _twin(op, **kw):
    """A legal row whose buffers and inputs the refused call uses."""
    n = len(LG.ROWS)
    LG._row(op, "-", "refusal", kw.pop("ext"), **kw)
    r = LG.ROWS[-1]
    del LG.ROWS[n:]
    return r


def _refusals():
    w = dict(ext=(5, 9), B=2, C=3)
    return [
        ("with_mask on a non-PWC mode", _twin("w_fwd", mask=1, **w), dict(mode=LG.RIFE), FS_ERR_ARG),
        ("with_mask on DILATED, backward", _twin("w_bwd", mask=1, gin=True, **w), dict(mode=LG.DILATED), FS_ERR_ARG),
        ("start on a non-DILATED mode", _twin("w_fwd", mode=LG.DILATED, start=True, **w), dict(mode=LG.PWC), FS_ERR_ARG),
        ("in_hw differs outside RIFE", _twin("w_fwd", mode=LG.RIFE, inp=(7, 11), **w), dict(mode=LG.PHOTO), FS_ERR_ARG),
        ("in_hw differs outside RIFE, pair backward", _twin("wp_bwd", mode=LG.RIFE, inp=(7, 11), gin=True, **w),
         dict(mode=LG.PWC), FS_ERR_ARG),
        ("RIFE with H = 1", _twin("w_fwd", ext=(1, 7), B=2, C=2, flow="small"), dict(mode=LG.RIFE), FS_ERR_SHAPE),
        ("mode 4", _twin("w_fwd", **w), dict(mode=4), FS_ERR_ARG),
        ("mode 4, pair backward", _twin("wp_bwd", mode=LG.RIFE, gin=True, **w), dict(mode=4), FS_ERR_ARG),
        ("both gradients NULL", _twin("w_bwd", **w), dict(gflow=False), FS_ERR_NULLPTR),
        ("both gradients NULL, pair", _twin("wp_bwd", mode=LG.RIFE, **w), dict(gflow=False), FS_ERR_NULLPTR),
        ("a pair with one grad_img NULL", _twin("wp_bwd", mode=LG.RIFE, gin=True, **w), dict(drop_gin1=True),
         FS_ERR_NULLPTR),
        ("occ mode 3", _twin("occ", ext=(6, 11), B=2, C=2, mode=LG.OCC_OUT, flow="integer"), dict(mode=3), FS_ERR_ARG),
        ("levels 0", _twin("l2_fwd", ext=(16, 16), levels=1), dict(levels=0), FS_ERR_SHAPE),
        ("levels 9", _twin("l2_bwd", ext=(16, 16), levels=1), dict(levels=9), FS_ERR_SHAPE),
        ("levels 0, 3-D", _twin("l3_bwd", ext=(5, 6, 7), levels=1), dict(levels=0), FS_ERR_SHAPE),
        ("levels 9, 3-D", _twin("l3_fwd", ext=(5, 6, 7), levels=1), dict(levels=9), FS_ERR_SHAPE),
        ("16 x 16 at levels 5", _twin("l2_fwd", ext=(16, 16), levels=2), dict(levels=5), FS_ERR_SHAPE),
        ("16 x 16 at levels 5, backward", _twin("l2_bwd", ext=(16, 16), levels=2), dict(levels=5), FS_ERR_SHAPE),
        ("3-D extent 2", _twin("l3_fwd", ext=(3, 4, 4), levels=1), dict(ext=(2, 4, 4)), FS_ERR_SHAPE),
        ("3-D extent 2, backward", _twin("l3_bwd", ext=(4, 4, 3), levels=1), dict(ext=(4, 4, 2)), FS_ERR_SHAPE),
    ]


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_argument_errors_are_refused(lib, case):
    _, r, over, status = case
    call = Call(lib, r, I.data(r))
    call.a.update(over)
    rc, launched = _kernels_launched(call.launch)
    assert rc == status, rc
    assert launched == [], launched
    for name, b in call.bufs.items():
        if name.startswith("gin"):
            assert b.intact() and bool((b.t == 0).all()), "%s was written" % name
        else:
            assert b.untouched(), "%s was written" % name
