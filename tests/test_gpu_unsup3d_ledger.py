"""GPU (-m gpu): every row of the ledger of the unsupervised 3-D loss kernels (tests/unsup3d_ledger.py) on the device.

Per row: one raw ctypes call of the C-ABI entry point with the row's inputs at the row's misalignments; the launched
kernels recorded with torch.profiler must be the row's compute kernel (plus the reduction finish for the smoothness
forward) and no other kernel of census3d.hip / flowsmooth3d.hip; status 0; every output element within its OWN band
tol * s_i of the fp64 reference (exactly 0 where the scale s_i is 0), sums[1] equal to the float nearest the pair count,
and equal to the exact expectations (equal volumes, zero blocks of grad_dist, constant volumes, coef == 0, no pair).
Every output, `sums` and `ws` lives inside 4096-float guard bands of a NaN bit pattern that must be bitwise unchanged
afterwards; they all start as that pattern (an unwritten element fails the comparison, a workspace element read without
having been written poisons the sums), and `ws` and `sums` have exactly the size the header documents.  Nullable outputs
that are not asked for are passed as NULL.  Backward rows run twice and must give equal bits; a row with a twin (the aligned
call of a misaligned one, the NULL-guide call of a guide that must not be read) must give the twin's bits.  A summary line
per row (kernel, worst error over band per output, time) is printed.

The argument errors the header defines for these entry points are refused with their status before anything is launched
or written."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unsup3d_ledger as LG  # noqa: E402
from ledger_harness import Guarded, kernels_launched, load_lib, normalize, on_device, stream as _stream  # noqa: E402
import unsup3d_ledger_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

FS_ERR_NULLPTR, FS_ERR_SHAPE, FS_ERR_ARG = 1, 2, 3
# how the kernels of the two sources are named: a launched kernel of that kind that is not a ledger symbol is an error
PREFIXES = ("census3d_", "flow_smooth3d_")
KNOWN = {k for r in LG.ROWS for k in LG.kernels_of(r)} | set(LG.UNREACHABLE) | LG.HELPERS

# entry point and argument names (pointers: an input of unsup3d_ledger_inputs.data or an output of out_sizes, NULL when the
# row has neither; the rest: scalars of the row)
SIG = {
    "cen_fwd": ("fs_census3d_dist_fwd", "vol1 vol2 dist B D H W R"),
    "cen_bwd": ("fs_census3d_dist_bwd", "vol1 vol2 gdist g1 g2 B D H W R"),
    "fs_fwd": ("fs_flow_smooth3d_fwd", "flow guide sums ws B C D H W q eps kappa"),
    "fs_bwd": ("fs_flow_smooth3d_bwd", "flow guide coef gflow B C D H W q eps kappa"),
}
SCALARS = ("B", "C", "D", "H", "W", "R", "q", "eps", "kappa")
# the pointers each entry point requires (FS_ERR_NULLPTR when one is NULL)
REQUIRED = {"cen_fwd": "vol1 vol2 dist", "cen_bwd": "vol1 vol2 gdist", "fs_fwd": "flow sums ws", "fs_bwd": "flow coef gflow"}


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _kernels_launched(fn):
    """(fn's return value, normalized names of the kernels of the two sources it launched); one the ledger does not know
    is an error."""
    return kernels_launched(fn, normalize, lambda n: n in KNOWN or n.startswith(PREFIXES), KNOWN)


class Call:
    """Device operands, guarded outputs and the launch of one row."""

    def __init__(self, lib, r, T):
        self.lib, self.r = lib, r
        m = r["mis"]
        self.D = {name: on_device(t, m.get(name, 0)) for name, t in T.items()}
        self.mis = m
        self.fresh()
        assert not set(self.D) & set(self.bufs)

    def fresh(self):
        self.bufs = {name: Guarded(n, mis=self.mis.get(name, 0)) for name, n in I.out_sizes(self.r).items()}

    def argv(self, over=None):
        over = over or {}
        out = []
        for name in SIG[self.r["op"]][1].split():
            if name in over:
                out.append(over[name])
            elif name in SCALARS:
                out.append(self.r[name])
            elif name in self.bufs:
                out.append(self.bufs[name].ptr())
            else:
                out.append(self.D[name].data_ptr() if name in self.D else None)
        return out

    def launch(self, over=None):
        return getattr(self.lib, SIG[self.r["op"]][0])(*self.argv(over), _stream())

    def got(self, name):
        """The output as a CPU tensor (sumK is sums[K])."""
        if name.startswith("sum"):
            k = int(name[3:])
            return self.bufs["sums"].t[k:k + 1].detach().cpu().view(())
        return self.bufs[name].t.detach().cpu()

    def intact(self):
        return [name for name, b in self.bufs.items() if not b.intact()]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("r", LG.ROWS, ids=[LG.row_id(r) for r in LG.ROWS])
def test_ledger_row(lib, r):
    t0 = time.perf_counter()
    T = I.data(r)
    ref = I.results(r, T, torch.float64)
    call = Call(lib, r, T)
    for name, a in zip(SIG[r["op"]][1].split(), call.argv()):  # NULL exactly where the row has no such operand
        if name not in SCALARS:
            assert (a is None) == (name not in T and name not in call.bufs), name
    rc, launched = _kernels_launched(call.launch)
    assert rc == 0, "status %d" % rc
    compute = [n for n in launched if n not in LG.HELPERS]
    want = LG.kernels_of(r)
    assert tuple(compute) == want, "expected %s, launched %s" % (want, launched)
    finishes = 1 if r["op"] == "fs_fwd" else 0
    assert len(launched) - len(compute) == finishes, "expected %d x %s, launched %s" % (finishes, sorted(LG.HELPERS), launched)
    got = {name: call.got(name) for name in ref}
    errs, off_zero, inexact = {}, {}, []
    for name, (rf, scale, tol) in ref.items():
        errs[name], off_zero[name] = I.compare(got[name], rf, scale, tol)
    for name, (want_x, mask) in I.exact(r, T).items():
        g, w = got[name].reshape(-1), want_x.reshape(-1)
        if mask is not None:
            g, w = g[mask.reshape(-1)], w[mask.reshape(-1)]
        if not torch.equal(g, w):
            inexact.append("%s: %d of %d elements differ, the largest by %.3g" % (name, int((g != w).sum()), g.numel(),
                                                                                 float((g - w).abs().max())))
    bad_guard = call.intact()
    if r["op"].endswith("bwd"):  # bit-reproducible: a second run into fresh buffers
        call.fresh()
        assert call.launch() == 0
        torch.cuda.synchronize()
        bad_guard += call.intact()
        for name in ref:
            if not torch.equal(_bits(call.got(name)), _bits(got[name])):
                inexact.append("%s: the second run gave other bits" % name)
    twin = LG.twin_of(r)
    if twin is not None:
        other = Call(lib, twin, I.data(twin))
        assert other.launch() == 0
        torch.cuda.synchronize()
        bad_guard += other.intact()
        for name in ref:
            if not torch.equal(_bits(other.got(name)), _bits(got[name])):
                inexact.append("%s: other bits than the twin row %s" % (name, LG.row_id(twin)))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("LEDGER %-8s %-26s err/band %s  %.2fs  %s" % (r["op"], "+".join(want), " ".join("%s=%.3f" % kv for kv in
                                                                                       sorted(errs.items())), dt, r["why"]))
    assert not bad_guard, "writes outside %s" % bad_guard
    assert errs and all(e <= 1.0 for e in errs.values()), errs
    assert not any(off_zero.values()), "elements of scale 0 that are not exactly 0: %s" % off_zero
    assert not inexact, inexact
    covered = {("sums" if n.startswith("sum") else n) for n in ref}
    assert covered == set(call.bufs) - {"ws"}, "outputs without a comparison: %s" % sorted(set(call.bufs) - covered)


# ---- argument errors are refused before anything is launched or written ---------------------------------------------
def _base_rows():
    """Legal calls with full-size buffers; "grid" is the census forward whose B alone is beyond the grid limit."""
    return {
        "cen_fwd": LG.make("cen_fwd", "refusal", D=2, H=3, W=4, R=1, kind="apart"),
        "cen_bwd": LG.make("cen_bwd", "refusal", D=2, H=3, W=4, R=1, kind="apart", grads=("g1", "g2")),
        "fs_fwd": LG.make("fs_fwd", "refusal", B=2, C=2, D=3, H=4, W=5, kind="mix", guide=True, kappa=12.5),
        "fs_bwd": LG.make("fs_bwd", "refusal", B=2, C=2, D=3, H=4, W=5, kind="mix", guide=True, kappa=12.5),
        "grid_fwd": LG.make("cen_fwd", "refusal", B=LG.GRID_Z + 1, R=1, kind="apart"),
        "grid_bwd": LG.make("cen_bwd", "refusal", B=LG.GRID_Z + 1, R=1, kind="apart", grads=("g1", "g2")),
    }


def _refusals():
    """(base row, what, {argument: value}, status) -- each argument error the header defines for these entry points; the
    source returns every one of them before its launch."""
    out = []
    for op, names in REQUIRED.items():
        out += [(op, "%s NULL" % name, {name: None}, FS_ERR_NULLPTR) for name in names.split()]
    out.append(("cen_bwd", "both gradients NULL", {"g1": None, "g2": None}, FS_ERR_NULLPTR))
    for op in ("cen_fwd", "cen_bwd"):
        out += [(op, "radius 0", {"R": 0}, FS_ERR_ARG), (op, "radius 4", {"R": 4}, FS_ERR_ARG)]
        out += [(op, "%s = 0" % k, {k: 0}, FS_ERR_SHAPE) for k in "BDHW"]
    out += [("grid_fwd", "B = 65536", {}, FS_ERR_SHAPE), ("grid_bwd", "B = 65536", {}, FS_ERR_SHAPE)]
    for op in ("fs_fwd", "fs_bwd"):
        out += [(op, "%s = 0" % k, {k: 0}, FS_ERR_SHAPE) for k in "BCDHW"]
        out += [(op, "q = 0", {"q": 0.0}, FS_ERR_ARG), (op, "q < 0", {"q": -0.25}, FS_ERR_ARG),
                (op, "q = NaN", {"q": float("nan")}, FS_ERR_ARG), (op, "q = inf", {"q": float("inf")}, FS_ERR_ARG),
                (op, "kappa < 0", {"kappa": -1.0}, FS_ERR_ARG), (op, "kappa = NaN", {"kappa": float("nan")}, FS_ERR_ARG),
                (op, "kappa = inf", {"kappa": float("inf")}, FS_ERR_ARG),
                (op, "eps = 0", {"eps": 0.0}, FS_ERR_ARG),
                (op, "eps = 1e-20, its square is subnormal", {"eps": 1e-20}, FS_ERR_ARG),
                (op, "eps = 1e20, its square is infinite", {"eps": 1e20}, FS_ERR_ARG),
                (op, "eps = NaN", {"eps": float("nan")}, FS_ERR_ARG)]
    return out


def test_argument_errors_are_refused(lib):
    rows = _base_rows()
    calls = {op: Call(lib, r, I.data(r)) for op, r in rows.items()}
    cases = _refusals()
    assert {op for op, _, _, _ in cases} == set(rows)

    def run():
        return [(op, what, status, calls[op].launch(over)) for op, what, over, status in cases]

    results, launched = _kernels_launched(run)
    wrong = [(op, what, "status %d, expected %d" % (rc, status)) for op, what, status, rc in results if rc != status]
    assert not wrong, wrong
    assert launched == [], launched
    written = [(op, name) for op, c in calls.items() for name, b in c.bufs.items() if not b.untouched()]
    assert not written, "written by a refused call: %s" % written
    # the same operands are legal: each call goes through once nothing is overridden (one batch item less at the grid limit)
    for op, c in calls.items():
        assert c.launch({"B": LG.GRID_Z} if op.startswith("grid") else None) == 0, op
    torch.cuda.synchronize()
    assert all(b.intact() for c in calls.values() for b in c.bufs.values())
