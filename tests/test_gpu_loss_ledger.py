"""GPU (-m gpu): every row of the ledger of the loss, epilogue and PReLU kernels (tests/loss_ledger.py) on the device.

Per row: one raw ctypes call of the C-ABI entry point with the row's inputs at the row's misalignments; the launched
kernels recorded with torch.profiler must be the row's compute kernel(s) plus the reduction helper and no other kernel of
losses.hip / wssim.hip / epilogue.hip / prelu.hip; status 0; every output and every element of `sums` the header defines
within the row's band of the fp64 reference at EVERY element, and equal to the exact expectation where the arithmetic is
exact (integer mask sums, PReLU's grad_x, gradients under a zero weight / mask / root / coef).  Every output, every `sums`
buffer and every workspace lives inside 4096-float guard bands of a NaN bit pattern that must be bitwise unchanged
afterwards; they all start as that pattern (an unwritten element fails the comparison, a workspace element read without
having been written poisons the sums), and the workspaces have exactly the size the header documents, so a write one
float beyond lands in the guard.  Nullable outputs that are not asked for are passed as NULL.  A summary line per row
(kernels, errors over band, time) is printed.

The argument errors the header defines for these entry points are refused with their status before anything is launched
or written."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ledger as LG  # noqa: E402
from ledger_harness import Guarded, kernels_launched, load_lib, normalize, on_device, stream as _stream  # noqa: E402
import loss_ledger_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

FS_ERR_NULLPTR, FS_ERR_SHAPE, FS_ERR_ARG = 1, 2, 3
# how the kernels of the four sources are named: a launched kernel of that kind that is not a ledger symbol is an error
PREFIXES = ("robust_sum_", "census_dist_", "wssim_", "merge_", "distill", "prelu_")
KNOWN = {k for r in LG.ROWS for k in LG.kernels_of(r)} | set(LG.UNREACHABLE) | LG.HELPERS

# entry point and argument names (pointers: an input of loss_ledger_inputs.data or an output of out_sizes, NULL when the
# row has neither; the rest: scalars of the row)
SIG = {
    "rs_fwd": ("fs_robust_sum", "x y w sums ws B C S H W border mode q eps"),
    "rs_bwd": ("fs_robust_sum_bwd", "x y w coef gx gy B C S H W border mode q eps"),
    "cen_fwd": ("fs_census_dist_fwd", "img1 img2 dist B H W md"),
    "cen_bwd": ("fs_census_dist_bwd", "img1 img2 gdist g1 g2 B H W md"),
    "ws_fwd": ("fs_wssim_fwd", "x y w sums ws B C H W use_occ"),
    "ws_bwd": ("fs_wssim_bwd", "x y w coef gx gy B C H W use_occ"),
    "mg_fwd": ("fs_merge_fwd", "w0 w1 m merged sig B C S"),
    "mg_bwd": ("fs_merge_bwd", "w0 w1 m gmerged gsig gw0 gw1 gm B C S"),
    "ds_fwd": ("fs_distill_fwd", "mi0 mt gt fi0 ft sums ws B C F S"),
    "ds_bwd": ("fs_distill_bwd", "mi0 mt gt fi0 ft coef gf0 B C F S"),
    "d3_fwd": ("fs_distill3_fwd", "mi0 mi1 mi2 mt gt fi0 fi1 fi2 ft sums ws B C F S"),
    "d3_bwd": ("fs_distill3_bwd", "mi0 mi1 mi2 mt gt fi0 fi1 fi2 ft coef gf0 gf1 gf2 B C F S"),
    "prelu": ("fs_prelu_bwd", "x g a gx gw gb ws B C S nw"),
}
SCALARS = ("B", "C", "S", "H", "W", "F", "border", "mode", "q", "eps", "md", "use_occ", "nw")
# the pointers each entry point requires (FS_ERR_NULLPTR when one is NULL)
REQUIRED = {
    "rs_fwd": "x sums ws", "rs_bwd": "x coef", "cen_fwd": "img1 img2 dist", "cen_bwd": "img1 img2 gdist",
    "ws_fwd": "x y w sums ws", "ws_bwd": "x y w coef", "mg_fwd": "w0 w1 m merged", "mg_bwd": "w0 w1 m gmerged",
    "ds_fwd": "mi0 mt gt fi0 ft sums ws", "ds_bwd": "mi0 mt gt fi0 ft coef gf0",
    "d3_fwd": "mi0 mi1 mi2 mt gt fi0 fi1 fi2 ft sums ws", "d3_bwd": "mi0 mi1 mi2 mt gt fi0 fi1 fi2 ft coef gf0 gf1 gf2",
    "prelu": "x g a gx gw ws",
}


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _kernels_launched(fn):
    """(fn's return value, normalized names of the kernels of the four sources it launched); one the ledger does not know
    is an error."""
    return kernels_launched(fn, normalize, lambda n: n in KNOWN or n.startswith(PREFIXES), KNOWN)


class Call:
    """Device operands, guarded outputs and the launch of one row."""

    def __init__(self, lib, r, T):
        self.lib, self.r = lib, r
        m = r["mis"]
        self.D = {name: on_device(t, m.get(name, 0)) for name, t in T.items()}
        self.bufs = {name: Guarded(n, mis=m.get(name, 0)) for name, n in I.out_sizes(r).items()}
        assert not set(self.D) & set(self.bufs)
        self.scal = dict({k: r[k] for k in SCALARS if k in r}, md=3)

    def argv(self, over=None):
        over = over or {}
        out = []
        for name in SIG[self.r["op"]][1].split():
            if name in over:
                out.append(over[name])
            elif name in SCALARS:
                out.append(self.scal[name])
            elif name in self.bufs:
                out.append(self.bufs[name].ptr())
            else:
                out.append(self.D[name].data_ptr() if name in self.D else None)
        return out

    def launch(self, over=None):
        return getattr(self.lib, SIG[self.r["op"]][0])(*self.argv(over), _stream())

    def got(self, name, shape):
        if name.startswith("sum"):
            k = int(name[3:])
            return self.bufs["sums"].t[k:k + 1].view(shape)
        return self.bufs[name].t.view(shape)


@pytest.mark.parametrize("r", LG.ROWS, ids=[LG.row_id(r) for r in LG.ROWS])
def test_ledger_row(lib, r):
    t0 = time.perf_counter()
    T = I.data(r)
    ref = I.results(r, T, torch.float64)
    call = Call(lib, r, T)
    argv = call.argv()
    for name, a in zip(SIG[r["op"]][1].split(), argv):  # NULL exactly where the row has no such operand
        if name not in SCALARS:
            assert (a is None) == (name not in T and name not in call.bufs), name
    rc, launched = _kernels_launched(call.launch)
    assert rc == 0, "status %d" % rc
    compute = [n for n in launched if n not in LG.HELPERS]
    want = LG.kernels_of(r)
    assert set(want) <= set(compute), "expected %s, launched %s" % (want, launched)
    assert set(compute) == set(want), "other kernels of these sources ran: %s" % launched
    assert len(compute) == len(want), "launched more than once: %s" % launched
    finishes = {"rs_fwd": 1, "ws_fwd": 1, "ds_fwd": 1, "d3_fwd": 2}.get(r["op"], 0)  # one reduction finish per sums pair
    assert len(launched) - len(compute) == finishes, "expected %d x %s, launched %s" % (finishes, sorted(LG.HELPERS), launched)
    errs, inexact = {}, []
    got = {}
    for name, (rf, tol) in ref.items():
        got[name] = call.got(name, rf.shape).detach().cpu()
        g = got[name].double()
        errs[name] = float("inf") if bool((~torch.isfinite(g)).any()) else float((g - rf).abs().max()) / I.band(rf, tol)
    for name, (want_x, mask) in I.exact(r, T).items():
        g, w = got[name].reshape(-1), want_x.reshape(-1)
        if mask is not None:
            g, w = g[mask.reshape(-1)], w[mask.reshape(-1)]
        if not torch.equal(g, w):
            inexact.append("%s: %d of %d elements differ" % (name, int((g != w).sum()), g.numel()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("LEDGER %-8s %-36s err/band %s  %.2fs  %s" % (r["op"], "+".join(want), " ".join("%s=%.3f" % kv for kv in
                                                                                         sorted(errs.items())), dt, r["why"]))
    bad_guard = [name for name, b in call.bufs.items() if not b.intact()]
    assert not bad_guard, "writes outside %s" % bad_guard
    assert errs and all(e <= 1.0 for e in errs.values()), errs
    assert not inexact, inexact
    covered = {("sums" if n.startswith("sum") else n) for n in ref}
    assert covered == set(call.bufs) - {"ws"}, "outputs without a comparison: %s" % sorted(set(call.bufs) - covered)


# ---- argument errors are refused before anything is launched or written ---------------------------------------------
def _base_rows():
    return {
        "rs_fwd": LG.make("rs_fwd", "-", "refusal", B=2, C=3, H=7, W=9, border=3, wkind="01"),
        "rs_bwd": LG.make("rs_bwd", "-", "refusal", B=2, C=3, H=7, W=9, border=3, wkind="01", grads=("gx", "gy")),
        "cen_fwd": LG.make("cen_fwd", "-", "refusal", H=7, W=7),
        "cen_bwd": LG.make("cen_bwd", "-", "refusal", H=7, W=7, grads=("g1", "g2")),
        "ws_fwd": LG.make("ws_fwd", "-", "refusal", C=2, H=5, W=6),
        "ws_bwd": LG.make("ws_bwd", "-", "refusal", C=2, H=5, W=6, grads=("gx", "gy")),
        "mg_fwd": LG.make("mg_fwd", "-", "refusal", C=2, S=33, sig=True),
        "mg_bwd": LG.make("mg_bwd", "-", "refusal", C=2, S=33, grads=("gw0", "gw1", "gm"), gsig=True),
        "ds_fwd": LG.make("ds_fwd", "-", "refusal", C=2, F=4, S=33),
        "ds_bwd": LG.make("ds_bwd", "-", "refusal", C=2, F=4, S=33),
        "d3_fwd": LG.make("d3_fwd", "-", "refusal", C=2, F=4, S=33),
        "d3_bwd": LG.make("d3_bwd", "-", "refusal", C=2, F=4, S=33),
        "prelu": LG.make("prelu", "-", "refusal", B=2, C=3, S=33, nw=3, bias=True),
    }


def _refusals():
    """(op, what, {argument: value}, status) -- each argument error the header defines for these entry points."""
    out = []
    for op, names in REQUIRED.items():
        out += [(op, "%s NULL" % name, {name: None}, FS_ERR_NULLPTR) for name in names.split()]
    for op, a, b in (("rs_bwd", "gx", "gy"), ("cen_bwd", "g1", "g2"), ("ws_bwd", "gx", "gy")):
        out.append((op, "both gradients NULL", {a: None, b: None}, FS_ERR_NULLPTR))
    out.append(("mg_bwd", "all three gradients NULL", {"gw0": None, "gw1": None, "gm": None}, FS_ERR_NULLPTR))
    out.append(("rs_bwd", "grad_y without y", {"y": None}, FS_ERR_NULLPTR))
    for op in ("rs_fwd", "rs_bwd"):
        out += [(op, "border > 0 with H * W != S", {"W": 8}, FS_ERR_SHAPE),
                (op, "mode 4", {"mode": 4}, FS_ERR_ARG), (op, "mode -1", {"mode": -1}, FS_ERR_ARG),
                (op, "border < 0", {"border": -1}, FS_ERR_ARG)]
    for op in ("cen_fwd", "cen_bwd"):
        out += [(op, "max_distance 2", {"md": 2}, FS_ERR_ARG), (op, "max_distance 4", {"md": 4}, FS_ERR_ARG),
                (op, "B = 65536", {"B": 65536}, FS_ERR_SHAPE)]
    for op in ("ws_fwd", "ws_bwd"):
        out += [(op, "H = 2", {"H": 2}, FS_ERR_SHAPE), (op, "W = 2", {"W": 2}, FS_ERR_SHAPE),
                (op, "B * C = 65536", {"B": 32768}, FS_ERR_SHAPE)]
    out += [("prelu", "num_weights 2 with C = 3", {"nw": 2}, FS_ERR_ARG),
            ("prelu", "num_weights 0", {"nw": 0}, FS_ERR_ARG)]
    return out


def test_argument_errors_are_refused(lib):
    rows = _base_rows()
    calls = {op: Call(lib, r, I.data(r)) for op, r in rows.items()}
    cases = _refusals()
    assert {op for op, _, _, _ in cases} == set(SIG)

    def run():
        return [(op, what, status, calls[op].launch(over)) for op, what, over, status in cases]

    results, launched = _kernels_launched(run)
    wrong = [(op, what, "status %d, expected %d" % (rc, status)) for op, what, status, rc in results if rc != status]
    assert not wrong, wrong
    assert launched == [], launched
    written = [(op, name) for op, c in calls.items() for name, b in c.bufs.items() if not b.untouched()]
    assert not written, "written by a refused call: %s" % written
    # the same operands are legal: each call goes through once nothing is overridden
    for op, c in calls.items():
        assert c.launch() == 0, op
    torch.cuda.synchronize()
    assert all(b.intact() for c in calls.values() for b in c.bufs.values())
