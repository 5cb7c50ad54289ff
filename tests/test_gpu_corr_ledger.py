"""GPU (-m gpu): every row of the ledger of the correlation and plane-moment kernels (tests/corr_ledger.py) on the device.

Per row: one raw ctypes call of the C-ABI entry point (the chain rows: four) with the row's inputs placed at the row's
misalignments; the kernels torch.profiler saw must be the row's kernel and no other kernel of corr2d.hip / corr3d.hip;
status 0; every output the call was given within the row's band of the float64 reference at EVERY element and bitwise
equal to the exact expectation where the band is 0 (displacement planes outside the volume, constant planes, windows
that are all padding); in the poison rows the output's non-finite set must be the reference's.  Every output of the
entry point lives inside 4096-float guard bands of a NaN bit pattern that must be bitwise unchanged afterwards and
starts as that pattern itself (an element the kernel never writes fails the comparison); a nullable output the row does
not ask for is passed as NULL and its buffer must stay untouched.  Backward rows are called a second time: the header
promises bitwise reproducible gradients.  One LEDGER line per row: entry point, kernel, error over band, time.

The argument errors the header defines for these entry points are refused with their status before anything is launched
or written; every buffer of a refused call is sized as if the call went through (for max_displacement = 5 too), so a
missed refusal still writes in bounds.  The 2^29-float and 2^31-workgroup size limits are NOT probed on the device: a
missed refusal there would launch over memory that does not exist."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corr_ledger as LG  # noqa: E402
from ledger_harness import Guarded, kernels_launched, load_lib, normalize, on_device, stream as _stream  # noqa: E402
import corr_ledger_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

FS_ERR_NULLPTR, FS_ERR_SHAPE, FS_ERR_ARG = 1, 2, 3
PREFIXES = ("corr", "plane_")  # how the kernels of the two sources are named
KNOWN = {k for r in LG.ROWS for k in LG.kernels_of(r)} | set(LG.UNREACHABLE) | LG.HELPERS

# entry point and argument names (pointers: an output of corr_ledger_inputs.out_sizes -- NULL unless the row asks for it --
# or an input of corr_ledger_inputs.data; the rest: scalars of the row)
SIG = {
    "c2_fwd": (("fs_corr2d_fwd", "f1 f2 out B C H W md"),),
    "c2_bwd": (("fs_corr2d_bwd", "f1 f2 gout g1 g2 B C H W md"),),
    "n_fwd": (("fs_corr2d_norm_fwd", "f1 f2 st1 st2 out B C H W md"),),
    "n_bwd": (("fs_corr2d_norm_bwd", "f1 f2 st1 st2 gout g1 g2 B C H W md"),),
    "p_fwd": (("fs_corr2d_pair_fwd", "f1a f2a f1b f2b stats outa outb B C H W md"),),
    "p_bwd": (("fs_corr2d_pair_bwd", "f1a f2a f1b f2b stats gouta goutb g1a g2a g1b g2b B C H W md"),),
    "mom": (("fs_plane_moments", "f stats planes S"),),
    "mom4": (("fs_plane_moments4", "fa fb fc fd stats planes S"),),
    "nb": (("fs_plane_norm_bwd", "f stats gn gf planes S"),),
    "nb4": (("fs_plane_norm_bwd4", "fa fb fc fd stats gna gnb gnc gnd gfa gfb gfc gfd planes S"),),
    "c3_fwd": (("fs_corr3d_fwd", "f1 f2 out B C D H W md"),),
    "c3_bwd": (("fs_corr3d_bwd", "f1 f2 gout g1 g2 B C D H W md"),),
    "chain": (("fs_plane_moments4", "f1a f2a f1b f2b stats BC HW"),
              ("fs_corr2d_pair_fwd", "f1a f2a f1b f2b stats outa outb B C H W md"),
              ("fs_corr2d_pair_bwd", "f1a f2a f1b f2b stats gouta goutb g1a g2a g1b g2b B C H W md"),
              ("fs_plane_norm_bwd4", "f1a f2a f1b f2b stats g1a g2a g1b g2b gfa gfb gfc gfd BC HW")),
}
SCALARS = ("B", "C", "D", "H", "W", "md", "planes", "S", "BC", "HW")
BACKWARD = ("c2_bwd", "n_bwd", "p_bwd", "c3_bwd", "nb", "nb4")
STATS_VIEW = {"mean": 0, "rstd": 1}  # results compared against a column of the `stats` output


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
        self.bufs = {name: Guarded(n, mis=m.get(name, 0)) for name, n in I.out_sizes(r).items()}
        self.asked = set(I.requested(r))
        self.scal = dict({k: r[k] for k in SCALARS if k in r}, BC=r["B"] * r["C"], HW=r["H"] * r["W"])

    def _ptr(self, name):
        r = self.r
        if name in self.bufs:
            return self.bufs[name].ptr() if name in self.asked else None
        if r["op"] == "nb4" and r["drop"] and "gf" + name[-1] not in self.asked and name != "stats":
            return None  # f / grad_n of a skipped tensor
        name = I.ALIAS.get(name, name) if r["alias"] else name
        return self.D[name].data_ptr() if name in self.D else None

    def argv(self, names, over=None):
        over = over or {}
        return [over[n] if n in over else (self.scal[n] if n in SCALARS else self._ptr(n)) for n in names.split()]

    def launch(self, over=None):
        for fn, names in SIG[self.r["op"]]:
            rc = getattr(self.lib, fn)(*self.argv(names, over), _stream())
            if rc != 0:
                return rc
        return 0

    def got(self, name, shape):
        if name in STATS_VIEW:
            return self.bufs["stats"].t.view(-1, 2)[:, STATS_VIEW[name]].reshape(shape)
        return self.bufs[name].t.view(shape)

    def bits(self):
        return {name: b.buf.view(torch.int32).clone() for name, b in self.bufs.items()}


@pytest.mark.parametrize("r", LG.ROWS, ids=[LG.row_id(r) for r in LG.ROWS])
def test_ledger_row(lib, r):
    t0 = time.perf_counter()
    T = I.data(r)
    ref = I.results(r, T)
    call = Call(lib, r, T)
    rc, launched = _kernels_launched(call.launch)
    assert rc == 0, "status %d" % rc
    want = LG.kernels_of(r)
    assert launched == list(want), "expected %s of %s, launched %s" % (want, r["src"], launched)
    errs, inexact, sets = {}, [], []
    for name, (rf, band) in ref.items():
        if name not in call.asked and name not in STATS_VIEW:
            continue
        g = call.got(name, rf.shape).detach().cpu()
        errs[name], miss, same_set = I.compare(g, rf, band, poison=bool(r["poison"]))
        if miss:
            inexact.append("%s: %d elements miss their exact expectation" % (name, miss))
        if not same_set:
            sets.append("%s: %d non-finite elements, the reference has %d" % (
                name, int((~torch.isfinite(g)).sum()), int((~torch.isfinite(rf)).sum())))
    if r["op"] == "mom4" and r["alias"]:
        st = call.bufs["stats"].t.view(4, -1).view(torch.int32)
        assert bool((st == st[0:1]).all()), "one tensor given four times, four different tables"
    twice = []
    if r["op"] in BACKWARD:
        first = call.bits()
        assert call.launch() == 0
        torch.cuda.synchronize()
        twice = [name for name, b in call.bits().items() if not torch.equal(b, first[name])]
    dt = time.perf_counter() - t0
    print("LEDGER %-9s %-36s err/band %s  %.2fs  %s" % (r["op"], "+".join(want), " ".join(
        "%s=%.3f" % kv for kv in sorted(errs.items())), dt, r["why"]))
    bad_guard = [name for name, b in call.bufs.items() if not b.intact()]
    assert not bad_guard, "writes outside %s" % bad_guard
    touched = [name for name, b in call.bufs.items() if name not in call.asked and not b.untouched()]
    assert not touched, "outputs that were not asked for were written: %s" % touched
    assert not sets, sets
    assert errs and all(e <= 1.0 for e in errs.values()), errs
    assert not inexact, inexact
    assert not twice, "a second call gave other bits in %s" % twice
    covered = {("stats" if n in STATS_VIEW else n) for n in errs}
    internal = {"g1a", "g2a", "g1b", "g2b"} if r["op"] == "chain" else set()
    assert covered == call.asked - internal, "outputs without a comparison: %s" % sorted(call.asked - internal - covered)


# ---- argument errors are refused before anything is launched or written ---------------------------------------------
_CORR = ("c2_fwd", "c2_bwd", "n_fwd", "n_bwd", "p_fwd", "p_bwd", "c3_fwd", "c3_bwd")
REQUIRED = {
    "c2_fwd": "f1 f2 out", "c2_bwd": "f1 f2 gout", "n_fwd": "f1 f2 st1 st2 out", "n_bwd": "f1 f2 st1 st2 gout",
    "p_fwd": "f1a f2a f1b f2b outa outb", "p_bwd": "f1a f2a f1b f2b gouta goutb", "mom": "f stats",
    "mom4": "fa fb fc fd stats", "nb": "f stats gn gf", "nb4": "stats", "c3_fwd": "f1 f2 out", "c3_bwd": "f1 f2 gout",
}


def _base_row(op, md=4):
    if op in I.MOMENT_OPS:
        return LG.make(op, "-", "refusal", planes=3, S=24)
    return LG.make(op, "-", "refusal", B=2, C=3, D=3 if op.startswith("c3_") else 1, H=4, W=9, md=md, stats=op.startswith("p_"))


def _refusals():
    """(op, md of the call's buffers, what, {argument: value}, status) -- each argument error the header defines."""
    out = []
    for op, names in REQUIRED.items():
        out += [(op, 4, "%s NULL" % name, {name: None}, FS_ERR_NULLPTR) for name in names.split()]
    for op in ("c2_bwd", "n_bwd", "c3_bwd"):
        out.append((op, 4, "both gradients NULL", {"g1": None, "g2": None}, FS_ERR_NULLPTR))
    out.append(("p_bwd", 4, "all four gradients NULL", dict.fromkeys(LG.GRADS_OF["p_bwd"]), FS_ERR_NULLPTR))
    for k in "abcd":
        out.append(("nb4", 4, "grad_f%s given with f%s NULL" % (k, k), {"f" + k: None}, FS_ERR_NULLPTR))
        out.append(("nb4", 4, "grad_f%s given with grad_n%s NULL" % (k, k), {"gn" + k: None}, FS_ERR_NULLPTR))
    for op in _CORR:
        out += [(op, 4, "max_displacement 0", {"md": 0}, FS_ERR_ARG), (op, 5, "max_displacement 5", {}, FS_ERR_ARG),
                (op, 4, "B = 0", {"B": 0}, FS_ERR_SHAPE)]
    for op in I.MOMENT_OPS:
        out += [(op, 4, "planes = 0", {"planes": 0}, FS_ERR_SHAPE), (op, 4, "S = 1", {"S": 1}, FS_ERR_SHAPE)]
    return out


def test_argument_errors_are_refused(lib):
    cases = _refusals()
    assert {c[0] for c in cases} == set(SIG) - {"chain"}
    calls = {}
    for op, md, _, _, _ in cases:
        if (op, md) not in calls:
            r = _base_row(op, md)
            calls[(op, md)] = Call(lib, r, I.data(r))

    def run():
        return [(op, what, status, calls[(op, md)].launch(over)) for op, md, what, over, status in cases]

    results, launched = _kernels_launched(run)
    wrong = [(op, what, "status %d, expected %d" % (rc, status)) for op, what, status, rc in results if rc != status]
    assert not wrong, wrong
    assert launched == [], launched
    written = [(key, name) for key, c in calls.items() for name, b in c.bufs.items() if not b.untouched()]
    assert not written, "written by a refused call: %s" % written
    # the same operands are legal: each call goes through once nothing is overridden
    for (op, md), c in calls.items():
        if md == 4:
            assert c.launch() == 0, op
    torch.cuda.synchronize()
    assert all(b.intact() for c in calls.values() for b in c.bufs.values())
    assert all(b.untouched() for (op, md), c in calls.items() if md == 5 for b in c.bufs.values())
