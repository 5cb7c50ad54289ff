"""CPU (no GPU needed): the ledger of the loss, epilogue and PReLU kernels (tests/loss_ledger.py) against the product build.

Completeness: the kernels hipcc compiles from losses.hip / wssim.hip / epilogue.hip / prelu.hip are exactly the kernels the
ledger's rows expect plus helpers -- a new kernel or instantiation without a row fails, and so does a row whose kernel no
longer exists.  Inputs: on every row's inputs the reference is finite, the fp32 oracle agrees with the fp64 reference
within the row's band at every element, the inputs keep their promised distance from every kink, every discontinuity
decision (signs, masks, clamps, root > 0, x > 0) is the same in fp32 and fp64, and the exact expectations hold for the
oracle's own arithmetic where it is exact too -- which is what lets the GPU test hold the kernels to the same bands
without leaving an element out."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import ledger_harness as H  # noqa: E402
import loss_ledger as L  # noqa: E402
import loss_ledger_inputs as I  # noqa: E402

SOURCES = ("losses.hip", "wssim.hip", "epilogue.hip", "prelu.hip")


@pytest.fixture(scope="module")
def compiled():
    return H.compiled_kernels(SOURCES, H.normalize)


def test_every_compiled_kernel_has_a_row(compiled):
    assert not L.UNREACHABLE, "these sources have no dispatch: every kernel is reachable at a test-sized tensor"
    H.assert_complete(compiled, {k for r in L.ROWS for k in L.kernels_of(r)}, L.UNREACHABLE, L.HELPERS)


def test_rows_are_well_formed():
    ids = [L.row_id(r) for r in L.ROWS]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    grads_of = {"rs_bwd": {"gx", "gy"}, "ws_bwd": {"gx", "gy"}, "cen_bwd": {"g1", "g2"}, "mg_bwd": {"gw0", "gw1", "gm"}}
    for r in L.ROWS:
        assert r["op"] in L.OPS, r
        assert r["why"], r
        assert all(0 <= m <= 3 for m in r["mis"].values()), r
        assert r["B"] >= 1 and r["C"] >= 1 and r["S"] >= 1, r
        assert isinstance(r["kernel"], tuple) and len(r["kernel"]) == (2 if r["op"] == "prelu" else 1), r
        if r["op"] in grads_of:
            assert r["grads"] and set(r["grads"]) <= grads_of[r["op"]], r
            assert "gy" not in r["grads"] or r["op"] != "rs_bwd" or r["with_y"], r
        else:
            assert not r["grads"], r
        if r["op"] in ("rs_fwd", "rs_bwd"):
            assert r["kernel"] == ((L.RS_F if r["op"] == "rs_fwd" else L.RS_B)(r["mode"]),), r
            assert r["border"] == 0 or r["S"] == r["H"] * r["W"], r
        if r["op"] == "prelu":
            assert r["nw"] in (1, r["C"]), r
        if r["op"] in ("ds_fwd", "ds_bwd", "d3_fwd", "d3_bwd"):
            assert r["F"] >= 1 and r["S"] >= 21, r
        # every misaligned name is an operand of the call
        assert set(r["mis"]) <= set(I.data(r)) | set(I.out_sizes(r)) if r["mis"] else True, r


def test_every_threshold_has_rows_on_both_sides():
    """The rows that name each rung's threshold: a row on each side for every one of them (spot check of the ledger's own
    reasons, so a deleted side is noticed)."""
    whys = " | ".join("%s: %s" % (r["op"], r["why"]) for r in L.ROWS)
    for needle in ("robust_sum fwd: n = 262144", "robust_sum fwd: n = 262145, second trip",
                   "n = 262145 = 1 x 5 x 52429", "robust_sum bwd: n = 4194304", "robust_sum bwd: n = 4194305, second trip, gx and gy",
                   "n = 4194305, second trip, gx", "n = 4194305, second trip, gy",
                   "abs_robust, y NULL, w NULL", "abs_robust, y given, w 01", "charbonnier, y NULL, w 01",
                   "charbonnier, y given, w NULL", "l1_eps, y NULL, w float", "l1_eps, y given, w 01", "l1, y NULL, w float",
                   "l1, y given, w 01", "l1, y given, w NULL", "q = 0.4 and eps = 1e-08", "q = 1 and eps = 1e-06",
                   "border = 3 on 7x9", "border = 3 on 6x9", "all weights zero", "border = 3 on 20x31", "border = 0 on 7x9",
                   "robust_sum fwd l1_eps: every operand misaligned", "robust_sum bwd charbonnier: every operand misaligned",
                   "census fwd 1x1", "census fwd 3x5", "census fwd 7x7", "census fwd 15x16", "census fwd 16x17",
                   "census fwd 17x33", "census bwd 1x1", "census bwd 15x16", "census bwd 16x17", "census bwd 17x33",
                   "B = 1, g1", "B = 3, g2", "g1 and g2", "census fwd: every operand misaligned",
                   "census bwd: every operand misaligned",
                   "wssim fwd 3x3", "wssim fwd 3x20", "wssim fwd 16x16", "wssim fwd 17x18", "wssim fwd 18x19", "wssim fwd 19x37",
                   "wssim bwd 3x3", "wssim bwd 16x16", "wssim bwd 17x18", "wssim bwd 18x19", "wssim bwd 19x37",
                   "B x C = 1x1, use_occ = 0", "B x C = 1x1, use_occ = 1", "B x C = 2x3, use_occ = 0", "B x C = 2x3, use_occ = 1",
                   "y noise, gx", "y near, gy", "gx and gy", "262144 windows", "262145 windows", "261942 windows",
                   "266412 windows", "wssim fwd: every operand misaligned", "wssim bwd: every operand misaligned",
                   "merge fwd: C = 1, sigmoid_out NULL", "merge fwd: C = 3, sigmoid_out given",
                   "merge bwd: gw0 asked for, grad_sigmoid NULL", "merge bwd: gw1 asked for", "merge bwd: gm asked for",
                   "merge bwd: gw0 gw1 asked for", "merge bwd: gw0 gm asked for", "merge bwd: gw1 gm asked for",
                   "merge bwd: gw0 gw1 gm asked for, grad_sigmoid given", "merge fwd: n = 4194304",
                   "merge fwd: n = 4194305, second trip", "merge bwd: B * S = 4194304", "merge bwd: B * S = 4194305",
                   "logits 0, +-20, +-88, +-100",
                   "distill fwd: F = 1", "distill fwd: F = 8", "distill bwd: F = 6 <= MAXF", "distill bwd: F = 7 > MAXF",
                   "distill3 bwd: F = 6 <= MAXF", "distill3 bwd: F = 7 > MAXF", "distill3 bwd: F = 8 > MAXF",
                   "distill bwd: F = 1 <= MAXF", "root == 0 block", "three students",
                   "distill bwd: coef == 0 with non-finite student flows, F = 4",
                   "distill bwd: coef == 0 with non-finite student flows, F = 7",
                   "distill3 bwd: coef == 0 with non-finite student flows, F = 4",
                   "distill3 bwd: coef == 0 with non-finite student flows, F = 7",
                   "distill_fwd_kernel: B * S = 262144", "distill_fwd_kernel: B * S = 262145",
                   "distill3_fwd_kernel: B * S = 262144", "distill3_fwd_kernel: B * S = 262145",
                   "distill_bwd_kernel: B * S = 4194304", "distill_bwd_kernel: B * S = 4194305",
                   "distill3_bwd_kernel: B * S = 4194304", "distill3_bwd_kernel: B * S = 4194305",
                   "S = 8192: 1 chunk", "S = 8193: 2 chunks", "S = 40961: 6 chunks", "S = 524288: 64 chunks",
                   "S = 524292: beyond the cap", "all four residues mod 4", "grad_bias NULL at 2 chunks",
                   "prelu: x misaligned", "prelu: g misaligned", "prelu: gx misaligned", "vector path in every block",
                   "weight, ws, grad_weight and grad_bias misaligned, not inspected",
                   "num_weights = C = 5, grad_bias given", "num_weights = C = 5, grad_bias NULL",
                   "num_weights = 1 with C = 5 (shared slope, one sum over every row), grad_bias given",
                   "num_weights = 1 with C = 5, grad_bias NULL", "num_weights = 1 with C = 1, grad_bias given",
                   "num_weights = 1 with C = 1, grad_bias NULL"):
        assert needle in whys, needle
    # the caps the needles speak of are the header's
    with open(os.path.join(ROOT, "include", "flowsci_hip.h")) as f:
        header = f.read()
    assert "#define FS_REDUCE_BLOCKS %d" % L.FS_REDUCE_BLOCKS in header
    assert "#define FS_PRELU_MAX_CHUNKS %d" % L.FS_PRELU_MAX_CHUNKS in header
    for mode, name in enumerate(("FS_PEN_ABS_ROBUST", "FS_PEN_CHARBONNIER", "FS_PEN_L1_EPS", "FS_PEN_L1")):
        assert "%s = %d" % (name, mode) in header


def test_census_restatement_is_the_oracle():
    """The dtype-generic census distance of the inputs module against oracle.losses.census_dist, both in float32."""
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(2, 3, 9, 11, generator=g), torch.rand(2, 3, 9, 11, generator=g)
    from oracle import losses as olosses
    assert float((I.census_dist(a, b) - olosses.census_dist(a, b)).abs().max()) < 2e-5


_ONE_BEYOND = [r for r in L.ROWS if I.second_trip(r) == 1 and r["B"] == 1 and r["C"] == 1]


@pytest.mark.parametrize("r", _ONE_BEYOND, ids=[L.row_id(r) for r in _ONE_BEYOND])
def test_a_dropped_second_trip_leaves_the_band(r):
    """The rows one item beyond a forward reduction's first trip: the reference without that item (the same inputs cut by
    their last element, window or voxel) is outside the band of every sum (differs at all, for a sum that is compared exactly), so a kernel whose grid-stride loop never took its
    second trip cannot pass."""
    T = I.data(r)
    full = I.results(r, T, torch.float64)
    cut = dict(r, W=r["W"] - 1, S=3 * (r["W"] - 1)) if r["op"] == "ws_fwd" else dict(r, S=r["S"] - 1)
    assert I.second_trip(cut) == 0
    short = I.results(cut, {k: t[..., :-1].contiguous() for k, t in T.items()}, torch.float64)
    assert len(full) >= 2
    exact = I.exact(r, T)
    for name, (rf, tol) in full.items():  # (an exact expectation notices any difference)
        assert float((rf - short[name][0]).abs()) > (0.0 if name in exact else 4 * I.band(rf, tol)), name


@pytest.mark.parametrize("r", L.ROWS, ids=[L.row_id(r) for r in L.ROWS])
def test_inputs_keep_the_fp32_oracle_inside_the_band(r):
    T = I.data(r)
    assert all(t.dtype == torch.float32 for t in T.values())
    for what, dist, promised in I.margins(r, T):
        assert dist >= promised, "%s: %g < %g" % (what, dist, promised)
    d64, d32 = I.decisions(r, T, torch.float64), I.decisions(r, T, torch.float32)
    for what in d64:
        assert torch.equal(d64[what], d32[what]), "fp32 and fp64 decide '%s' differently" % what
    ref = I.results(r, T, torch.float64)
    orc = I.results(r, T, torch.float32)
    sizes = I.out_sizes(r)
    worst = {}
    for name, (rf, tol) in ref.items():
        assert torch.isfinite(rf).all(), name
        assert rf.numel() == (1 if name.startswith("sum") else sizes[name]), name
        worst[name] = float((orc[name][0].double() - rf).abs().max()) / I.band(rf, tol)
    assert {("sums" if n.startswith("sum") else n) for n in ref} == set(sizes) - {"ws"}, (sorted(ref), sorted(sizes))
    for name, (want, mask) in I.exact(r, T).items():  # an exact expectation is inside the band of the reference too
        rf, tol = ref[name]
        d = (want.double().view(rf.shape) - rf).abs()
        sel = d.reshape(-1) if mask is None else d[mask.view(rf.shape)]
        assert sel.numel() == 0 or float(sel.max()) <= I.band(rf, tol), name
    print("ORACLE %-90s %s" % (L.row_id(r), " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))
    assert ref and all(v <= 1.0 for v in worst.values()), worst
