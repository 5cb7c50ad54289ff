"""CPU (no GPU needed): the ledger of the unsupervised 3-D loss kernels (tests/unsup3d_ledger.py) against the product build.

Completeness: the kernels hipcc compiles from census3d.hip / flowsmooth3d.hip are exactly the kernels the ledger's rows
expect plus helpers -- a new instantiation without a row fails, and so does a row whose kernel no longer exists.  Inputs:
on every row's inputs the reference is finite, the fp32 oracle agrees with the fp64 reference within a QUARTER of the
row's local band at every element (exactly where the scale is 0), every discontinuity decision (which pairs exist, weights
of exactly 0 and 1) is the same in fp32 and fp64, and the exact expectations hold for the reference.  Mutants: six ways a
kernel could be subtly wrong, applied to the reference, each leave the band on the rows that exist for them -- which is
what lets the GPU test hold the kernels to the same bands without leaving an element out."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import census3d_ref as ref  # noqa: E402
import ledger_harness as H  # noqa: E402
import unsup3d_ledger as L  # noqa: E402
import unsup3d_ledger_inputs as I  # noqa: E402

SOURCES = ("census3d.hip", "flowsmooth3d.hip")
IDS = [L.row_id(r) for r in L.ROWS]


def _rows(pred):
    rows = [r for r in L.ROWS if pred(r)]
    return pytest.mark.parametrize("r", rows, ids=[L.row_id(r) for r in rows])


@pytest.fixture(scope="module")
def compiled():
    return H.compiled_kernels(SOURCES, H.normalize)


def test_every_compiled_kernel_has_a_row(compiled):
    assert not L.UNREACHABLE, "these sources dispatch on the radius alone: every kernel is reachable at a test-sized tensor"
    H.assert_complete(compiled, {k for r in L.ROWS for k in L.kernels_of(r)}, L.UNREACHABLE, L.HELPERS)


def test_rows_are_well_formed():
    assert len(IDS) == len(set(IDS)), sorted(i for i in IDS if IDS.count(i) > 1)
    operands = {"cen_fwd": {"vol1", "vol2", "dist"}, "cen_bwd": {"vol1", "vol2", "gdist", "g1", "g2"},
                "fs_fwd": {"flow", "guide", "sums", "ws"}, "fs_bwd": {"flow", "guide", "coef", "gflow"}}
    for r in L.ROWS:
        assert r["op"] in L.OPS and r["why"], r
        assert all(1 <= m <= 3 for m in r["mis"].values()), r
        assert min(r[k] for k in "BCDHW") >= 1, r
        assert r["kernel"] == (L.kernel_of(r["op"], r["R"]),), r
        if r["op"] in ("cen_fwd", "cen_bwd"):
            assert r["R"] in (1, 2, 3) and r["C"] == 1 and "<%d>" % r["R"] in r["kernel"][0], r
            assert r["kind"] in ("noise", "near", "apart", "equal", "const", "kzero"), r
            assert (r["kind"] == "apart") == (r["D"] * r["H"] * r["W"] <= 24), r
            assert (r["kind"] != "kzero" or r["op"] == "cen_bwd" and r["W"] > I.KZERO_X + r["R"]), r
            assert (r["kind"] != "const" or r["op"] == "cen_fwd" and min(r["D"], r["H"], r["W"]) > 2 * r["R"]), r
        else:
            assert r["R"] == 0 and r["kind"] in ("mix", "heavy", "plain") and r["kappa"] >= 0, r
            assert r["op"] == "fs_bwd" or r["coef"] == L.DEFAULTS["coef"], r
        assert bool(r["grads"]) == (r["op"] == "cen_bwd") and set(r["grads"]) <= {"g1", "g2"}, r
        # every misaligned name is an operand of the call, and of this row's call
        assert set(r["mis"]) <= operands[r["op"]], r
        if r["mis"]:
            assert set(r["mis"]) <= set(I.data(r)) | set(I.out_sizes(r)), r
        twin = L.twin_of(r)
        if twin is not None:  # a twin sees the same values (all but a guide that must not be read)
            T, U = I.data(r), I.data(twin)
            assert all(torch.equal(T[k], U[k]) for k in U), r
            assert set(T) - set(U) <= {"guide"}, r


def test_every_threshold_has_rows_on_both_sides():
    """The rows that name each rung's threshold: a row on each side for every one of them (spot check of the ledger's own
    reasons, so a deleted side is noticed)."""
    whys = " | ".join("%s: %s" % (r["op"], r["why"]) for r in L.ROWS)
    needles = []
    for d in ("fwd", "bwd"):
        for R in (1, 3):
            needles += ["census %s R = %d, %s" % (d, R, s) for s in (
                "1x1x1", "2x3x4", "%dx%dx%d: one patch" % ((2 * R + 1,) * 3), "7x16x32", "8x16x32", "9x16x32", "8x15x32",
                "8x17x32", "8x16x31", "8x16x33", "9x17x33", "17x33x65")]
            needles += ["census %s R = %d: every operand misaligned" % (d, R),
                        "census %s R = %d: vol2 bitwise equal to vol1" % (d, R)]
        needles += ["census %s R = 2, 8x16x32" % d, "census %s R = 2, 9x17x33" % d]
        needles += ["census %s R = %d, B = 3 with 17x17x33" % (d, R) for R in (1, 2, 3)]
        needles += ["census %s: B = 65535" % d]
        needles += ["smooth %s %s" % (d, s) for s in ("1x7x9", "5x1x9", "5x7x1", "1x1x1", "2x2x2", "3x4x5", "6x10x12")]
        needles += ["smooth %s: every operand misaligned" % d]
    needles += ["census bwd R = %d: a block of zeros in grad_dist" % R for R in (1, 3)]
    needles += ["census fwd R = %d: two constant volumes" % R for R in (1, 2, 3)]
    needles += ["vol2 noise, g1 and g2", "vol2 near, g1 and g2", "vol2 noise, g1 |", "vol2 near, g2 |"]
    needles += ["6x10x12 with the special blocks, B x C = 2x6 (flow offset b * C * DHW, guide offset b * DHW), %s, %s" % (g[2], q[2])
                for g in L.GUIDES for q in L.QEPS]
    needles += ["coef 0.5", "coef -3", "coef 0 |", "B x C = 1x1", "B x C = 2x6", "B x C = 1x6", "B x C = 2x1",
                "262144 voxels (1x2x131072), C = 1", "262146 voxels (1x2x131073), C = 1: second trip",
                "262144 voxels (1x2x131072), C = 2", "262146 voxels (1x2x131073), C = 2: second trip",
                "4194304 voxels (1x1x4194304)", "4194305 voxels (1x1x4194305), second trip",
                "4194306 voxels (1x2x2097153), second trip with H > 1",
                "16777216 pairs: sums[1] == 2^24 exactly", "16777217 pairs", "16777219 pairs"]
    whys += " |"
    for needle in needles:
        assert needle in whys, needle
    # every gradient choice per radius
    for R in (1, 2, 3):
        assert {r["grads"] for r in L.ROWS if r["op"] == "cen_bwd" and r["R"] == R} == {("g1",), ("g2",), ("g1", "g2")}, R
    # the numbers the needles speak of are the sources'
    with open(os.path.join(ROOT, "include", "flowsci_hip.h")) as f:
        assert "#define FS_REDUCE_BLOCKS %d" % L.FS_REDUCE_BLOCKS in f.read()
    with open(os.path.join(H.CSRC, "census3d.hip")) as f:
        census = f.read()
    assert "constexpr int BX = %d, BY = %d, BZ = %d," % (L.BX, L.BY, L.BZ) in census
    assert "(long long)B * nbz > %d" % L.GRID_Z in census
    with open(os.path.join(H.CSRC, "flowsmooth3d.hip")) as f:
        smooth = f.read()
    assert "want < FS_REDUCE_BLOCKS ? want : FS_REDUCE_BLOCKS" in smooth
    assert "want < %d ? want : %d" % (L.BWD_BLOCKS, L.BWD_BLOCKS) in smooth
    assert len(re.findall(r"dim3\(256\)", smooth)) == 3  # 256 voxels per workgroup, and the finish


def test_census_terms_are_the_gradient():
    """The scale's restatement of the header's pair formula: its signed sum is autograd of census3d_ref within 1e-12 of the
    scale, at every element; borders, several radii, a batch."""
    g = torch.Generator().manual_seed(7)
    for R, shape in ((1, (2, 1, 3, 4, 5)), (2, (1, 1, 5, 6, 7)), (3, (2, 1, 4, 9, 8))):
        v1 = torch.rand(*shape, generator=g, dtype=torch.float64)
        v2 = (v1 + 0.1 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(0, 1)
        k = torch.randn(*shape, generator=g, dtype=torch.float64)
        a, b = v1.clone().requires_grad_(), v2.clone().requires_grad_()
        w1, w2 = torch.autograd.grad((ref.census3d_dist(a, b, R) * k).sum(), [a, b])
        g1, g2, s1, s2 = I.census_terms(v1, v2, k, R)
        assert bool((s1 > 0).all()) and bool((s2 > 0).all())
        assert float(((g1 - w1).abs() / s1).max()) <= 1e-12 and float(((g2 - w2).abs() / s2).max()) <= 1e-12


def test_smooth_terms_are_the_gradient():
    g = torch.Generator().manual_seed(8)
    flow = torch.randn(2, 3, 4, 5, 6, generator=g, dtype=torch.float64)
    guide = torch.rand(2, 1, 4, 5, 6, generator=g, dtype=torch.float64)
    for gd, kappa in ((None, 0.0), (guide, 12.5)):
        a = flow.clone().requires_grad_()
        (want,) = torch.autograd.grad(ref.flow_smooth3d_sums(a, gd, 0.25, 1e-3, kappa)[0], [a])
        got, s = I.smooth_terms(flow, gd, 0.25, 1e-3, kappa, -3.0)
        assert float(((got + 3.0 * want).abs() / s).max()) <= 1e-12


def test_closed_forms_of_the_padding_rows():
    """Zero padding in closed form: two constant volumes a != b give n_out(p) * D(T(-a) - T(-b)), n_out the number of taps
    outside the volume (0 inside: exactly 0); a single voxel gives ((2R+1)^3 - 1) * D(T(-v1) - T(-v2))."""
    T_ = lambda u: u / torch.sqrt(0.81 + u * u)
    D_ = lambda e: e * e / (0.1 + e * e)
    seen = 0
    for r in L.ROWS:
        if r["op"] != "cen_fwd" or not (r["kind"] == "const" or r["D"] * r["H"] * r["W"] == 1):
            continue
        T = I.data(r)
        v1, v2 = T["vol1"].double(), T["vol2"].double()
        rf, _, tol = I.results(r, T)["dist"]
        ones = torch.ones(1, 1, r["D"], r["H"], r["W"], dtype=torch.float64)
        P = 2 * r["R"] + 1
        n_in = torch.nn.functional.conv3d(ones, torch.ones(1, 1, P, P, P, dtype=torch.float64), padding=r["R"])
        want = (P ** 3 - n_in) * D_(T_(-v1) - T_(-v2))
        assert float((rf - want).abs().max()) <= 1e-12 * float(want.max()), L.row_id(r)
        seen += 1
    assert seen == 6


@_rows(lambda r: True)
def test_inputs_keep_the_fp32_oracle_inside_a_quarter_of_the_band(r):
    T = I.data(r)
    assert all(t.dtype == torch.float32 for t in T.values())
    d64, d32 = I.decisions(r, T, torch.float64), I.decisions(r, T, torch.float32)
    for what in d64:
        assert torch.equal(d64[what], d32[what]), "fp32 and fp64 decide '%s' differently" % what
        if r["kappa"] >= 1e4 and what.endswith("== 1"):  # every weight is exactly 0 or 1, and both occur
            zero = d64[what.replace("== 1", "== 0")]
            assert bool(((d64[what] + zero) == 1).all()), what
    ref64 = I.results(r, T, torch.float64)
    orc = I.results(r, T, torch.float32)
    sizes = I.out_sizes(r)
    worst = {}
    for name, (rf, scale, tol) in ref64.items():
        assert torch.isfinite(rf).all(), name
        assert rf.numel() == (1 if name.startswith("sum") else sizes[name]), name
        worst[name], not_zero = I.compare(orc[name][0], rf, scale, tol)
        assert not_zero == 0, "%s: %d elements of scale 0 are not exactly 0 in the oracle" % (name, not_zero)
    assert {("sums" if n.startswith("sum") else n) for n in ref64} == set(sizes) - {"ws"}, (sorted(ref64), sorted(sizes))
    if r["op"] == "fs_fwd":
        assert float(ref64["sum1"][0]) == I.pairs(r)
    for name, (want, mask) in I.exact(r, T).items():  # the exact expectations hold for the reference
        rf = ref64[name][0]
        sel = slice(None) if mask is None else mask.reshape(-1)
        assert torch.equal(rf.float().reshape(-1)[sel], want.reshape(-1)[sel]), name
        assert mask is None or bool(mask.any()), name
    print("ORACLE %-70s %s" % (L.row_id(r), " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))
    assert ref64 and all(v <= 0.25 for v in worst.values()), worst


# ---- mutants --------------------------------------------------------------------------------------------------------------
def _out_of_band(mut, rf, scale, tol):
    """bool tensor: the elements of a mutant's output outside the reference's band (any difference where the scale is 0)."""
    return (mut - rf).abs() > tol * scale


def _volume_border(r):
    """[D,H,W] bool: voxels with a tap outside the volume."""
    inside = torch.zeros(r["D"], r["H"], r["W"], dtype=torch.bool)
    R = r["R"]
    inside[R:r["D"] - R, R:r["H"] - R, R:r["W"] - R] = True
    return ~inside


@_rows(lambda r: r["op"] in ("cen_fwd", "cen_bwd") and r["kind"] != "equal")
def test_mutant_replicate_padding_leaves_the_band(r):
    """Mutant 1: replicate padding.  Out of band at border voxels on every row (each has a border), the constant volumes
    included; voxels whose neighbourhood (and, for a gradient, whose neighbours' neighbourhoods) is inside are unchanged."""
    T = I.data(r)
    rf = I.results(r, T)
    border = _volume_border(r)
    deep = ~_volume_border(dict(r, R=2 * r["R"]))
    for name, m in I.census_mutant(r, T, "replicate").items():
        bad = _out_of_band(m, *rf[name])
        assert bool(bad[:, :, border].any()), name
        assert not bool(bad[:, :, ~border if name == "dist" else deep].any()), name


@_rows(lambda r: r["op"] in ("cen_fwd", "cen_bwd") and L.bricks(r) > 1 and r["kind"] not in ("equal", "const"))
def test_mutant_missing_halo_leaves_the_band(r):
    """Mutant 2: every brick evaluated with zeros around it.  Out of band on every row with more than one brick, and only
    within R of a face between bricks."""
    T = I.data(r)
    rf = I.results(r, T)
    face = I.near_brick_face(r)
    for name, m in I.census_mutant(r, T, "bricked").items():
        bad = _out_of_band(m, *rf[name])
        assert bool(bad[:, :, face].any()), name
        assert not bool(bad[:, :, ~face].any()), name


@_rows(lambda r: r["op"] == "cen_bwd" and r["kind"] != "equal" and r["D"] * r["H"] * r["W"] > 1)
def test_mutant_centre_weight_only_leaves_the_band(r):
    """Mutant 3: k[q] in place of k[q] + k[q+delta] (a voxel's role as the neighbour of other centres forgotten)."""
    T = I.data(r)
    rf = I.results(r, T)
    for name, m in I.census_mutant(r, T, "centre_weight").items():
        assert bool(_out_of_band(m, *rf[name]).any()), name


@_rows(lambda r: r["op"] == "fs_bwd" and r["guide"] and r["kappa"] > 0 and r["coef"] != 0 and I.pairs(r) > 0)
def test_mutant_own_weight_leaves_the_band(r):
    """Mutant 4: w_a(p) in place of w_a(p - e_a) on the three backward-neighbour terms."""
    T = I.data(r)
    rf, scale, tol = I.results(r, T)["gflow"]
    m = I.smooth_terms(T["flow"].double(), T["guide"].double(), I.f32(r["q"]), I.f32(r["eps"]), I.f32(r["kappa"]),
                       r["coef"], own_weight=True)[0]
    assert bool(_out_of_band(m, rf, scale, tol).any())


@_rows(lambda r: r["op"] == "fs_fwd" and r["B"] * r["D"] * r["H"] * r["W"] > L.FWD_CAP)
def test_mutant_dropped_second_trip_leaves_the_band(r):
    """Mutant 5: the forward without its second trip: sums[0] moves by more than four bands and sums[1] differs -- also
    on the rows where the second trip owns a single voxel with a pair."""
    T = I.data(r)
    R_ = I.results(r, T)
    s1, n = I.smooth_sums_mutant(r, T, "first_trip")
    (rf, scale, tol), cnt = R_["sum0"], int(R_["sum1"][0])
    assert 0 < cnt - n, (cnt, n)
    assert float((s1 - rf).abs()) > 4 * tol * float(scale)


@_rows(lambda r: r["op"] == "fs_fwd" and r["D"] * r["H"] > 1 and r["H"] * r["W"] > 1)
def test_mutant_flattened_neighbours_leave_the_band(r):
    """Mutant 6: pairs that straddle rows and planes: the count differs on every row with more than one row of voxels, and
    sums[0] is out of band -- but for the heavy rows (one straddling pair among 393 216) and kappa = 1e4 (the few straddling
    pairs may all have the weight 0), which the count alone catches."""
    T = I.data(r)
    R_ = I.results(r, T)
    s1, n = I.smooth_sums_mutant(r, T, "flat")
    (rf, scale, tol), cnt = R_["sum0"], int(R_["sum1"][0])
    assert n > cnt, (cnt, n)
    if r["kind"] == "mix" and r["kappa"] < 1e4:
        assert float((s1 - rf).abs()) > tol * float(scale)


def test_sum_mutants_restate_the_reference():
    """The two sum mutants are the reference where their defect cannot show: a volume of one trip, a single row of voxels."""
    r = L.make("fs_fwd", "-", B=2, C=3, D=3, H=4, W=5, kind="mix", guide=True, kappa=12.5)
    T = I.data(r)
    rf = I.results(r, T)
    s1, n = I.smooth_sums_mutant(r, T, "first_trip")
    assert n == int(rf["sum1"][0]) and abs(float(s1 - rf["sum0"][0])) <= 1e-12 * float(rf["sum0"][0])
    r = L.make("fs_fwd", "-", B=2, C=3, W=9, kind="mix", guide=True, kappa=12.5)
    T = I.data(r)
    rf = I.results(r, T)
    s1, n = I.smooth_sums_mutant(r, T, "flat")
    assert n == int(rf["sum1"][0]) and abs(float(s1 - rf["sum0"][0])) <= 1e-12 * float(rf["sum0"][0])
