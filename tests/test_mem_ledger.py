"""CPU (no GPU needed): the ledger of the warp and resize kernels (tests/mem_ledger.py) against the product build.

Completeness: the kernels hipcc compiles from warp3d.hip / interp.hip are exactly the kernels the ledger's rows expect plus
UNREACHABLE_IN_PRODUCT plus helpers -- a new instantiation without a row fails, and so does a row or an unreachable entry
whose kernel no longer exists.  Plan agreement: for every warp row with a plan, fs_warp3d_kernel_id (through ops._plan,
placeholder pointers that carry the row's in0 / in1 / flow misalignments) gives it.  Inputs: on every row's inputs the
project's own fp32 oracle agrees with the fp64 reference within the row's band at every voxel (one printed line per row),
which is what lets the GPU test hold the kernels to the same band without exceptions."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import ledger_harness as H  # noqa: E402
import mem_ledger as L  # noqa: E402
import mem_ledger_inputs as I  # noqa: E402

SOURCES = ("warp3d.hip", "interp.hip")


@pytest.fixture(scope="module")
def compiled():
    return H.compiled_kernels(SOURCES, L.normalize)


def test_every_compiled_kernel_has_a_row(compiled):
    H.assert_complete(compiled, {k for r in L.ROWS for k in L.kernels_of(r)}, L.UNREACHABLE_IN_PRODUCT, L.HELPERS)


def test_rows_are_well_formed():
    ids = [L.row_id(r) for r in L.ROWS]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for r in L.ROWS:
        assert r["op"] in L.WARP_OPS + L.RESIZE_OPS, r
        assert r["why"], r
        assert all(0 <= m <= 3 for m in r["mis"].values()), r
        assert all(k in I.FLOW_KINDS for k in r["flow"]), r
        assert r["plan"] in (None, L.GATHER, L.RC), r
        if r["op"] not in L.WARP_OPS or r["op"].startswith("uw_"):
            assert r["plan"] is None, r  # the query describes fs_warp3d[_pair]_{fwd,bwd*} only
        assert r["factor"] in ((0,) if r["op"] in ("w_fwd", "w_bwd", "wp_fwd", "wp_bwd", "wp_acc", "wp_acc3") else (2, 4)), r
        assert len(L.kernels_of(r)) == (2 if r["op"] in ("uw_bwd", "uw_bwd3") else 1), r


def test_every_threshold_has_rows_on_both_sides():
    """The rows that name each rung's threshold: a row on each side for every one of them (spot check of the ledger's own
    reasons, so a deleted side is noticed)."""
    whys = " | ".join(r["why"] for r in L.ROWS)
    for needle in ("row cache: C = 1", "row cache: C = 2", "W_in = 72", "W_in = 68 < 72", "D_in = 37", "D_in = 36 < 37",
                   "row cache: W_in % 4 != 0", "row cache: in0 misaligned", "row cache: in1 misaligned",
                   "row cache backward: without grad_in", "row cache backward: with grad_in",
                   "grad_flow null with grad_in set", "pick_dc stays at 64", "pick_dc shrinks to 8", "1022 < 1024",
                   "D = 6 smaller than the chosen dc", "global-gather fallback", "restarts the row ring",
                   "the ring slot wraps", "discontinuity every slice", "window origin 10 columns",
                   "strictly holds the window (fwd)", "strictly holds the window (bwd)",
                   "strictly holds the window (acc3)",
                   "D = 2 below the 4 ring stages", "D = 3 below the 4 ring stages", "D = 2 below the 3 ring stages",
                   "D = 17 not a multiple of 16", "H = 63 below a tile", "at a tile", "H = 65 one above a tile",
                   "W = 28 below a tile", "W = 36 one above a tile",
                   "vec_ok fwd: flow misaligned", "vec_ok fwd: out0 misaligned", "vec_ok fwd: out1 misaligned",
                   "vec_ok fwd: in0 misaligned, not inspected", "W % 4 != 0",
                   "vec_ok bwd: flow misaligned", "vec_ok bwd: gflow misaligned", "vec_ok bwd: gout0 misaligned",
                   "vec_ok bwd: gout1 misaligned", "vec_ok bwd: add0 misaligned", "vec_ok bwd: add1 misaligned",
                   "vec_ok bwd: add2 misaligned", "vec_ok bwd: in0 misaligned, not inspected",
                   "vec_ok bwd: grad_in misaligned, not inspected",
                   "stride of add0 % 4", "stride of add1 % 4", "stride of add2 % 4", "stride of gout0 % 4",
                   "stride of gout1 % 4", "acc3: 0 addends", "acc3: 1 strided", "acc3: 2 addends", "acc3: 3 addends",
                   "aliases grad_flow6",
                   "x2 without prev_flow", "x2 with prev_flow", "x4 with prev_flow", "x4 without prev_flow",
                   "images larger than the flow", "vec_ok upsample-warp: prev misaligned",
                   "vec_ok upsample-warp: fout misaligned", "vec_ok upsample-warp: out0 misaligned",
                   "vec_ok upsample-warp: out1 misaligned", "vec_ok upsample-warp: delta misaligned, not inspected",
                   "backward x2", "backward x4", "backward3 x2", "backward3 x4",
                   "upsample tile x2", "upsample tile x4", "Wo = 64", "Wo = 60", "Do = 8", "Do = 12", "Ho = 8", "Ho = 12",
                   "upsample: out misaligned", "upsample: prev misaligned", "Wo = 62, Wo % 4 != 0",
                   "upsample: small misaligned, not inspected",
                   "downsample v4 /2", "downsample v4 /4", "downsample: in misaligned", "Win % 4 != 0 with Wo = 4",
                   "Wo = 6, Wo % 4 != 0", "downsample: out misaligned", "multi-source /2", "multi-source /4",
                   "multi-source stride with % 4 != 0", "multi-source: src1 misaligned",
                   "down exact v4<unsigned>", "down exact scalar (Win = 6", "down exact scalar (grad_in misaligned)",
                   "floor extents /2 -> adjoint<3>", "up x2 with workspace -> fused", "up x4 with workspace -> separable",
                   "up x2 without workspace -> adjoint<4>", "up x4 without workspace -> adjoint<8>", "scale = 2",
                   "scale = 4", "scale = 1/4",
                   "resize2d forward up x2", "resize2d forward down /2", "resize2d backward down /2",
                   "resize2d backward up x2", "resize2d backward up x4"):
        assert needle in whys, needle


def test_plan_agrees_with_every_warp_row():
    from opticalflowscivis_amd import _lib, ops
    _lib.lib()  # the library is the project's own artifact: not built or not loadable is a failure, not a skip
    bad, n = [], 0
    for r in L.ROWS:
        if r["plan"] is None:
            continue
        n += 1
        m = r["mis"]
        mis = (4 * m.get("in0", 0), 4 * m.get("in1", 0), 4 * m.get("flow", 0))
        family = "warp3d_bwd" if r["op"] in L.BWD_OPS else "warp3d_fwd"
        geo = (r["B"], r["C"], *I.img_ext(r), *I.flow_ext(r), int(r["with_grad_in"]))
        pid = ops._plan(family, mis, geo)[0]
        if pid != r["plan"]:
            bad.append((L.row_id(r), "plan %r, expected %r" % (pid, r["plan"])))
        want = {L.RC: (L.RC_B if family == "warp3d_bwd" else L.RC_F,)}.get(r["plan"])
        if want is not None and L.kernels_of(r) != want:
            bad.append((L.row_id(r), "plan names the row cache, the row %s" % (L.kernels_of(r),)))
        if r["plan"] == L.GATHER and any(k in (L.RC_F, L.RC_B) for k in L.kernels_of(r)):
            bad.append((L.row_id(r), "plan names the gather kernels, the row the row cache"))
    assert n > 40
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.parametrize("r", L.ROWS, ids=[L.row_id(r) for r in L.ROWS])
def test_inputs_keep_the_fp32_oracle_inside_the_band(r):
    T = I.data(r)
    ref = I.results(r, T, torch.float64)
    orc = I.results(r, T, torch.float32)
    worst = {}
    for name, (rf, tol) in ref.items():
        assert torch.isfinite(rf).all(), name
        worst[name] = float((orc[name][0].double() - rf).abs().max()) / I.band(rf, tol)
    print("ORACLE %-100s %s" % (L.row_id(r), " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))
    assert ref and all(v <= 1.0 for v in worst.values()), worst
