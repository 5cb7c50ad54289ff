"""CPU (no GPU needed): the ledger of the 2-D warp, occlusion and Laplacian-pyramid kernels (tests/w2lap_ledger.py)
against the product build.

Completeness: the kernels hipcc compiles from warp2d.hip / laplacian.hip / laplacian3d.hip are exactly the kernels the
ledger's rows expect plus helpers, and nothing is listed as unreachable.  Dispatch: a restatement of slices_for / launch_fwd
/ launch_bwd predicts every warp row's kernels and (NC, CG); the library's own size queries agree with the restated buffer
sizes.  Inputs: on every row the margins hold (sample coordinates off the cell boundaries, |lhs - thresh| and the outgoing
positions off their thresholds, |lap| off zero by 8 x the fp32 error), the fp32 and fp64 restatements of the kernels'
decisions are equal at every element (masks of the dyadic rows included), and the project's fp32 oracle agrees with the
fp64 reference within the row's band at every element (one printed line per row) -- which is what lets the GPU test hold
the kernels to the same bands without exceptions."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import ledger_harness as H  # noqa: E402
import w2lap_ledger as L  # noqa: E402
import w2lap_ledger_inputs as I  # noqa: E402
from oracle import ifnet_ref, warps as owarps  # noqa: E402

SOURCES = ("warp2d.hip", "laplacian.hip", "laplacian3d.hip")
IDS = [L.row_id(r) for r in L.ROWS]


@pytest.fixture(scope="module")
def compiled():
    return H.compiled_kernels(SOURCES, L.normalize)


def test_every_compiled_kernel_has_a_row(compiled):
    assert not L.UNREACHABLE, "every kernel of these sources is reachable at a test-sized tensor"
    H.assert_complete(compiled, {k for r in L.ROWS for k in L.kernels_of(r)}, L.UNREACHABLE, L.HELPERS)
    ours = {k for k in compiled if k.startswith(L.PREFIXES)}
    assert len(ours) == 51 + 4 + 4 and ours == compiled - L.HELPERS, sorted(compiled - ours)


def test_rows_are_well_formed():
    assert len(IDS) == len(set(IDS)), sorted(i for i in IDS if IDS.count(i) > 1)
    for r in L.ROWS:
        assert r["op"] in L.OPS and r["why"], r
        assert all(0 <= m <= 3 for m in r["mis"].values()), r
        assert r["flow"] in I.FLOW_KINDS, r
        if r["op"] in L.WARP_OPS:
            assert r["mode"] in (L.RIFE, L.PWC, L.PHOTO, L.DILATED), r
            assert not r["mask"] or (r["mode"] == L.PWC and r["flow"] == "dyadic"), r
            assert not r["start"] or r["mode"] == L.DILATED, r
            assert r["inp"] is None or r["mode"] == L.RIFE, r
            assert r["op"] in L.BWD_OPS or not (r["gin"] or r["alias"]), r
            assert r["gin"] or r["gflow"], r
            assert not (r["op"] in L.PAIR_OPS and (r["mask"] or r["start"])), r
            if r["mask"]:  # dyadic: W - 1 and H - 1 powers of two
                assert all((n - 1) & (n - 2) == 0 and n >= 2 for n in r["ext"]), r
        elif r["op"] == "occ":
            assert r["mode"] in (L.OCC_ALL, L.OCC_OBJ, L.OCC_OUT) and r["kernel"] == (L.OCC,), r
        else:
            nd = 2 if r["op"].startswith("l2") else 3
            assert len(r["ext"]) == nd and 1 <= r["levels"] <= 8 and r["gl"] in (1.0, -2.5), r
            assert r["kernel"] == {"l2_fwd": L.L2_FWD, "l2_bwd": L.L2_BWD, "l3_fwd": L.L3_FWD, "l3_bwd": L.L3_BWD}[r["op"]], r
            assert all(min(e) >= 3 for e in I.lap_sizes(r)[0][:-1]), r
            assert r["margin"] == (1e-3 if r["data"] == "cb" else 1e-5), r


def test_the_restated_dispatch_predicts_every_warp_row():
    n = 0
    for r in L.ROWS:
        if r["op"] not in L.WARP_OPS:
            continue
        n += 1
        ks, nc = I.predict(r)
        assert ks == r["kernel"], (L.row_id(r), ks)
        if r["nc"] is not None:
            assert nc == r["nc"], (L.row_id(r), nc)
    assert n > 80
    fwd = {k for r in L.ROWS for k in r["kernel"] if k.startswith("warp2d_fwd")}
    bwd = {k for r in L.ROWS for k in r["kernel"] if k.startswith("warp2d_bwd")}
    plane = {k for r in L.ROWS for k in r["kernel"] if k.startswith("warp2d_gin_plane")}
    assert (len(fwd), len(bwd), len(plane)) == (15, 30, 5)


def test_every_threshold_has_rows_on_both_sides():
    """The rows that name each rung's threshold: a row on each side for every one of them (a deleted side is noticed)."""
    whys = " | ".join(r["why"] for r in L.ROWS)
    for needle in ("C = 3 < 4", "C = 4 at small n", "C = 15 < 16", "C = 16 at n < 32768", "n = 32767", "n = 32768",
                   "n = 131071", "n = 131072", "grad_in only -> the plane kernel alone", "grad_flow only",
                   "both, the plane fits", "96 x 128) fits", "96 x 129 does not fit",
                   "the flow's plane fits (96 x 128), the image's does not", "the flow's plane does not fit (96 x 129)",
                   "B*C = 6 < 512: nc = 1", "B*C = 1024", "B*C = 1022", "nc = 12, CG = 17", "fill = 2 is cut to C = 1",
                   "plane kernel RIFE: B*C = 1088", "plane kernel PWC: B*C = 1088", "plane kernel PWC masked: B*C = 1088",
                   "plane kernel PHOTO: B*C = 1088", "plane kernel DILATED: B*C = 1088",
                   "pair forward RIFE", "pair forward PHOTO", "pair backward RIFE, distinct", "grad_img0 == grad_img1",
                   "pair backward PHOTO", "grid cap: n = 4194304", "grid cap: n = 4194305", "grid cap backward: n = 4194304",
                   "grid cap backward: n = 4194305, second trip", "with grad_in through the atomic kernel",
                   "DILATED: start NULL", "DILATED: start given", "start given together with slices",
                   "tiny: PWC at 1 x 1", "tiny: PWC at 1 x 7", "tiny: PWC at 6 x 1", "tiny: PHOTO at 1 x 1",
                   "tiny: DILATED at 1 x 1", "tiny: DILATED at 6 x 1", "RIFE at 2 x 2",
                   "fs_warp2d_fwd, every operand misaligned", "fs_warp2d_bwd, every operand misaligned",
                   "fs_warp2d_pair_fwd, every operand misaligned", "fs_warp2d_pair_bwd, every operand misaligned",
                   "occ mode ALL", "occ mode OBJ", "occ mode OUT", "occ: H = 1", "occ: W = 1", "occ grid cap: n = 4194304",
                   "occ grid cap: n = 4194305", "fs_occ_check2d, every operand misaligned", "occ exact",
                   "2-D extents 3 x 3, levels = 1, N = 1", "2-D extents 3 x 3, levels = 1, N = 3",
                   "2-D extents 3 x 9, levels = 1, N = 1", "2-D extents 3 x 9, levels = 1, N = 3",
                   "17 x 33 at levels = 1", "17 x 33 at levels = 4", "257 x 257 at levels = 8", "2-D target NULL",
                   "2-D target given", "N*H*W = 131072", "N*H*W = 131073", "2-D grid cap, fine kernels: N*H*W = 4194304",
                   "2-D grid cap, fine kernels: N*H*W = 4194306", "2-D backward grid cap, fine kernels: N*H*W = 4194304",
                   "2-D backward grid cap, fine kernels: N*H*W = 4194306", "2-D exact", "fs_laploss2d_fwd, every operand",
                   "fs_laploss2d_bwd, every operand", "3-D extents 3 x 3 x 3", "one axis odd, the others even",
                   "33 x 17 x 9 at levels = 1", "33 x 17 x 9 at levels = 2", "65^3 at levels = 6", "3-D target NULL",
                   "3-D target given", "N*D*H*W = 262144", "N*D*H*W = 262145", "3-D exact",
                   "fs_laploss3d_fwd, every operand", "fs_laploss3d_bwd, every operand"):
        assert needle in whys, needle
    exts2 = {e for r in L.ROWS if r["op"] == "l2_fwd" and r["levels"] == 1 for e in r["ext"]}
    assert {3, 4, 5, 6, 7, 8, 9} <= exts2
    for op in ("w_fwd", "w_bwd", "wp_fwd", "wp_bwd", "occ", "l2_fwd", "l2_bwd", "l3_fwd", "l3_bwd"):
        full = [r for r in L.ROWS if r["op"] == op and r["mis"]]
        assert full and all(v > 0 for r in full for v in r["mis"].values()), op


def test_the_size_queries_agree_with_the_restated_buffer_sizes():
    from opticalflowscivis_amd import _lib
    lib = _lib.lib()  # the library is the project's own artifact: not built or not loadable is a failure, not a skip
    for r in L.ROWS:
        if r["op"] not in L.LAP_OPS:
            continue
        out = [ctypes.c_longlong(0) for _ in range(3)]
        fn = lib.fs_laploss2d_sizes if len(r["ext"]) == 2 else lib.fs_laploss3d_sizes
        assert fn(r["B"], *r["ext"], r["levels"], *[ctypes.byref(o) for o in out]) == 0, L.row_id(r)
        assert tuple(o.value for o in out) == I.lap_sizes(r)[1:], L.row_id(r)


def test_the_pyramid_restatement_is_the_oracle():
    g = torch.Generator().manual_seed(5)
    for ext, fn in (((2, 3, 17, 22), ifnet_ref.lap_loss), ((2, 1, 9, 12, 11), ifnet_ref.lap_loss3d)):
        a, b = torch.randn(*ext, generator=g), torch.randn(*ext, generator=g)
        for levels in (1, 2):
            want = float(fn(a.double(), b.double(), levels)) if len(ext) == 5 else float(fn(a, b, levels))
            laps = I.pyramid((a.double() - b.double()).reshape(-1, *ext[2:]), levels)
            got = float(sum(p.abs().mean() for p in laps))
            assert abs(got - want) <= (1e-12 if len(ext) == 5 else 2e-6) * max(1.0, abs(want)), (ext, levels, got, want)


def test_generic_flows_leave_the_mask_undefined_and_dyadic_ones_do_not():
    """The disagreement that keeps mask parity on generic flows out of the ledger, and its absence on the
    dyadic inputs the masked rows use."""
    g = torch.Generator().manual_seed(0)
    r = dict(L.ROWS[0], ext=(37, 130), B=2, mask=1, mode=L.PWC, inp=None)
    flow = torch.randn(2, 2, 37, 130, generator=g) * 2
    c32, c64 = I.chain(r, flow, None, torch.float32), I.chain(r, flow, None, torch.float64)
    n32, n64 = int((c32["mask"] & c64["interior"]).sum()), int((c64["mask"] & c64["interior"]).sum())
    print("generic 2x2x37x130: interior %d, fp32 mask 1 at %d, fp64 at %d" % (int(c64["interior"].sum()), n32, n64))
    assert n32 != n64
    for ext in ((5, 9), (9, 17), (17, 33), (33, 65), (3, 5), (2, 3)):
        r = dict(r, ext=ext)
        flow = I.dyadic_flow(2, *ext, g)
        c32, c64 = I.chain(r, flow, None, torch.float32), I.chain(r, flow, None, torch.float64)
        assert torch.equal(c32["mask"], c64["mask"]) and torch.equal(c32["msum"].double(), c64["msum"]), ext
        assert bool((c32["msum"][c32["interior"]] == 1).all()), ext
        assert bool((c32["msum"][~c32["interior"]] <= 1 - 1.0 / 32).all()), ext


def test_the_wide_flows_clamp_on_all_four_sides():
    rows = [r for r in L.ROWS if r["flow"] == "wide"]
    assert len(rows) >= 3 and all(r["mode"] == L.DILATED for r in rows)
    for r in rows:
        T = I.data(r)
        c, _, top = I.coords(r, T["flow"], T.get("start"))
        for a in range(2):
            assert bool((c[:, a] < -1).any()) and bool((c[:, a] > top[a] + 1).any()), (L.row_id(r), a)


@pytest.mark.parametrize("r", [r for r in L.ROWS if r["spike"]], ids=[L.row_id(r) for r in L.ROWS if r["spike"]])
def test_a_dropped_second_trip_leaves_the_band(r):
    """The rows one item beyond a cap put 100 at the last element: the loss without that element's term is outside the
    band, so a kernel whose grid-stride loop never took its second trip cannot pass (its sgn element stays NaN as well)."""
    cap = 512 if r["op"] == "l2_fwd" else 1024
    n = r["B"] * I.numel(r["ext"])
    assert n > 256 * cap and (n - 1) >= 256 * cap, r  # the last element belongs to the second trip of lap*_level_kernel
    short, loss, bnd = I.dropped_second_trip(r, I.data(r))
    assert abs(loss - short) > 4 * bnd, (short, loss, bnd)


@pytest.mark.parametrize("r", L.ROWS, ids=IDS)
def test_inputs_keep_the_fp32_oracle_inside_the_band(r):
    T = I.data(r)
    assert all(t.dtype == torch.float32 for t in T.values())
    for what, dist, promised in I.margins(r, T):
        assert dist >= promised, "%s: %g < %g" % (what, dist, promised)
    d64, d32 = I.decisions(r, T, torch.float64), I.decisions(r, T, torch.float32)
    for what in d64:
        assert torch.equal(d64[what], d32[what]), "fp32 and fp64 decide '%s' differently at %d elements" % (
            what, int((d64[what] != d32[what]).sum()))
    if r["op"] in L.WARP_OPS and r["mask"]:
        for i in range(2 if r["op"] in L.PAIR_OPS else 1):
            c = I.chain(r, T["flow"][:, 2 * i:2 * i + 2], None, torch.float32)
            assert bool((c["msum"][c["interior"]] == 1).all()), "interior weight sums are not exactly 1"
            share = float(c["mask"].float().mean())
            assert share >= 0.25 and 1 - share >= 0.1, "mask 1 at %.3f of the pixels" % share
    ref = I.results(r, T, torch.float64)
    orc = I.results(r, T, torch.float32)
    worst = {}
    for name, (rf, tol) in ref.items():
        assert torch.isfinite(rf).all(), name
        if tol is None:
            assert torch.equal(orc[name][0].double(), rf.double()), "%s: the fp32 oracle differs from the exact expectation" % name
            worst[name] = 0.0
        else:
            worst[name] = float((orc[name][0].double() - rf).abs().max()) / I.band(rf, tol)
    print("ORACLE %-90s %s" % (L.row_id(r), " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))
    assert ref and all(v <= 1.0 for v in worst.values()), worst
