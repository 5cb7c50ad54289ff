"""CPU (no GPU needed): the convolution ledger (tests/conv_ledger.py) against the product build.

Completeness: the compute kernels hipcc compiles from convfwd.hip / convtr.hip / convwrw.hip are exactly the kernels the
ledger's rows expect plus UNREACHABLE_IN_PRODUCT -- a new instantiation without a row fails, and so does a row or an
unreachable entry whose kernel no longer exists.  Plan agreement: for every row, the library's own plan (the slab kind of
fs_conv3d_{fwd,tr}_wprep_jobs, the FS_WRW_KERNEL_* id of fs_conv3d_wrw_kernel_id, both asked with placeholder pointers
that carry the row's misalignments) is the one of the row's kernel."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ledger as L  # noqa: E402
import ledger_harness as H  # noqa: E402

SOURCES = ("convfwd.hip", "convtr.hip", "convwrw.hip")


@pytest.fixture(scope="module")
def compiled():
    return H.compiled_kernels(SOURCES, L.normalize)


def test_every_compiled_kernel_has_a_row(compiled):
    H.assert_complete(compiled, {r["kernel"] for r in L.ROWS}, L.UNREACHABLE_IN_PRODUCT, L.HELPERS)


def test_rows_are_well_formed():
    ids = [L.row_id(r) for r in L.ROWS]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for r in L.ROWS:
        assert r["op"] in L.FORMS, r
        assert 0 <= r["mis"] <= 3 and 0 <= r["mis2"] <= 3, r
        assert r["why"], r
        L.plan_of(r["kernel"])


def test_every_threshold_has_rows_on_both_sides():
    """The rows that name each rung's threshold: a row on each side for every one of them (spot check of the ledger's
    own reasons, so a deleted side is noticed)."""
    whys = " | ".join(r["why"] for r in L.ROWS)
    for needle in ("exactly 256 bricks", "240 wino2d bricks < 256", "big = 512", "big = 480 < 512", "small = 256",
                   "small = 240 < 256", "Wo == 16", "Wo = 20 > 16", "Wi % 4 != 0", "misaligned", "Cin % 8 == 0",
                   "Cin % 8 != 0", "256 bricks", "255 split-bf16 bricks < 256", "k4tiles = 512", "k4tiles = 510 < 512",
                   "= 512, loader-wave", "= 448 < 512", "big = 256", "big = 224 < 256", "small = 192 < 256",
                   "16 bricks", "15 bricks < 16", "Cin = 32", "Cin = 33 > 32", "Cin = 65 > 64", "Cout <= 2",
                   "3 <= Cout <= 6", "7..16 channels", "17..32 channels", "224 split-bf16 bricks < 256",
                   "exactly 128 bricks", "112 bricks < 128", "output W = 2 Wi + 1", "2 slices", "1024 bricks",
                   "960 Winograd bricks < 1024", "Cs >= 8", "Cs = 7 < 8", "Cg > 32", "Cg = 32", "Cs = 3 < 4",
                   "Cs = 2 < 3", "cost2 1 < cost4 2", "cost2 = cost4", "pad 2 > stride", "src misaligned",
                   "g misaligned", "multi-source"):
        assert needle in whys, needle


def test_plan_agrees_with_every_row():
    from opticalflowscivis_amd import _lib, ops
    try:
        _lib.lib()
    except _lib.FlowsciLibraryError as e:
        pytest.skip("library not built: %s" % e)
    bad = []
    for r in L.ROWS:
        want = L.plan_of(r["kernel"])
        if r["op"].startswith("wrw"):
            geo = (r["B"], r["cout"], r["cin"], *r["out"], *r["inp"], r["k"], r["stride"], r["pad"])
            pid = ops._plan("wrw", (4 * r["mis"], 4 * r["mis2"]), geo)[0]
        elif r["op"].startswith("tr"):
            geo = (r["B"], r["cin"], r["cout"], *r["inp"], *r["out"], int(r["op"] == "tr_prelu"))
            pid = ops._plan("tr", (4 * r["mis"],), geo)[0]
        else:
            geo = (r["B"], r["cin"], r["cout"], *r["inp"], *r["out"], r["k"], r["stride"], r["pad"], r["wmode"])
            pid = ops._plan("fwd", (4 * r["mis"],), geo)[0]
        if pid != want:
            bad.append((L.row_id(r), r["kernel"], "plan %r, expected %r" % (pid, want)))
    assert not bad, "\n".join(map(str, bad))
