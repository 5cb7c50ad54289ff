"""CPU (no GPU needed): the ledger of the correlation and plane-moment kernels (tests/corr_ledger.py) against the product build.

Completeness, per source: the kernels hipcc compiles from corr2d.hip and from corr3d.hip for gfx950 are exactly the kernels
that source's rows expect plus helpers (the two sources share normalised names, so the key is (source, kernel)).  Rows: a
threshold pair differs in the one field it names, and every row's kernel is the one a Python restatement of the dispatch
code picks.  Inputs: on every row the fp32 oracle is inside the band of the float64 reference at every element, meets the
exact expectations and has the reference's non-finite set -- which is what lets the GPU test hold the kernels to the same
bands without leaving an element out.  Sensitivity: on named rows the reference without the last channel, the last
channel slice of a direct row, the last displacement row, the second 256-stride trip of a moments row or the one channel
past a 32-channel group leaves the band."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import ledger_harness as H  # noqa: E402
import corr_ledger as L  # noqa: E402
import corr_ledger_inputs as I  # noqa: E402

IDS = [L.row_id(r) for r in L.ROWS]


@pytest.mark.parametrize("src", L.SOURCES)
def test_every_compiled_kernel_has_a_row(src):
    assert not L.UNREACHABLE, "every kernel of both sources is reachable at a test-sized tensor"
    compiled = H.compiled_kernels((src,), H.normalize)
    H.assert_complete(compiled, {k for r in L.ROWS if r["src"] == src for k in L.kernels_of(r)}, L.UNREACHABLE, L.HELPERS)


def test_rows_are_well_formed():
    assert len(IDS) == len(set(IDS)), sorted(i for i in IDS if IDS.count(i) > 1)
    assert {r["op"] for r in L.ROWS} == set(L.OPS)
    for r in L.ROWS:
        assert r["why"] and r["src"] in L.SOURCES, r
        assert all(0 <= m <= 3 for m in r["mis"].values()), r
        assert len(r["kernel"]) == (4 if r["op"] == "chain" else 1), r
        if r["op"] in I.MOMENT_OPS:
            assert r["planes"] >= 1 and r["S"] >= 2, r
        else:
            assert 1 <= r["md"] <= 4 and min(I.shape5(r)) >= 1 and (r["D"] == 1 or r["op"].startswith("c3_")), r
        if r["op"] in L.GRADS_OF:
            assert r["grads"] and set(r["grads"]) <= set(L.GRADS_OF[r["op"]]), r
        else:
            assert not r["grads"], r
        T = I.data(r)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in T.values()), r
        assert set(r["mis"]) <= set(T) | set(I.out_sizes(r)), r
        assert not set(T) & set(I.out_sizes(r)), r


def test_threshold_pairs_differ_in_one_field():
    pairs = {}
    for r in L.ROWS:
        if r["pair"]:
            pairs.setdefault(r["pair"], []).append(r)
    assert len(pairs) >= 16
    for (tag, field), rows in pairs.items():
        assert len(rows) == 2, tag
        a, b = rows
        differ = {k for k in a if a[k] != b[k]} - {"kernel", "why"}
        assert differ == {field}, (tag, differ)
        assert abs(a[field] - b[field]) == (8 if tag.startswith("mean4") else 1), tag


def expected_kernel(r):
    """The dispatch code of corr2d.hip / corr3d.hip restated (launch_fwd, launch_bwd, launch_small_fwd)."""
    op, md = r["op"], r["md"]
    if op in ("mom", "mom4"):
        return (L.MOM,)
    if op in ("nb", "nb4"):
        return (L.NB,)
    if op == "chain":
        return (L.MOM,) + expected_kernel(dict(r, op="p_fwd")) + expected_kernel(dict(r, op="p_bwd")) + (L.NB,)
    if op.startswith("c3_"):
        return (L.TF(md) if op == "c3_fwd" else L.TB(md),)
    hw = r["H"] * r["W"]
    if op.endswith("_bwd"):
        return (L.SB(md) if hw <= L.K_SMALL_BWD else L.TB(md),)
    normed = op == "n_fwd" or r["stats"]
    if hw > (L.K_SMALL_FWD_NORM if normed else L.K_SMALL_FWD):
        return (L.TF(md),)
    items, cs = r["B"] * (2 * md + 1) ** 2 * hw, 1
    while cs < 8 and items * cs < L.ITEM_CAP and r["C"] // (2 * cs) >= L.SLICE_MIN_CHANNELS:
        cs *= 2
    return (L.SF(md, cs),)


@pytest.mark.parametrize("r", L.ROWS, ids=IDS)
def test_row_names_the_kernel_the_dispatch_code_picks(r):
    assert L.kernels_of(r) == expected_kernel(r)


def test_the_thresholds_are_the_sources():
    with open(os.path.join(H.CSRC, "corr2d.hip")) as f:
        src = f.read()
    assert "constexpr int kSmallFwd = %d, kSmallFwdNorm = %d, kSmallBwd = %d;" % (
        L.K_SMALL_FWD, L.K_SMALL_FWD_NORM, L.K_SMALL_BWD) in src
    assert "items * cs < 256ll * 256 * 2 && C / (2 * cs) >= %d" % L.SLICE_MIN_CHANNELS in src and 256 * 256 * 2 == L.ITEM_CAP


def test_every_rung_has_its_rows():
    """The rungs the ledger's docstring and reasons speak of, counted from the rows' fields (a deleted side is noticed)."""
    def rows(op, **kw):
        return [r for r in L.ROWS if r["op"] == op and all(r[k] == v for k, v in kw.items())]
    assert {(r["md"], r["kernel"][0]) for r in rows("c2_fwd")} >= {(md, L.SF(md, cs)) for md in (1, 2, 3, 4) for cs in (1, 2, 4, 8)}
    for C in (1, 7, 8, 9, 16, 17):
        assert {r["md"] for r in rows("c2_fwd", C=C) if r["kernel"] == (L.TF(r["md"]),)} == {1, 2, 3, 4}, C
    for C in (1, 2, 3, 31, 32, 33, 65):
        assert [r for r in rows("c2_bwd", C=C) if r["kernel"][0].startswith("corr_bwd_q")], C
    for C in (33, 65):
        assert {r["grads"] for r in rows("c2_bwd", C=C, poison=None)} == {("g1",), ("g2",), ("g1", "g2")}, C
    for md, Ds in ((1, (1, 2, 3, 4)), (2, (1, 2, 3, 5, 6)), (4, (1, 2, 4, 5, 9, 10))):
        for op in ("c3_fwd", "c3_bwd"):
            assert {r["D"] for r in rows(op, md=md)} >= set(Ds), (op, md)
    assert {r["grads"] for r in rows("p_bwd")} >= {(g,) for g in L.GRADS_OF["p_bwd"]}
    assert {r["grads"] for r in rows("nb4")} >= {(g,) for g in L.GRADS_OF["nb4"]}
    assert {len(r["grads"]) for r in rows("nb4")} == {1, 3, 4}
    for op in ("mom", "nb"):
        assert {(r["S"], r["planes"]) for r in rows(op)} >= {(S, p) for S in (2, 3, 24, 255, 256, 257, 512, 513, 4294) for p in (1, 3)}
    assert {r["kind"] for r in rows("mom")} == {"rand", "const", "offset"}
    assert {r["alias"] for r in rows("mom4")} == {False, True} and {r["alias"] for r in rows("chain")} == {False, True}
    poisoned = {(r["src"], r["kernel"][0].split("<")[0], r["op"][-3:]) for r in L.ROWS if r["poison"]}
    assert poisoned == {(L.SRC2, "corr2d_small_fwd_kernel", "fwd"), (L.SRC2, "corr2d_small_bwd_kernel", "bwd"),
                        (L.SRC2, "corr_fwd_q_kernel", "fwd"), (L.SRC2, "corr_bwd_q_kernel", "bwd"),
                        (L.SRC3, "corr_fwd_q_kernel", "fwd"), (L.SRC3, "corr_bwd_q_kernel", "bwd")}
    assert {m for r in L.ROWS for k, m in r["mis"].items() if k.startswith("st")} >= {1, 3}


@pytest.mark.parametrize("r", L.ROWS, ids=IDS)
def test_inputs_keep_the_fp32_oracle_inside_the_band(r):
    T = I.data(r)
    ref, orc = I.results(r, T), I.oracle(r, T)
    assert set(ref) == set(orc) and ref
    sizes = I.out_sizes(r)
    worst = {}
    for name, (rf, band) in ref.items():
        assert r["poison"] or bool(torch.isfinite(rf).all()), name
        assert bool((band >= 0).all()) or r["poison"], name
        if name in sizes:
            assert rf.numel() == sizes[name], name
        err, inexact, same_set = I.compare(orc[name].float(), rf, band, poison=bool(r["poison"]))
        assert same_set, "%s: the oracle's non-finite set is not the reference's" % name
        assert inexact == 0, "%s: %d elements miss their exact expectation" % (name, inexact)
        worst[name] = err
    if r["poison"]:  # a poison row poisons something, and not everything
        bad = sum(int((~torch.isfinite(rf)).sum()) for rf, _ in ref.values())
        assert 0 < bad < sum(rf.numel() for rf, _ in ref.values())
    print("ORACLE %-70s %s" % (L.row_id(r), " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_exact_expectations_are_where_the_ledger_says():
    """Displacement planes outside the volume and constant planes give exact zeros (band == 0), and nothing else does on
    random data apart from windows that are all padding."""
    r = next(r for r in L.ROWS if r["op"] == "c3_fwd" and r["md"] == 4 and r["D"] == 2)
    T = I.data(r)
    rf, band = I.results(r, T)["out"]
    v = band.expand_as(rf).view(r["B"], 9, 81, 2, r["H"], r["W"])
    assert bool((v[:, :3] == 0).all()) and bool((v[:, 6:] == 0).all())  # |dz| >= 2 never lands inside D = 2
    assert bool((v[:, 3, :, 0] == 0).all()) and bool((v[:, 5, :, 1] == 0).all())  # dz = -1 at z = 0, dz = +1 at z = 1
    assert bool((v[:, 4, 40] > 0).all()) and bool((v[:, 3, 40, 1] > 0).all())
    for op, name in (("n_fwd", "out"), ("n_bwd", "g1"), ("n_bwd", "g2")):
        for r in (r for r in L.ROWS if r["op"] == op and r["kind"] == "const"):
            rf, band = I.results(r, I.data(r))[name]
            band = band.expand_as(rf)
            if op == "n_fwd" and r["C"] == 1:
                assert bool((band == 0).all()) and bool((rf == 0).all())
            elif op == "n_bwd":
                assert bool((band[:, -1] == 0).all()) and bool((band[:, 0] > 0).all())


# ---- sensitivity of the bands: an omission leaves them ----------------------------------------------------------------------
def _row(op, **kw):
    (r,) = [r for r in L.ROWS if r["op"] == op and not r["mis"] and not r["poison"] and r["pair"] is None and
            all(r[k] == v for k, v in kw.items())][:1]
    return r


def _leaves(full, band, cut):
    """Fraction of the elements with a band (not the exact zeros) at which `cut` is outside the band of `full`."""
    band = band.expand_as(full)
    return float(((full - cut).abs() > band)[band > 0].double().mean())


@pytest.mark.parametrize("C,md", [(9, 4), (17, 2), (1, 1)])
def test_omitting_the_last_channel_leaves_the_band(C, md):
    r = _row("c2_fwd", C=C, md=md, H=5, W=27)
    T = I.data(r)
    rf, band = I.results(r, T)["out"]
    cut = I.corr(T["f1"][:, :C - 1].double(), T["f2"][:, :C - 1].double(), md, 1) * (C - 1) / C if C > 1 else torch.zeros_like(rf)
    assert _leaves(rf, band, cut) > 0.9


def test_omitting_the_last_channel_slice_of_a_direct_row_leaves_the_band():
    r = _row("c2_fwd", C=97, H=8, W=16)
    assert r["kernel"] == (L.SF(4, 8),)
    T = I.data(r)
    rf, band = I.results(r, T)["out"]
    keep = 7 * 13  # 8 slices of 13 channels, the last one holds channels 91 .. 96
    cut = I.corr(T["f1"][:, :keep].double(), T["f2"][:, :keep].double(), 4, 1) * keep / 97
    assert _leaves(rf, band, cut) > 0.5


@pytest.mark.parametrize("op,kw", [("c2_bwd", dict(C=3, H=9, W=31, md=4)), ("c2_bwd", dict(C=5, H=4, W=8, md=1)),
                                   ("c3_bwd", dict(C=3, D=4, md=1))])
def test_omitting_the_last_displacement_row_leaves_the_band(op, kw):
    r = _row(op, grads=("g1", "g2"), **kw)
    T = I.data(r)
    ref = I.results(r, T)
    nd = I.nd_of(r)
    G = T["gout"].clone().view(r["B"], -1, nd, nd, r["D"], r["H"], r["W"])
    G[:, :, nd - 1] = 0  # dy = +md of every dz plane
    cut = I.corr_all(r, T["f1"], T["f2"], None, None, G.view(T["gout"].shape), torch.float64)
    for name, c in zip(("g1", "g2"), cut):
        assert _leaves(ref[name][0], ref[name][1], c) > 0.3, name


@pytest.mark.parametrize("S", [257, 513])
def test_omitting_the_last_stride_trip_of_a_moments_row_leaves_the_band(S):
    r = _row("mom", S=S, planes=3, kind="rand")
    T = I.data(r)
    ref = I.results(r, T)
    short = I.moments(T["f"][:, :S - 1])
    for k, name in enumerate(("mean", "rstd")):
        assert bool(((ref[name][0][0] - short[:, k]).abs() > 4 * ref[name][1][0]).all()), name
    rn = _row("nb", S=S, planes=3, kind="rand")
    T = I.data(rn)
    rf, band = I.results(rn, T)["gf"]
    cut, _ = I._adjoint(T["f"][:, :S - 1], T["stats"], T["gn"][:, :S - 1], torch.float64)
    assert _leaves(rf[:, :S - 1], band[:, :S - 1], cut) > 0.9


@pytest.mark.parametrize("C", [33, 65])
def test_the_channel_past_a_group_is_not_zero_within_the_band(C):
    """C = 33 / 65: a kernel that stopped at the last full 32-channel group and wrote zeros for the channel past it would
    leave the band at that channel (an unwritten one fails on the NaN pattern)."""
    r = _row("c2_bwd", C=C, grads=("g1", "g2"), md=4)
    ref = I.results(r, I.data(r))
    for name in ("g1", "g2"):
        rf, band = ref[name]
        assert _leaves(rf[:, C - 1], band.expand_as(rf)[:, C - 1], torch.zeros_like(rf[:, C - 1])) > 0.9, name
