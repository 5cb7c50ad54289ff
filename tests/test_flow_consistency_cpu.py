"""CPU: what of the forward-backward consistency measure is checkable without a GPU -- the C-ABI's refusals and
workspace queries (host-side, before any launch), ops.flow_consistency's refusal of CPU tensors, the index rule that
pairs a RIFE model's mid-frame flows into opposite flows, the entry points' argument rules, and the fp64 restatement
(tests/flow_consistency_ref.py) on inputs whose answer is known in closed form."""
import numpy as np
import pytest
import torch

import flow_consistency_ref as ref

NULLPTR, SHAPE, ARG = 1, 2, 3


def test_ws_bytes_queries():
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    for n in (L.fs_flow_consistency2d_ws_bytes(1, 2, 3, 3), L.fs_flow_consistency2d_ws_bytes(32, 2, 150, 450),
              L.fs_flow_consistency3d_ws_bytes(2, 3, 256, 256, 256), L.fs_flow_consistency3d_ws_bytes(2, 3, 1, 5, 9),
              L.fs_flow_consistency3d_ws_bytes(1, 3, 1, 1, 1)):
        assert n > 0 and n % 8 == 0
    assert L.fs_flow_consistency2d_ws_bytes(1, 2, 3, 3) == 13 * 8                 # one workgroup
    assert L.fs_flow_consistency3d_ws_bytes(2, 3, 256, 256, 256) == 1024 * 13 * 8
    assert L.fs_flow_consistency2d_ws_bytes(0, 2, 8, 8) == -SHAPE                 # N < 1
    assert L.fs_flow_consistency2d_ws_bytes(2, 3, 8, 8) == -SHAPE                 # C
    assert L.fs_flow_consistency3d_ws_bytes(2, 2, 8, 8, 8) == -SHAPE              # C
    assert L.fs_flow_consistency3d_ws_bytes(2, 3, 0, 8, 8) == -SHAPE              # an extent < 1
    assert L.fs_flow_consistency2d_ws_bytes(2, 2, 8, -1) == -SHAPE


def test_abi_refusals_without_gpu():
    """Every refusal is decided on the host before anything is launched; the pointers are placeholders that are never
    dereferenced (only NULL-ness and alignment are looked at)."""
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    p = 0x10000
    ok2 = dict(ff=p, fb=p, N=2, C=2, sp=(8, 8), fbs=128, bbs=128, i0=None, i1=None, v=None, a1=0.01, a2=0.5, cm=None,
               rm=None, ws=p, out=p)

    def call(nd, **kw):
        a = dict(ok2 if nd == 2 else dict(ok2, C=3, sp=(8, 8, 8), fbs=1536, bbs=1536))
        a.update(kw)
        fn = L.fs_flow_consistency2d if nd == 2 else L.fs_flow_consistency3d
        return fn(a["ff"], a["fb"], a["N"], a["C"], *a["sp"], a["fbs"], a["bbs"], a["i0"], a["i1"], a["v"], a["a1"],
                  a["a2"], a["cm"], a["rm"], a["ws"], a["out"], None)

    for nd in (2, 3):
        for k in ("ff", "fb", "ws", "out"):
            assert call(nd, **{k: None}) == NULLPTR, (nd, k)
        assert call(nd, N=0) == SHAPE
        assert call(nd, C=5 - nd) == SHAPE                               # 3 in 2-D, 2 in 3-D
        assert call(nd, sp=(0,) + (8,) * (nd - 1)) == SHAPE
        assert call(nd, sp=(8,) * (nd - 1) + (0,)) == SHAPE
        assert call(nd, fbs=nd * 8 ** nd - 1) == SHAPE                   # batch stride below C * P
        assert call(nd, bbs=nd * 8 ** nd - 1) == SHAPE
        assert call(nd, a1=-0.01) == ARG and call(nd, a2=-1.0) == ARG
        assert call(nd, a1=float("nan")) == ARG and call(nd, a2=float("inf")) == ARG
        assert call(nd, i0=p) == ARG and call(nd, i1=p) == ARG           # exactly one image


def test_flow_consistency_refuses_cpu_tensors():
    from opticalflowscivis_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.flow_consistency(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.flow_consistency(torch.zeros(1, 3, 4, 8, 8), torch.zeros(1, 3, 4, 8, 8))


def test_cost_model():
    from opticalflowscivis_amd import ops
    P = 4 * 5 * 6
    b0, f0 = ops.flow_consistency_cost((2, 3, 4, 5, 6), images=False, maps=False)
    b1, f1 = ops.flow_consistency_cost((2, 3, 4, 5, 6), images=True, maps=True)
    assert b0 == 2 * 2 * 3 * P * 4 and b1 == b0 + 2 * P * (8 + 5) and f1 > f0 > 0


def test_rife_consistency_pairs():
    """Pair t = (t, t+g) has mid frame t+h and the flows 2t = mid -> t, 2t + 1 = mid -> t+g."""
    from opticalflowscivis_amd.flow_eval import rife_consistency_pairs, rife_pairs
    assert rife_consistency_pairs(7, 2) == [(1, 2, 1, 2), (2, 3, 3, 4), (3, 4, 5, 6), (4, 5, 7, 8)]
    assert rife_consistency_pairs(7, 4) == [(2, 4, 1, 4)]
    assert rife_consistency_pairs(4, 4) == [] and rife_consistency_pairs(3, 2) == [] and rife_consistency_pairs(1, 2) == []
    for T, g in ((7, 2), (7, 4), (12, 6), (9, 2)):
        pairs = rife_pairs(T, g)
        starts = []  # (from, to) of every flow in the order rife_flows stacks them
        for a, b in pairs:
            starts += [((a + b) // 2, a), ((a + b) // 2, b)]
        got = rife_consistency_pairs(T, g)
        for m, n, i, j in got:
            assert starts[i] == (m, n) and starts[j] == (n, m)
        # every pair of opposite flows the sequence holds is found
        want = sorted((s[0], s[1]) for s in starts if s[0] < s[1] and (s[1], s[0]) in starts)
        assert sorted((m, n) for m, n, _, _ in got) == want
    with pytest.raises(ValueError):
        rife_consistency_pairs(7, 3)


def test_parser_accepts_seq_with_consistency_alone():
    from opticalflowscivis_amd import flow_eval
    for nd in (2, 3):
        ap = flow_eval._common_args(nd, "x")
        a = flow_eval.check_args(ap.parse_args(["--seq", "x.npy", "--consistency"]))
        assert a.consistency and a.gt is None and tuple(a.alpha) == (0.01, 0.5)
        a = flow_eval.check_args(ap.parse_args(["--seq", "x.npy", "--consistency", "--alpha", "0.05", "1"]))
        assert tuple(a.alpha) == (0.05, 1.0)
        with pytest.raises(SystemExit, match="--seq needs --gt"):
            flow_eval.check_args(ap.parse_args(["--seq", "x.npy"]))
        with pytest.raises(SystemExit):
            flow_eval.check_args(ap.parse_args(["--seq", "x.npy", "--consistency", "--zero-baseline"]))
        with pytest.raises(SystemExit):
            flow_eval.check_args(ap.parse_args(["--seq", "x.npy", "--consistency", "--alpha", "-1", "0.5"]))
        a = flow_eval.check_args(ap.parse_args(["--seq", "x.npy", "--gt", "v.npy"]))  # as before
        assert not a.consistency
        a = flow_eval.check_args(ap.parse_args(["--dataset", flow_eval.DATASETS[nd][0]]))
        assert not a.consistency


# ---- the restatement on inputs with a closed-form answer ----

def _shift(N, sp, s):
    """flow_f == s, flow_b == -s (s per channel: along W, H, (D))."""
    C = len(sp)
    ff = np.zeros((N, C) + sp, np.float32)
    for c in range(C):
        ff[:, c] = s[c]
    return ff, -ff


@pytest.mark.parametrize("sp,s", [((5, 7), (2, -1)), ((9, 12), (0, 3)), ((5, 6, 7), (1, -2, 3)), ((1, 5, 9), (-4, 2, 0)),
                                  ((4, 5, 16), (15, 0, -3)), ((3, 3, 3), (0, 0, 0))])
def test_ref_integer_shift(sp, s):
    ff, fb = _shift(2, sp, s)
    cls, r, r2, _ = ref.per_element(ff, fb)
    inside = cls != ref.OUTGOING
    assert set(np.unique(cls)) <= {ref.CONSISTENT, ref.OUTGOING}
    assert np.all(r[inside] == 0) and np.all(np.isnan(r[~inside]))
    C = len(sp)
    S = [sp[C - 1 - c] for c in range(C)]
    P = int(np.prod(sp))
    n_in = int(np.prod([max(S[c] - abs(s[c]), 0) for c in range(C)]))
    out = ref.sums(ff, fb)
    assert np.all(out[:, 0] == P) and np.all(out[:, 2] == P - n_in) and np.all(out[:, 4] == n_in)
    assert np.all(out[:, 1] == 0) and np.all(out[:, 3] == 0) and np.all(out[:, 5] == 0)
    st = ref.stats(ff, fb)
    assert np.all(st["fb_max"] == 0) and np.all(st["occ_frac"] == 0) and np.all(np.isnan(st["warp_psnr"]))
    assert np.allclose(st["out_frac"], (P - n_in) / P)


def test_ref_shift_onto_the_border_is_inside():
    """x + s == S - 1 exactly is inside (and i1 == i0 there: the weight-0 corner repeats the border element)."""
    sp = (4, 6)
    ff, fb = _shift(1, sp, (5, 3))                     # only x = (0, 0) stays: it lands on (W-1, H-1)
    cls = ref.per_element(ff, fb)[0]
    assert cls[0, 0, 0] == ref.CONSISTENT and (cls == ref.OUTGOING).sum() == 23
    ff, fb = _shift(1, sp, (5.0000005, 3))             # the next fp32 value beyond the border is outgoing
    assert (ref.per_element(ff, fb)[0] == ref.OUTGOING).all()
    ff, fb = _shift(1, (1, 1, 1), (0, 0, 0))           # extents of 1: p == 0 == S - 1
    assert ref.per_element(ff, fb)[0].tolist() == [[[[ref.CONSISTENT]]]]


def test_ref_threshold_and_images():
    """A half-element shift of a linear ramp: the bilinear sample is exact, the photometric error 0; a backward flow
    that does not undo the forward one is occluded once the residual passes alpha."""
    H, W = 6, 10
    ff, fb = _shift(1, (H, W), (0.5, 0))
    ramp = np.tile(np.arange(W, dtype=np.float32) / 16, (H, 1))[None]
    st = ref.stats(ff, fb, ramp + np.float32(0.5 / 16), ramp)
    assert st["n_out"][0] == H and st["n_noc"][0] == H * (W - 1) and st["warp_l1"][0] == 0
    assert st["warp_psnr"][0] == np.inf
    fb2 = fb.copy()
    fb2[0, 0, :, 4] += 2.0                             # column 4 of flow_b: sampled with weight 1/2 from x = 3 and x = 4
    cls, r, _, _ = ref.per_element(ff, fb2)
    assert np.all(cls[0, :, 3:5] == ref.OCCLUDED) and np.all(r[0, :, 3:5] == 1.0)   # Fbw = 0.5: 1 > 0.01 * 0.5 + 0.5
    assert np.all(cls[0, :, :3] == ref.CONSISTENT) and np.all(cls[0, :, 5:9] == ref.CONSISTENT)
    assert np.all(ref.per_element(ff, fb2, alpha=(0.0, 1.0))[0][0, :, 3:5] == ref.CONSISTENT)  # r2 == 1 is not > 1


def test_ref_nonfinite_rules():
    sp = (4, 5)
    ff, fb = _shift(1, sp, (1, 0))
    ff[0, 1, 2, 2] = np.nan                            # flow_f itself: nonfinite whatever else holds
    ff[0, 0, 0, 4] = np.inf                            # (would be outgoing were it finite)
    fb[0, 0, 0, 3] = np.inf                            # row 0 (no row above has it as a corner), sampled ...
    cls, r, _, _ = ref.per_element(ff, fb)
    assert cls[0, 2, 2] == ref.NONFINITE and cls[0, 0, 4] == ref.NONFINITE
    assert cls[0, 0, 2] == ref.NONFINITE               # ... with weight 1 from x = 2
    assert cls[0, 0, 1] == ref.NONFINITE               # ... and as the zero-weight corner i0 + 1 of x = 1: 0 * inf = NaN
    assert cls[0, 0, 0] == ref.CONSISTENT and cls[0, 0, 3] == ref.CONSISTENT and cls[0, 1, 4] == ref.OUTGOING
    assert np.isnan(r[0, 0, 1]) and np.isnan(r[0, 2, 2])
    v = np.ones((1,) + sp, bool)
    v[0, 0, 1] = False
    out = ref.sums(ff, fb, valid=v)
    assert out[0, 0] == 19 and out[0, 1] == 3 and out[0, 2] == 3 and out[0, 4] == 13
    assert ref.class_map(ff, fb, valid=v)[0, 0, 1] == ref.NOT_VALID
    # an image: a non-finite img0(x) or sampled img1 makes an inside element nonfinite
    i0 = np.zeros((1,) + sp, np.float32)
    i1 = np.zeros((1,) + sp, np.float32)
    i0[0, 3, 0] = np.nan
    i1[0, 3, 3] = -np.inf
    cls2 = ref.per_element(ff, fb, i0, i1)[0]
    assert cls2[0, 3, 0] == ref.NONFINITE and cls2[0, 3, 2] == ref.NONFINITE and cls2[0, 3, 1] == ref.NONFINITE
    assert cls2[0, 3, 3] == ref.CONSISTENT
