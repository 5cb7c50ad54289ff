"""CPU: the fp64 restatement of the FTLE kernel (tests/ftle_ref.py) on maps with known answers -- a linear map, a
translation, a saddle advected by the advection restatement, a constant map, the difference selection at a border and
beside an ended node -- and what runs without a GPU of the product: costs, lattice seeds, window arithmetic, the
argument errors of ops.ftle and of the C entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

import advect_ref
import ftle_ref as ref

# dyadic entries: A x + b is exact in fp32 on a lattice of multiples of 1/2, so J == A and G == A^T A bit for bit
A2 = np.array([[1.5, 0.25], [-0.5, 0.75]])
A3 = np.array([[1.25, 0.5, -0.25], [0.0, 0.75, 0.5], [-0.5, 0.25, 1.5]])


def _linear(A, shape, refine):
    seeds, lattice, h = ref.lattice_seeds(shape, refine)
    b = np.array([3.0, -1.5, 0.25][:len(shape)])
    pos = (A @ seeds.astype(np.float64) + b[:, None]).astype(np.float32)
    assert (pos.astype(np.float64) == A @ seeds.astype(np.float64) + b[:, None]).all()
    return pos, lattice, h


@pytest.mark.parametrize("refine", [1, 2])
@pytest.mark.parametrize("A,shape", [(A2, (4, 5)), (A3, (3, 4, 5))])
def test_linear_map(A, shape, refine):
    pos, lattice, h = _linear(A, shape, refine)
    assert lattice == tuple((s - 1) * refine + 1 for s in shape) and h == 1.0 / refine
    T = 2.5
    r = ref.ftle(pos, np.zeros(pos.shape[1], np.uint8), lattice, h, T)
    assert (r["cls"] == ref.OK).all()
    G = A.T @ A
    for n, (a, b) in enumerate(ref.PLANES[:len(r["cg"])]):
        np.testing.assert_array_equal(r["cg"][n], np.float32(G[a, b]))
    want = math.log(np.linalg.svd(A, compute_uv=False)[0]) / T
    np.testing.assert_allclose(r["ftle64"], want, rtol=1e-14)
    np.testing.assert_array_equal(r["ftle"], r["ftle64"].astype(np.float32))
    # the border takes one-sided differences, the interior central ones: a linear map cannot tell them apart
    assert (r["kinds"][0][..., 0] == ref.FORWARD).all() and (r["kinds"][0][..., -1] == ref.BACKWARD).all()
    assert (r["kinds"][0][..., 1:-1] == ref.CENTRAL).all()


@pytest.mark.parametrize("shape", [(4, 5), (3, 4, 5)])
def test_translation_is_exactly_zero(shape):
    seeds, lattice, h = ref.lattice_seeds(shape, 2)
    pos = seeds + np.array([0.75, -2.0, 1.5], np.float32)[:len(shape), None]
    r = ref.ftle(pos, np.zeros(pos.shape[1], np.uint8), lattice, h, 3.0)
    assert (r["cls"] == ref.OK).all() and (r["ftle"] == 0.0).all() and not np.signbit(r["ftle"]).any()


def test_saddle_through_the_advection_restatement():
    """u = (a x', -a y') about the centre of a 17 x 17 grid, K Euler steps: x' grows by (1 + a) per step, so interior
    nodes have lambda_max = (1 + a)^(2K); with a = 1/4 every position is exact in fp32.  |x'| >= 5 leaves the box."""
    S, a, K, T = 17, 0.25, 3, 3.0
    c = (S - 1) // 2
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    flows = np.broadcast_to(np.stack([a * (x - c), -a * (y - c)]).astype(np.float32), (K, 2, S, S))
    seeds, lattice, h = ref.lattice_seeds((S, S), 1)
    traj, st, _ = advect_ref.advect(seeds, flows)
    left = np.abs(seeds[0] - c) >= 5
    assert ((st == advect_ref.OUT) == left).all() and (st[~left] == advect_ref.ALIVE).all()
    r = ref.ftle(traj[-1], st, lattice, h, T)
    want = K * math.log(1 + a) / T
    assert ((r["cls"] == ref.ENDED) == left.reshape(lattice)).all() and (r["cls"][~left.reshape(lattice)] == ref.OK).all()
    np.testing.assert_allclose(r["ftle64"][r["cls"] == ref.OK], want, rtol=1e-14)
    assert np.isnan(r["ftle"][r["cls"] == ref.ENDED]).all()
    # with the exit points standing in, every node has a neighbourhood again (the map there is no longer linear)
    r2 = ref.ftle(traj[-1], st, lattice, h, T, accept_out=True)
    assert (r2["cls"] == ref.OK).all()
    inner = np.abs(seeds[0] - c).reshape(lattice) <= 3
    np.testing.assert_array_equal(r2["ftle"][inner], r["ftle"][inner])


@pytest.mark.parametrize("shape", [(3, 4), (2, 3, 4)])
def test_constant_map_is_collapsed(shape):
    seeds, lattice, h = ref.lattice_seeds(shape, 1)
    r = ref.ftle(np.full_like(seeds, 2.5), np.zeros(seeds.shape[1], np.uint8), lattice, h, 1.0)
    assert (r["cls"] == ref.COLLAPSED).all() and np.isnan(r["ftle"]).all() and (r["cg"] == 0.0).all()


def test_difference_selection_at_a_border_and_beside_an_ended_node():
    """phi = (x^2, y): the three differences of x^2 at x are 2x (central), 2x + 1 (forward), 2x - 1 (backward)."""
    seeds, lattice, h = ref.lattice_seeds((3, 7), 1)
    pos = np.stack([seeds[0] ** 2, seeds[1]])
    st = np.zeros(lattice, np.uint8)
    st[1, 3] = advect_ref.OUT
    pos.reshape((2,) + lattice)[:, 1, 3] = np.nan  # never read: (1, 3) enters central differences of its neighbours only
    r = ref.ftle(pos, st.reshape(-1), lattice, h, 1.0)
    C, F, B, N = ref.CENTRAL, ref.FORWARD, ref.BACKWARD, ref.NONE
    assert r["kinds"][0][0].tolist() == [F, C, C, C, C, C, B]          # an undisturbed row
    assert r["kinds"][0][1].tolist() == [F, C, B, C, F, C, B]          # beside the ended node; its own state is not asked
    assert r["kinds"][1][:, 3].tolist() == [N, C, N] and r["kinds"][1][:, 2].tolist() == [F, C, B]
    assert r["cls"][:, 3].tolist() == [ref.ENDED, ref.OK, ref.ENDED] and (np.delete(r["cls"], 3, 1) == ref.OK).all()
    xs = np.arange(7.0)
    np.testing.assert_array_equal(r["cg"][0][0], np.float32(np.array([1, 2, 4, np.nan, 8, 10, 11.0]) ** 2))  # (0, 3) ended
    np.testing.assert_array_equal(r["cg"][0][1], np.float32(np.array([1, 2, 3, 6, 9, 10, 11.0]) ** 2))
    assert np.isfinite(r["ftle"][r["cls"] == ref.OK]).all() and (2 * xs[3]) ** 2 == r["cg"][0][1, 3]
    # accept_out: the node is usable and its NaN is used by its four neighbours (its own central differences skip it)
    r = ref.ftle(pos, st.reshape(-1), lattice, h, 1.0, accept_out=True)
    nf = np.zeros(lattice, bool)
    nf[1, 2] = nf[1, 4] = nf[0, 3] = nf[2, 3] = True
    assert ((r["cls"] == ref.NONFINITE) == nf).all() and (r["cls"][~nf] == ref.OK).all()
    # valid masks the node itself, not its use as a neighbour
    valid = np.ones(lattice, np.uint8)
    valid[0, 0] = valid[1, 2] = 0
    rv = ref.ftle(pos, st.reshape(-1), lattice, h, 1.0, valid=valid)
    assert rv["cls"][0, 0] == ref.NOT_VALID == rv["cls"][1, 2] and np.isnan(rv["ftle"][0, 0]) and np.isnan(rv["cg"][:, 0, 0]).all()
    assert rv["cls"][0, 1] == ref.OK and rv["cg"][0][0, 1] == 4.0


def test_costs_seeds_windows_and_operand_errors():
    from opticalflowscivis_amd import ftle as drv
    from opticalflowscivis_amd import ops
    assert (ops.FTLE_NOT_VALID, ops.FTLE_OK, ops.FTLE_ENDED, ops.FTLE_NONFINITE, ops.FTLE_COLLAPSED) == (0, 1, 2, 3, 4)
    assert ops.FTLE_K == 9 and len(ops.FTLE_CLASSES) == 5
    n = 128 ** 3
    b, f = ops.ftle_cost((128, 128, 128))
    assert b == n * (4 * 3 + 1 + 5) and f > 0
    assert ops.ftle_cost((128, 128, 128), with_cg=True)[0] == b + n * 2 * 3 * 4
    assert ops.ftle_cost((64, 32), with_cg=True)[0] == 64 * 32 * (4 * 2 + 1 + 5 + 2 * 2 * 3)
    for bad in ((5,), (5, 1), (1, 4, 4), (2048, 2048, 1024)):
        with pytest.raises(ValueError):
            ops.ftle_cost(bad)
    for shape, refine in (((3, 4), 1), ((3, 4), 2), ((2, 3, 4), 3)):
        s, lattice, h = ops.lattice_seeds(shape, refine, "cpu")
        want, wl, wh = ref.lattice_seeds(shape, refine)
        assert lattice == wl and h == wh and s.dtype == torch.float32
        np.testing.assert_array_equal(s.numpy(), want)
    s, lattice, h = ops.lattice_seeds((2, 3), 2, "cpu")
    assert lattice == (3, 5) and h == 0.5 and s[:, 1].tolist() == [0.5, 0.0] and s[:, 5].tolist() == [0.0, 0.5]
    assert torch.equal(ops.lattice_seeds((3, 4), 1, "cpu")[0], ops.grid_seeds((3, 4), 1, 0, "cpu"))
    for bad in (((5,), 1), ((5, 1), 1), ((5, 5), 0)):
        with pytest.raises(ValueError):
            ops.lattice_seeds(*bad, device="cpu")
    pos, st = torch.zeros(2, 12), torch.zeros(12, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.ftle(pos, st, (3, 4), 1.0, 1.0)
    for kw in (dict(lattice=(12,)), dict(lattice=(1, 12)), dict(spacing=0.0), dict(spacing=(1.0, 1.0, 1.0)),
               dict(spacing=float("nan")), dict(T=0.0), dict(T=float("inf"))):
        a = dict(lattice=(3, 4), spacing=1.0, T=1.0)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.ftle(pos, st, **a)
    st9 = ops.ftle_stats(torch.tensor([1, 4, 2, 0, 0, 2.0, 3.0, -1.0, 2.0], dtype=torch.float64))
    assert st9["counts"] == {"not_valid": 1, "ok": 4, "ended": 2, "nonfinite": 0, "collapsed": 0}
    assert st9["mean"] == 0.5 and st9["std"] == math.sqrt(0.5) and (st9["min"], st9["max"]) == (-1.0, 2.0)
    assert math.isnan(ops.ftle_stats(torch.tensor([0, 0, 3, 0, 0, 0, 0, math.inf, -math.inf], dtype=torch.float64))["mean"])
    # windows: every `every`-th step that still closes
    assert drv.window_starts(5, 3, 1) == [0, 1, 2] and drv.window_starts(5, 3, 2) == [0, 2]
    assert drv.window_starts(5, 5, 1) == [0] and drv.window_starts(2, 3, 1) == []
    with pytest.raises(ValueError):
        drv.window_starts(5, 0, 1)
    ap = drv._args(3, "x", "rife")
    ok = drv.check_args(ap.parse_args(["--flows", "f.npy", "--window", "3"]))
    assert (ok.every, ok.refine, ok.dt, ok.accept_out, ok.method, ok.direction, ok.gap) == (1, 1, 1.0, False, "euler", "fwd", 2)
    assert drv._args(2, "x", "upflow").parse_args(["--dataset", "rectangle2d", "--window", "2"]).gap == 1
    for argv in (["--window", "3"], ["--dataset", "droplet3d", "--seq", "s.npy", "--window", "3"],
                 ["--flows", "f.npy", "--window", "0"], ["--flows", "f.npy", "--window", "2", "--every", "0"],
                 ["--flows", "f.npy", "--window", "2", "--refine", "0"], ["--flows", "f.npy", "--window", "2", "--dt", "0"],
                 ["--flows", "f.npy", "--window", "2", "--start", "-1"]):
        with pytest.raises(SystemExit):
            drv.check_args(ap.parse_args(argv))
    with pytest.raises(SystemExit):
        ap.parse_args(["--flows", "f.npy"])  # no window


def test_kernel_refuses_bad_arguments_before_any_launch():
    """Argument validation happens before the launch: testable without a GPU, with dummy non-NULL device pointers."""
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    d3 = lambda *v: (ctypes.c_double * 3)(*v)
    one, half = d3(1.0, 1.0, 1.0), d3(0.5, 0.5, 0.5)
    f3 = lambda m=16, mcs=64, st=16, valid=None, C=3, D=4, H=4, W=4, ih=one, i2h=half, iT=1.0, acc=0, e=16, cls=16, \
        cg=None, ws=None, out=None: L.fs_ftle3d(m, mcs, st, valid, C, D, H, W, ih, i2h, iT, acc, e, cls, cg, ws, out, None)
    f2 = lambda m=16, mcs=16, st=16, valid=None, C=2, H=4, W=4, ih=one, i2h=half, iT=1.0, acc=0, e=16, cls=16, cg=None, \
        ws=None, out=None: L.fs_ftle2d(m, mcs, st, valid, C, H, W, ih, i2h, iT, acc, e, cls, cg, ws, out, None)
    for fn in (f2, f3):
        for ptr in ("m", "st", "ih", "i2h", "e", "cls"):
            assert fn(**{ptr: None}) == 1, ptr                                        # FS_ERR_NULLPTR
        assert fn(out=16) == 1                                                        # a summary needs its workspace
        for kw in (dict(H=1), dict(W=1), dict(H=0), dict(C=4), dict(C=1), dict(mcs=15)):
            assert fn(**kw) == 2, kw                                                  # FS_ERR_SHAPE
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(iT=bad) == 3, bad                                               # FS_ERR_ARG
            assert fn(ih=d3(1.0, bad, 1.0)) == 3 and fn(i2h=d3(bad, 0.5, 0.5)) == 3, bad
    assert f3(D=1) == 2 and f3(C=2) == 2 and f2(C=3) == 2 and f3(D=2048, H=2048, W=1024, mcs=1 << 40) == 2
    assert L.fs_ftle2d_ws_bytes(2, 4, 4) == 9 * 8 and L.fs_ftle3d_ws_bytes(3, 64, 64, 64) == 1024 * 9 * 8
    assert L.fs_ftle3d_ws_bytes(3, 256, 256, 256) == 2048 * 9 * 8
    assert L.fs_ftle2d_ws_bytes(3, 4, 4) == -2 and L.fs_ftle3d_ws_bytes(3, 1, 4, 4) == -2
