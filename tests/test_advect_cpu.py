"""CPU: the fp64 restatement of the advection kernel (tests/advect_ref.py) on problems with known answers -- a constant
field, a rigid rotation (the integrators' orders of convergence), the composed ground truth of a synthetic sequence,
the border and non-finite rules -- and the pure-Python parts of the trace driver: step_chain, the chaining of a
--save-flows directory, seeds, costs and argument errors."""
import math
import os

import numpy as np
import pytest
import torch

import advect_ref as ref

METHODS = (ref.EULER, ref.RK2, ref.RK4)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("sp", [(9, 20), (6, 9, 20)])
def test_constant_field_is_exact(method, sp):
    C, K = len(sp), 5
    c = np.array([0.75, -0.5, 0.25][:C], np.float32)  # exactly representable, and so is every partial sum
    flows = np.broadcast_to(c.reshape((1, C) + (1,) * C), (K, C) + sp).astype(np.float32)
    rng = np.random.default_rng(0)
    pos = np.stack([rng.integers(4, 9, 50), rng.integers(3, 5, 50), rng.integers(0, 4, 50)][:C]).astype(np.float32)
    pos += np.float32(0.125)
    traj, st, n = ref.advect(pos, flows, method=method, substeps=4)
    assert (st == ref.ALIVE).all() and (n == K).all()
    for k in range(K):
        np.testing.assert_array_equal(traj[k], pos + np.float32(k + 1) * c[:, None])


def _rotation(S=17, omega=0.2, K=8, n=200):
    c = (S - 1) / 2.0
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    # the field's values are rounded to fp32 once, as a stored field is: multiples of omega in fp32 stay a linear
    # function of the grid index to within fp32 rounding, far below the integrators' errors measured here
    w32 = float(np.float32(omega))
    field = np.stack([-w32 * (y - c), w32 * (x - c)]).astype(np.float32)
    rng = np.random.default_rng(7)
    r = rng.uniform(0.5, 5.0, n)
    a = rng.uniform(0, 2 * math.pi, n)
    pos = np.stack([c + r * np.cos(a), c + r * np.sin(a)]).astype(np.float32)
    flows = np.broadcast_to(field, (K,) + field.shape)
    p0 = pos.astype(np.float64) - c
    th = w32 * K
    exact = np.stack([p0[0] * math.cos(th) - p0[1] * math.sin(th), p0[0] * math.sin(th) + p0[1] * math.cos(th)]) + c
    return pos, flows, exact


def _rot_err(method, S):
    pos, flows, exact = _rotation()
    traj, st, _ = ref.advect(pos, flows, method=method, substeps=S)
    assert (st == ref.ALIVE).all()
    return float(np.sqrt(((traj[-1].astype(np.float64) - exact) ** 2).sum(0)).max())


def test_rigid_rotation_orders():
    """Bilinear sampling reproduces a linear field, so the error against the exact rotation is the integrator's: it must
    shrink from 1 to 2 substeps by ~2 (Euler), ~4 (RK2), >= 10 (RK4; 16 in exact arithmetic, but RK4 at 2 substeps
    is already near the fp32 rounding of the stored positions)."""
    e = {m: (_rot_err(m, 1), _rot_err(m, 2)) for m in METHODS}
    ratio = {m: e[m][0] / e[m][1] for m in METHODS}
    print("rotation errors", e, "ratios", ratio)
    assert 1.8 <= ratio[ref.EULER] <= 2.3, ratio
    assert 3.5 <= ratio[ref.RK2] <= 4.5, ratio
    assert ratio[ref.RK4] >= 10, ratio
    assert e[ref.RK4][0] < e[ref.RK2][0] < e[ref.EULER][0]


def test_composed_ground_truth_equals_the_long_displacement():
    """Integer velocity: a voxel of the sphere stays on grid points of the sphere, so Euler through gt(t, t+1) lands
    exactly on gt(0, 5).  Outside the sphere the moving object legitimately picks up background particles: not compared."""
    from opticalflowscivis_amd.data import synthetic
    from opticalflowscivis_amd import ops
    T, S = 6, 32
    frames, gt = synthetic.droplet3d_motion(T, S, seed=3, v=(1, -2, 1))
    flows = np.stack([gt(t, t + 1)[0].numpy() for t in range(T - 1)])
    seeds = ops.grid_seeds((S, S, S), 1, 0, "cpu").numpy()
    traj, st, n = ref.advect(seeds, flows)
    inside = frames[0].numpy().reshape(-1) > 0
    assert inside.sum() >= 100
    long_disp = gt(0, T - 1)[0].numpy().reshape(3, -1)
    assert np.abs(long_disp[:, inside]).max() == 10.0  # 5 steps of -2 along y
    np.testing.assert_array_equal((traj[-1] - seeds)[:, inside], long_disp[:, inside])
    assert (st[inside] == ref.ALIVE).all() and (n[inside] == T - 1).all()


def test_border_and_nonfinite_rules():
    sp = (4, 5)  # H, W
    zero = np.zeros((2, 2) + sp, np.float32)
    # x = W - 1 and y = H - 1: the border is inside; -0.5: OUT without moving; NaN seed: NONFINITE without moving
    pos = np.array([[4.0, -0.5, np.nan, 1.0], [3.0, 1.0, 1.0, 1.0]], np.float32)
    traj, st, n = ref.advect(pos, zero)
    assert st.tolist() == [ref.ALIVE, ref.OUT, ref.NONFINITE, ref.ALIVE] and n.tolist() == [2, 0, 0, 2]
    for k in range(2):
        np.testing.assert_array_equal(traj[k].view(np.uint32), pos.view(np.uint32))
    # a NaN corner of weight 0: the particle sits exactly on (x=1, y=1); its (x=2, y=1) neighbour is NaN
    f = zero.copy()
    f[0, 0, 1, 2] = np.nan
    p = np.array([[1.0, 3.0], [1.0, 3.0]], np.float32)
    traj, st, n = ref.advect(p, f)
    assert st.tolist() == [ref.NONFINITE, ref.ALIVE] and n.tolist() == [0, 2]
    np.testing.assert_array_equal(traj[:, :, 0], np.ones((2, 2), np.float32))  # it keeps its last finite position
    # an infinite flow: NONFINITE (p + inf is not finite), never OUT
    f = zero.copy()
    f[0, 1] = np.inf
    traj, st, n = ref.advect(np.array([[1.25], [1.5]], np.float32), f)
    assert st.tolist() == [ref.NONFINITE] and traj[1, :, 0].tolist() == [1.25, 1.5]
    # leaving the box: the exit point is kept, later fields are not applied, an ended particle's status passes through
    f = np.zeros((3, 2) + sp, np.float32)
    f[:, 0] = 2.5
    traj, st, n = ref.advect(np.array([[1.0], [1.0]], np.float32), f)
    assert st.tolist() == [ref.OUT] and n.tolist() == [1] and traj[:, 0, 0].tolist() == [3.5, 6.0, 6.0]
    traj, st, n = ref.advect(np.array([[1.0], [1.0]], np.float32), f, status=np.array([ref.OUT], np.uint8),
                             steps=np.array([7], np.int32))
    assert st.tolist() == [ref.OUT] and n.tolist() == [7] and (traj == 1.0).all()
    # substeps: the exit is found at the substep where it happens (1 -> 2.5 -> 4.0, on the border -> 5.5)
    f[:, 0] = 6.0
    traj, st, n = ref.advect(np.array([[1.0], [1.0]], np.float32), f[:1], substeps=4)
    assert st.tolist() == [ref.OUT] and n.tolist() == [0] and traj[0, 0, 0] == 5.5
    # stage points are clamped by the sampling, never classified: the midpoint 0 + 0.5 * 10 = 5 lies outside x <= 4,
    # is sampled at x = 4, where the flow is 1, and the end point 0 + 1 is inside
    f1 = np.ones((1, 2) + sp, np.float32)
    f1[0, 1] = 0.0
    f1[0, 0, :, 0] = 10.0
    traj, st, _ = ref.advect(np.array([[0.0], [1.0]], np.float32), f1, method=ref.RK2)
    assert st.tolist() == [ref.ALIVE] and traj[0, :, 0].tolist() == [1.0, 1.0]
    traj, st, _ = ref.advect(np.array([[0.0], [1.0]], np.float32), f1, method=ref.EULER)
    assert st.tolist() == [ref.OUT] and traj[0, :, 0].tolist() == [10.0, 1.0]


def test_k_steps_equal_k_single_steps():
    rng = np.random.default_rng(3)
    sp = (5, 6, 7)
    flows = (0.6 * rng.standard_normal((3, 3) + sp)).astype(np.float32)
    pos = (rng.random((3, 40)) * np.array(sp[::-1])[:, None]).astype(np.float32)
    for m, S in ((ref.EULER, 1), (ref.RK2, 2), (ref.RK4, 3)):
        traj, st, n = ref.advect(pos, flows, method=m, substeps=S)
        p, s1, n1 = pos, None, None
        for k in range(3):
            t1, s1, n1 = ref.advect(p, flows[k:k + 1], s1, n1, m, S)
            np.testing.assert_array_equal(t1[0].view(np.uint32), traj[k].view(np.uint32))
            p = t1[0]
        assert (s1 == st).all() and (n1 == n).all()


def test_step_chain():
    from opticalflowscivis_amd.stepflows import step_chain
    assert step_chain(7, 2, "fwd") == [(1, 2, 1), (2, 3, 3), (3, 4, 5), (4, 5, 7)]
    assert step_chain(7, 2, "bwd") == [(5, 4, 8), (4, 3, 6), (3, 2, 4), (2, 1, 2)]
    assert step_chain(9, 4, "fwd") == [(2, 4, 1), (4, 6, 5)]
    assert step_chain(9, 4, "bwd") == [(6, 4, 8), (4, 2, 4)]
    assert step_chain(4, 2, "fwd") == [(1, 2, 1)]
    assert step_chain(4, 2, "bwd") == [(2, 1, 2)]
    assert step_chain(3, 2, "fwd") == [] and step_chain(3, 2, "bwd") == []
    assert step_chain(4, 1, "fwd", "upflow") == [(0, 1, 0), (1, 2, 2), (2, 3, 4)]
    assert step_chain(4, 1, "bwd", "upflow") == [(3, 2, 5), (2, 1, 3), (1, 0, 1)]
    assert step_chain(6, 2, "fwd", "upflow") == [(0, 2, 0), (2, 4, 4)]
    assert step_chain(1, 1, "fwd", "upflow") == []
    for bad in ((7, 3, "fwd", "rife"), (7, 2, "up", "rife"), (7, 0, "fwd", "upflow"), (7, 2, "fwd", "pwc")):
        with pytest.raises(ValueError):
            step_chain(*bad)
    # the chain's flows are the consistency pairs' (the RIFE flow m -> m+h lives on frame m's grid)
    from opticalflowscivis_amd.flow_eval import rife_consistency_pairs
    cp = {(a, b): (i, j) for a, b, i, j in rife_consistency_pairs(9, 2)}
    for a, b, i in step_chain(9, 2, "fwd"):
        assert cp[(a, b)][0] == i
    for a, b, i in step_chain(9, 2, "bwd"):
        assert cp[(b, a)][1] == i


def test_flow_directory_chaining(tmp_path):
    from opticalflowscivis_amd.stepflows import chain_flow_files
    d = str(tmp_path)
    # what evaluate_flow --save-flows writes for a RIFE model at gap 2: mid -> t0 and mid -> t1 of every pair
    for a, b in ((1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (3, 4), (3, 6)):
        np.save(os.path.join(d, "flow_%03d_to_%03d.npy" % (a, b)), np.zeros((2, 3, 3), np.float32))
    open(os.path.join(d, "class_001_to_002.npy"), "w").close()
    names = lambda c: [(a, b, os.path.basename(p)) for a, b, p in c]
    assert names(chain_flow_files(d, 1, "fwd")) == [(1, 2, "flow_001_to_002.npy"), (2, 3, "flow_002_to_003.npy"),
                                                    (3, 4, "flow_003_to_004.npy")]  # the nearest later frame
    assert names(chain_flow_files(d, 3, "bwd")) == [(3, 2, "flow_003_to_002.npy"), (2, 1, "flow_002_to_001.npy"),
                                                    (1, 0, "flow_001_to_000.npy")]
    assert chain_flow_files(d, 0, "fwd") == [] and chain_flow_files(d, 0, "bwd") == []
    with pytest.raises(ValueError):
        chain_flow_files(d, 0, "sideways")


def test_argument_errors():
    from opticalflowscivis_amd import trace
    ap = trace._args(3, "x", "rife")
    ok = trace.check_args(ap.parse_args(["--dataset", "droplet3d", "--seed-grid", "1", "--map-out", "m.npy"]))
    assert ok.gap == 2 and ok.chunk == 4 and ok.method == "euler" and ok.direction == "fwd"
    assert trace._args(2, "x", "upflow").parse_args(["--seq", "s.npy", "--seed-grid", "2"]).gap == 1
    for argv in (["--seed-grid", "2"],                                                   # no source
                 ["--dataset", "droplet3d", "--seq", "s.npy", "--seed-grid", "2"],        # two series
                 ["--dataset", "droplet3d", "--gt", "v.npy", "--seed-grid", "2"],         # a dataset has its own motion
                 ["--dataset", "droplet3d", "--seed-grid", "2", "--map-out", "m.npy"],    # the map needs every element
                 ["--dataset", "droplet3d", "--seeds", "s.npy", "--map-out", "m.npy"],
                 ["--dataset", "droplet3d", "--seed-grid", "0"],
                 ["--dataset", "droplet3d", "--seed-grid", "2", "--substeps", "0"],
                 ["--dataset", "droplet3d", "--seed-grid", "2", "--chunk", "0"],
                 ["--flows", "f.npy", "--seed-grid", "2", "--start", "-1"]):
        with pytest.raises(SystemExit):
            trace.check_args(ap.parse_args(argv))
    for argv in (["--dataset", "droplet3d"],                                              # no seeds
                 ["--dataset", "droplet3d", "--seeds", "s.npy", "--seed-grid", "2"],
                 ["--dataset", "droplet3d", "--seed-grid", "2", "--method", "rk3"],
                 ["--dataset", "rectangle2d", "--seed-grid", "2"]):                      # a 2-D dataset for a 3-D model
        with pytest.raises(SystemExit):
            ap.parse_args(argv)


def test_grid_seeds_costs_and_operand_errors():
    from opticalflowscivis_amd import ops
    s = ops.grid_seeds((2, 3, 4), 1, 0, "cpu")
    assert s.shape == (3, 24) and s.dtype == torch.float32
    assert s[:, 0].tolist() == [0, 0, 0] and s[:, 1].tolist() == [1, 0, 0] and s[:, 4].tolist() == [0, 1, 0]
    assert s[:, 23].tolist() == [3, 2, 1]  # (x, y, z): x runs along W, fastest
    v = s.view(3, 2, 3, 4)
    assert v[0, 1, 2, 3] == 3 and v[1, 1, 2, 3] == 2 and v[2, 1, 2, 3] == 1
    s = ops.grid_seeds((5, 7), 3, 1, "cpu")
    assert s.shape == (2, 4) and s.tolist() == [[1, 4, 1, 4], [1, 1, 4, 4]]
    for bad in (((5,), 1, 0), ((5, 0), 1, 0), ((5, 5), 0, 0), ((5, 5), 1, -1)):
        with pytest.raises(ValueError):
            ops.grid_seeds(*bad, device="cpu")
    b1, f1 = ops.advect_cost((32, 32, 32), 32 ** 3, 4, "euler", 1)
    b4, f4 = ops.advect_cost((32, 32, 32), 32 ** 3, 4, "rk4", 1)
    assert b1 == b4 == 4 * (4 * 3 * 32 ** 3) + 4 * 3 * 32 ** 3 * 2 + 10 * 32 ** 3 and 3.5 * f1 < f4 < 4.5 * f1
    assert ops.advect_cost((32, 32, 32), 10, 4, "euler", 1)[0] == 4 * 10 * 4 * 24 + 4 * 3 * 10 * 2 + 100  # sparse: the gathers
    assert ops.advect_cost((32, 32), 100, 4, "euler", 1, record=True)[0] > ops.advect_cost((32, 32), 100, 4, "euler", 1)[0]
    with pytest.raises(ValueError):
        ops.advect_cost((32, 32), 100, 4, "heun", 1)
    pos, flows = torch.zeros(2, 5), torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.advect(pos, flows)
    for kw in (dict(method="heun"), dict(substeps=0), dict(scale=float("nan"))):
        with pytest.raises(ValueError):
            ops.advect(pos, flows, **kw)
    with pytest.raises(ValueError):
        ops.advect(pos, torch.zeros(2, 4, 4))


def test_kernel_refuses_bad_arguments_before_any_launch():
    """Argument validation happens before the launch: testable without a GPU, with dummy non-NULL pointers."""
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    a3 = lambda flows=16, K=1, C=3, D=4, H=4, W=4, fss=192, pos=16, pcs=8, P=8, traj=16, tss=24, tcs=8, st=16, n=None, \
        m=0, S=1, scale=1.0: L.fs_advect3d(flows, K, C, D, H, W, fss, pos, pcs, P, traj, tss, tcs, st, n, m, S, scale, None)
    a2 = lambda flows=16, K=1, C=2, H=4, W=4, fss=32, pos=16, pcs=8, P=8, traj=16, tss=16, tcs=8, st=16, n=None, m=0, \
        S=1, scale=1.0: L.fs_advect2d(flows, K, C, H, W, fss, pos, pcs, P, traj, tss, tcs, st, n, m, S, scale, None)
    for fn in (a2, a3):
        for ptr in ("flows", "pos", "traj", "st"):
            assert fn(**{ptr: None}) == 1, ptr                                       # FS_ERR_NULLPTR
        for kw in (dict(K=0), dict(P=0), dict(H=0), dict(W=0), dict(C=4), dict(pcs=7), dict(tcs=7),
                   dict(K=2, fss=1), dict(K=2, tss=3)):
            assert fn(**kw) == 2, kw                                                 # FS_ERR_SHAPE
        for kw in (dict(S=0), dict(m=3), dict(m=-1), dict(scale=float("inf")), dict(scale=float("nan"))):
            assert fn(**kw) == 3, kw                                                 # FS_ERR_ARG
    assert a3(D=0) == 2 and a3(C=2) == 2 and a2(C=3) == 2
