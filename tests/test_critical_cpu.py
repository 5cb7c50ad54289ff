"""CPU: the numpy restatement of ops.critical_points (tests/critical_ref.py) against things it does not compute itself
-- planted linear fields and numpy.linalg.eigvals, the winding number of a 2-D field along its boundary --, its edge
cases, the C-ABI's argument checks (returned before any launch), ops' host-side checks, and the linking of steps."""
import ctypes

import numpy as np
import pytest
import torch

import critical_ref as R


def _kind(i):
    """Where seed i plants its zero: a fifth of the seeds near a diagonal face of the split (i % 5 == 1), five eighths of
    the others -- half of all -- near an axis face, the rest anywhere."""
    if i % 5 == 1:
        return "diagonal"
    j = i - (i + 3) // 5  # the rank of i among the seeds that are not diagonal ones
    return "axis" if j % 8 < 5 else "free"


def _planted(rng, sp, i):
    """(u [C, *sp] fp32, p (x, y(, z)), A) of the linear field A (x - p): p strictly inside the node range, by _kind(i)
    1e-7 .. 1e-12 from an axis face of the split or as near to a diagonal face."""
    nd = len(sp)
    ext = np.array(sp[::-1], dtype=np.float64)  # (x, y, z)
    A = rng.standard_normal((nd, nd))
    p = 0.5 + rng.random(nd) * (ext - 2.0)
    eps = 10.0 ** -rng.uniform(7, 12) * rng.choice((-1.0, 1.0))
    kind = _kind(i)
    if kind == "axis":
        a = rng.integers(nd)
        p[a] = np.clip(np.rint(p[a]), 1, ext[a] - 2) + eps
    elif kind == "diagonal":
        a, b = rng.choice(nd, 2, replace=False)
        p[b] = np.floor(p[b]) + (p[a] - np.floor(p[a])) + eps  # the fractions of two coordinates nearly agree
    grid = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sp], indexing="ij")[::-1]  # x, y(, z) as [*sp]
    d = np.stack([g - p[a] for a, g in enumerate(grid)])
    return np.einsum("rc,c...->r...", A, d).astype(np.float32), p, A


@pytest.mark.parametrize("sp", [(4, 5, 6), (7, 9)])
def test_planted_linear_fields_give_one_point_of_the_right_class(sp):
    nd = len(sp)
    n = 240
    worst = 0.0
    near = {"axis": 0, "diagonal": 0, "free": 0}
    for i in range(n):
        rng = np.random.default_rng(1000 * nd + i)
        u, p, A = _planted(rng, sp, i)
        # what was realised, read off p itself: the distance to the nearest axis face and to the nearest diagonal face
        frac = p - np.floor(p)
        d_axis = np.minimum(frac, 1.0 - frac).min()
        d_diag = min(abs(frac[a] - frac[b]) for a in range(nd) for b in range(a))
        kind = "axis" if d_axis < 2e-7 else "diagonal" if d_diag < 2e-7 else "free"
        assert kind == _kind(i), (i, kind, d_axis, d_diag)
        near[kind] += 1
        r = R.critical_points(u[None])
        assert r["counts"][0, 0] == 1 and len(r["cell"]) == 1, (i, r["counts"])
        # the node values are fp32: relative errors of 6e-8 in a field of size O(10) move the zero by O(1e-6)
        err = float(np.abs(r["pos"][0].astype(np.float64) - p).max())
        worst = max(worst, err)
        assert err < 1e-5, (i, err)
        n_pos, spiral = R.class_from_eigenvalues(A)
        assert int(r["cls"][0]) == (n_pos | (R.CP_SPIRAL if spiral else 0)), (i, r["cls"], n_pos, spiral)
    assert n >= 200 and 2 * near["axis"] >= n and 5 * near["diagonal"] >= n, near  # half and a fifth of the seeds
    print("planted %s: %r, worst position error %.2e" % (sp, near, worst))


@pytest.mark.parametrize("nd", [2, 3])
def test_class_rule_agrees_with_eigvals(nd):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((20000, nd, nd))
    w = np.linalg.eigvals(A)
    near = np.abs(w.real).min(1) < 1e-6 * np.abs(w).max(1)
    assert near.sum() <= 200  # at most 1 % may be excluded
    cls = R.classify(R.invariants(A, nd), nd)
    want = (w.real > 0).sum(1) | np.where((w.imag != 0).any(1), R.CP_SPIRAL, 0)
    bad = np.nonzero((cls != want) & ~near)[0]
    assert len(bad) == 0, (bad[:5], cls[bad[:5]], want[bad[:5]])
    print("excluded %d of %d" % (int(near.sum()), len(A)))


def _band_limited(rng, shape):
    """A smooth random field: a few low Fourier modes with random phases."""
    C = len(shape)
    grid = np.meshgrid(*[np.arange(s) / s for s in shape], indexing="ij")
    u = np.zeros((C,) + tuple(shape))
    for r in range(C):
        for _ in range(6):
            k = rng.integers(-2, 3, size=C)
            ph = rng.uniform(0, 2 * np.pi)
            u[r] += rng.standard_normal() * np.cos(2 * np.pi * sum(ki * g for ki, g in zip(k, grid)) + ph)
    return u.astype(np.float32)


def test_index_sum_is_the_boundary_winding_number():
    rng = np.random.default_rng(1)
    done = 0
    for i in range(20):
        u = rng.standard_normal((2, 9, 11)).astype(np.float32) if i % 2 == 0 else _band_limited(rng, (9, 11))
        r = R.critical_points(u[None])
        assert r["counts"][0, 1] == 0  # (a seed with a degenerate simplex would prove nothing)
        idx = int(np.sign(r["inv"][:, 1]).sum())
        wn = R.winding_number(u)
        assert abs(wn - round(wn)) < 1e-9 and idx == round(wn), (i, idx, wn)
        done += 1
    assert done == 20


def test_a_node_exactly_at_a_zero_is_degenerate():
    z, y, x = np.meshgrid(np.arange(4.0), np.arange(5.0), np.arange(6.0), indexing="ij")
    u = np.stack([x - 2.0, y - 2.0, z - 1.0]).astype(np.float32)  # zero at the node (1, 2, 2)
    r = R.critical_points(u[None])
    assert r["counts"][0, 1] > 0 and (r["mask"] & R.MASK_DEGENERATE).any()
    y, x = np.meshgrid(np.arange(7.0), np.arange(9.0), indexing="ij")
    r = R.critical_points(np.stack([x - 3.0, y - 2.0]).astype(np.float32)[None])
    assert r["counts"][0, 1] > 0 and r["counts"][0, 0] == 0


def test_all_zero_field_is_quiet():
    for sp in ((3, 4, 5), (4, 5)):
        r = R.critical_points(np.zeros((2, len(sp)) + sp, np.float32))
        assert not r["counts"].any() and not r["mask"].any() and len(r["cell"]) == 0 and list(r["offsets"]) == [0, 0, 0]


def test_vmin_silences_slow_simplices():
    rng = np.random.default_rng(5)
    u = rng.standard_normal((1, 3, 5, 6, 7)).astype(np.float32)
    a = R.critical_points(u)
    assert a["counts"][0, 0] > 0
    slow = float(a["vmax"].min())
    b = R.critical_points(u, vmin=slow * 1.0001)
    assert 0 < a["counts"][0, 0] - b["counts"][0, 0] and (b["vmax"] > slow).all()
    assert R.critical_points(u, vmin=1e3)["counts"][0, 0] == 0


@pytest.mark.parametrize("sp", [(4, 5, 6), (6, 7)])
def test_nonfinite_nodes_silence_exactly_their_cells(sp):
    nd = len(sp)
    rng = np.random.default_rng(9)
    u = rng.standard_normal((1, nd) + sp).astype(np.float32)
    clean = R.critical_points(u)
    bad = u.copy()
    node = tuple(s // 2 for s in sp)
    bad[(0, 1) + node] = np.nan
    far = tuple(0 for _ in sp)
    bad[(0, 0) + far] = -np.inf
    r = R.critical_points(bad)
    touched = np.zeros(sp, dtype=bool)
    for n in (node, far):
        touched[tuple(slice(max(0, c - 1), c + 1) for c in n)] = True
    cells = tuple(slice(0, s - 1) for s in sp)
    nf = (r["mask"][0] & R.MASK_NONFINITE) != 0
    assert np.array_equal(nf[cells], touched[cells]) and not nf[cells].all()
    assert r["counts"][0, 2] == touched[cells].sum()
    assert (r["mask"][0][nf] == R.MASK_NONFINITE).all()
    # every other cell is what it was
    assert np.array_equal(r["mask"][0][~touched], clean["mask"][0][~touched])
    keep = ~touched.reshape(-1)[clean["cell"]]
    for c in ("cell", "simplex", "pos", "jac", "cls"):
        assert np.array_equal(clean[c][keep], r[c]), c


def test_spacing_and_scale_scale_the_jacobian_only():
    rng = np.random.default_rng(3)
    u = rng.standard_normal((2, 3, 4, 5, 6)).astype(np.float32)
    a = R.critical_points(u)
    hs, ss = (2.0, 0.5, 4.0), (0.25, 8.0)  # powers of two: exact
    b = R.critical_points(u, spacing=hs, scale=ss)
    assert len(a["cell"]) > 4 and np.array_equal(a["cell"], b["cell"]) and np.array_equal(a["simplex"], b["simplex"])
    h_xyz = np.array(hs[::-1])
    assert np.array_equal(b["pos"], (a["pos"].astype(np.float64) * h_xyz).astype(np.float32))  # index space unchanged
    sc = np.array(ss)[a["step"]]
    assert np.array_equal(b["jac"], (a["jac"].reshape(-1, 3, 3) / h_xyz * sc[:, None, None]).reshape(-1, 9))
    assert np.array_equal(b["vmax"], (a["vmax"].astype(np.float64) * sc).astype(np.float32))


def test_points_are_ordered_by_step_cell_and_simplex():
    rng = np.random.default_rng(11)
    u = rng.standard_normal((3, 3, 5, 6, 7)).astype(np.float32)
    r = R.critical_points(u)
    key = (r["step"] * 1000 + r["cell"].astype(np.int64)) * 8 + r["simplex"]
    assert len(key) > 20 and (np.diff(key) > 0).all()
    assert np.array_equal(r["offsets"], np.searchsorted(r["step"], np.arange(4)))
    # a step's table does not depend on its neighbours in the stack
    one = R.critical_points(u[1:2])
    a, b = r["offsets"][1:3]
    for c in ("cell", "simplex", "pos", "jac", "inv", "cls", "vmax"):
        assert np.array_equal(one[c], r[c][a:b]), c


def test_class_names():
    from opticalflowscivis_amd import ops
    assert ops.critical_class_names([0, 1, 2, 4, 6, 8, 18], 2) == ["sink", "saddle", "source", "focus_sink", "focus_source",
                                                                   "degenerate", "center"]
    assert ops.critical_class_names(np.array([0, 1, 2, 3, 5, 7, 12], np.uint8), 3) == [
        "sink", "saddle1", "saddle2", "source", "spiral_saddle1", "spiral_source", "degenerate"]
    assert set(ops.critical_class_names(list(range(3)) + [4, 6, 8, 16], 2)) <= set(ops.critical_class_list(2))
    with pytest.raises(ValueError):
        ops.critical_class_names([3], 2)
    assert (ops.CP_SPIRAL, ops.CP_DEGENERATE, ops.CP_MARGINAL) == (R.CP_SPIRAL, R.CP_DEGENERATE, R.CP_MARGINAL)
    assert (ops.CP_MASK_DEGENERATE, ops.CP_MASK_NONFINITE) == (R.MASK_DEGENERATE, R.MASK_NONFINITE)


def test_c_abi_errors_without_gpu():
    """Every argument error is returned before anything is launched, so it is testable on the CPU."""
    from opticalflowscivis_amd import _lib
    lib = _lib.lib()
    P = 8 * 8 * 8
    assert lib.fs_critical3d_ws_bytes(2, 8, 8, 8) == 2 * 2 * 64 * 4 + 2 * P
    assert lib.fs_critical2d_ws_bytes(3, 5, 7) == 128 + 3 * 35  # 3 * 5 * 8 = 120 bytes of counts, padded to 16
    assert lib.fs_critical3d_ws_bytes(1, 1, 8, 8) == -2 and lib.fs_critical3d_ws_bytes(0, 8, 8, 8) == -2
    assert lib.fs_critical2d_ws_bytes(1, 8, 1) == -2
    assert lib.fs_critical3d_ws_bytes(1, 2048, 2048, 512) == -2  # 2^31 nodes
    assert lib.fs_critical2d_ws_bytes(1, 1 << 15, (1 << 16) - 1) != -2 and lib.fs_critical2d_ws_bytes(1, 1 << 15, 1 << 16) == -2
    # count: flows, K, C, (D,) H, W, sstride, vmin, ws, stream
    assert lib.fs_critical_count3d(None, 1, 3, 8, 8, 8, 3 * P, 0.0, 16, None) == 1
    assert lib.fs_critical_count3d(16, 1, 3, 8, 8, 8, 3 * P, 0.0, None, None) == 1
    assert lib.fs_critical_count3d(16, 1, 2, 8, 8, 8, 3 * P, 0.0, 16, None) == 2      # C
    assert lib.fs_critical_count2d(16, 1, 3, 8, 8, 3 * 64, 0.0, 16, None) == 2
    assert lib.fs_critical_count3d(16, 1, 3, 8, 1, 8, 3 * P, 0.0, 16, None) == 2      # an extent below 2
    assert lib.fs_critical_count3d(16, 2, 3, 8, 8, 8, 3 * P - 1, 0.0, 16, None) == 2  # sstride too small
    assert lib.fs_critical_count3d(16, 0, 3, 8, 8, 8, 3 * P, 0.0, 16, None) == 2      # K
    for bad in (-1.0, float("nan"), float("inf"), 1e300):
        assert lib.fs_critical_count3d(16, 1, 3, 8, 8, 8, 3 * P, bad, 16, None) == 3, bad
        assert lib.fs_critical_count2d(16, 1, 2, 8, 8, 2 * 64, bad, 16, None) == 3, bad
    assert lib.fs_critical_count3d(16, 1, 3, 8, 8, 8, 3 * P, 0.0, 24, None) == 3      # ws not 16-byte aligned
    h = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    sc = (ctypes.c_double * 2)(1.0, 2.0)
    names = ("flows", "K", "C", "D", "H", "W", "sstride", "inv_h", "scale", "vmin", "ws", "row_offsets", "N", "cell",
             "simplex", "pos", "jac", "inv", "cls", "vmax", "status", "stream")
    ok = [16, 2, 3, 8, 8, 8, 3 * P, h, sc, 0.0, 16, 16, 10, 16, 16, 16, 16, 16, 16, 16, 16, None]

    def emit(nd=3, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        if nd == 2:
            a[names.index("C")] = kw.get("C", 2)
            del a[names.index("D")]
            return lib.fs_critical_emit2d(*a)
        return lib.fs_critical_emit3d(*a)

    for nd in (2, 3):
        for name in ("flows", "inv_h", "scale", "ws", "row_offsets", "status", "cell", "simplex", "pos", "jac", "inv", "cls",
                     "vmax"):
            assert emit(nd, **{name: None}) == 1, name
        assert emit(nd, W=1) == 2 and emit(nd, sstride=2 * 64 - 1) == 2 and emit(nd, K=0) == 2 and emit(nd, C=4) == 2
        assert emit(nd, vmin=-0.5) == 3 and emit(nd, N=-1) == 3 and emit(nd, ws=20) == 3
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert emit(nd, inv_h=(ctypes.c_double * 3)(1.0, bad, 1.0)) == 3, bad
            assert emit(nd, scale=(ctypes.c_double * 2)(1.0, bad)) == 3, bad
        # nothing to write: FS_OK with nothing launched, the outputs may be absent
        assert emit(nd, N=0, cell=None, simplex=None, pos=None, jac=None, inv=None, cls=None, vmax=None) == 0


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from opticalflowscivis_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.critical_points(torch.rand(1, 3, 4, 4, 4))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.critical_points_count(torch.rand(1, 2, 4, 4))
    for bad in (-1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="vmin"):
            ops.critical_points(torch.rand(1, 2, 4, 4), vmin=bad)
    with pytest.raises(ValueError):
        ops.critical_points_cost((8, 8, 1))
    with pytest.raises(ValueError):
        ops.critical_points_cost((8, 8), op="both")
    with pytest.raises(ValueError):
        ops.critical_points_cost((8, 8), K=0)
    assert ops.critical_points_cost((8, 8, 8), 2, op="count") == (2 * (13 * 512 + 8 * 64), 0)
    assert ops.critical_points_cost((4, 8), 1, N=10, op="emit") == (32 + 10 * (4 + 1 + 8 + 32 + 32 + 1 + 4), 2000)
    assert ops.critical_points_cost((8, 8, 8), 1, N=1, op="emit")[0] == 512 + 4 + 1 + 12 + 72 + 32 + 1 + 4


def _table(pos, cls):
    return {"pos": np.asarray(pos, dtype=np.float32), "cls": np.asarray(cls, dtype=np.uint8)}


def test_link_points_by_hand():
    from opticalflowscivis_amd import critical
    # step 0: a sink at 0, a saddle at 10, a sink at 20.  step 1: two sinks equally far from the first (a tie: the lower
    # row wins), a SOURCE right on the saddle (class mismatch inside the radius), nothing near 20 (a death), and a new
    # sink far away (a birth)
    t0 = _table([[0, 0], [10, 0], [20, 0]], [0, 1, 0])
    t1 = _table([[1, 0], [-1, 0], [10, 0.25], [40, 0]], [0, 4, 2, 0])  # row 1: a focus sink: n_pos 0 as well
    track, births, deaths = critical.link_points([t0, t1], 2.0)
    assert list(track[0]) == [0, 1, 2] and list(track[1]) == [0, 3, 4, 5]
    assert births == [3, 3] and deaths == [2, 0]
    # the tie the other way round: two old points equally far from one new one
    track, births, deaths = critical.link_points([_table([[1, 0], [-1, 0]], [0, 0]), _table([[0, 0]], [0])], 2.0)
    assert list(track[0]) == [0, 1] and list(track[1]) == [0] and births == [2, 0] and deaths == [1, 0]
    # just outside the radius; on it
    far = critical.link_points([_table([[0, 0, 0]], [1]), _table([[0, 3, 4.001]], [1])], 5.0)
    on = critical.link_points([_table([[0, 0, 0]], [1]), _table([[0, 3, 4]], [1])], 5.0)
    assert list(far[0][1]) == [1] and list(on[0][1]) == [0]
    # no radius, empty steps
    track, births, deaths = critical.link_points([t0, _table(np.zeros((0, 2)), []), t1], 0.0)
    assert [list(t) for t in track] == [[0, 1, 2], [], [3, 4, 5, 6]] and births == [3, 0, 4] and deaths == [3, 0, 0]
    assert critical.link_points([], 1.0) == ([], [], [])


def test_link_points_grid_matches_the_dense_search():
    from opticalflowscivis_amd import critical
    rng = np.random.default_rng(2)
    a = _table(rng.random((300, 3)) * 20, rng.integers(0, 4, 300))
    b = _table(a["pos"] + rng.normal(0, 0.4, (300, 3)), a["cls"])
    b["pos"], b["cls"] = b["pos"][::-1].copy(), b["cls"][::-1].copy()
    radius = 1.0
    track, births, deaths = critical.link_points([a, b], radius)
    pa, pb = a["pos"].astype(np.float64), b["pos"].astype(np.float64)
    d2 = ((pa[:, None] - pb[None]) ** 2).sum(-1)
    d2[(a["cls"][:, None] & 3) != (b["cls"][None] & 3)] = np.inf
    d2[d2 > radius * radius] = np.inf
    want = np.arange(300, 600, dtype=np.int64)
    fa, fb = d2.argmin(1), d2.argmin(0)
    new = 300
    for j in range(300):
        i = fb[j]
        if np.isfinite(d2[i, j]) and fa[i] == j:
            want[j] = i
        else:
            want[j] = new
            new += 1
    assert np.array_equal(track[1], want) and births[1] == new - 300 and deaths[0] == births[1]
    assert 10 < births[1] < 290  # (both outcomes occur)


def test_link_points_at_the_radius_itself():
    """Pairs whose distance equals the radius up to rounding: the bins must not hide a link that `<= radius` allows."""
    from opticalflowscivis_amd import critical
    radius = 0.1
    k = np.arange(0, 400, 2, dtype=np.float64)
    a = {"pos": np.stack([k * radius, np.zeros_like(k)], 1), "cls": np.zeros(len(k), np.uint8)}
    b = {"pos": np.stack([(k + 1) * radius, np.zeros_like(k)], 1), "cls": np.zeros(len(k), np.uint8)}
    d2 = ((a["pos"][:, None] - b["pos"][None]) ** 2).sum(-1)
    d2[d2 > radius * radius] = np.inf
    fa, fb = d2.argmin(1), d2.argmin(0)
    want = np.array([np.isfinite(d2[fb[j], j]) and fa[fb[j]] == j for j in range(len(k))])
    assert 20 < want.sum() < len(k)  # (rounding goes both ways)
    track, births, deaths = critical.link_points([a, b], radius)
    assert np.array_equal(track[1] < len(k), want) and births[1] == (~want).sum()


def test_parser_and_out_of_scope():
    from opticalflowscivis_amd import critical
    for nd, model in ((2, "rife"), (3, "rife"), (2, "upflow")):
        ap = critical._args(nd, "x", model)
        a = critical.check_args(ap.parse_args(["--flows", "f.npy", "--classes", "sink,saddle" if nd == 2 else "saddle1"]))
        assert a.vmin == 0.0 and a.link_radius == 2.0 and a.spacing == [1.0] and a.dt == 1.0 and hasattr(a, "png_dir") == (nd == 2)
        for bad in (["--vmin", "-1"], ["--classes", "vortex"], ["--link-radius", "nan"], ["--min-jnorm", "-2"]):
            with pytest.raises(SystemExit):
                critical.check_args(ap.parse_args(["--flows", "f.npy"] + bad))
    for word in ("separatrices", "trilinear", "simulation-of-simplicity", "periodic", "space-time", "autograd"):
        assert word in critical.__doc__, word
