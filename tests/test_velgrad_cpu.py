"""CPU: the fp64 restatement of the velocity-gradient kernel (tests/velgrad_ref.py) on fields with known answers -- a
linear field, rigid rotations, a pure strain, a constant field, the trace identity, 2-D incompressible fields, the
difference selection at an extent-2 axis, a planted NaN -- and what runs without a GPU of the product: costs, plane
layout, statistics, the driver's argument checks, the argument errors of ops.velgrad and of the C entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

import velgrad_ref as ref

# dyadic entries: A x + b is exact in fp32 on an integer grid, so every difference is exact and J == A bit for bit
A2 = np.array([[1.5, 0.25], [-0.5, 0.75]])
A3 = np.array([[1.25, 0.5, -0.25], [0.0, 0.75, 0.5], [-0.5, 0.25, 1.5]])


def _coords(sp):
    """[C, *sp] fp64 node coordinates, component 0 = x (the last axis)."""
    return np.indices(sp)[::-1].astype(np.float64)


def _linear(A, sp, b=None):
    x = _coords(sp)
    b = np.array([3.0, -1.5, 0.25][:len(sp)]) if b is None else b
    u = np.einsum("rc,c...->r...", A, x) + b.reshape((-1,) + (1,) * len(sp))
    u32 = u.astype(np.float32)
    assert (u32.astype(np.float64) == u).all()
    return u32[None]


@pytest.mark.parametrize("A,sp", [(A2, (4, 5)), (A3, (3, 4, 5))])
def test_linear_field_gives_its_matrix_at_every_node(A, sp):
    r = ref.velgrad(_linear(A, sp))
    C = len(sp)
    for a in range(C):
        for b in range(C):
            np.testing.assert_allclose(r["J"][0, a, b], A[a, b], rtol=1e-14)
            np.testing.assert_array_equal(r["out"][0, r["planes"]["grad"]][a * C + b], np.float32(A[a, b]))
    np.testing.assert_array_equal(r["out"][0, r["planes"]["div"]][0], np.float32(np.trace(A)))
    # spacing and scale: J = A / h_c * scale, the border (one-sided differences) included
    hs = (0.5, 2.0, 0.25)[:C]  # in the array's axis order
    r2 = ref.velgrad(_linear(A, sp), spacing=hs, scale=0.5)
    for a in range(C):
        for b in range(C):
            np.testing.assert_allclose(r2["J"][0, a, b], A[a, b] / hs[::-1][b] * 0.5, rtol=1e-14)
    assert (r["kinds"][0][..., 0] == ref.FORWARD).all() and (r["kinds"][0][..., -1] == ref.BACKWARD).all()
    assert (r["kinds"][0][..., 1:-1] == ref.CENTRAL).all() and (r["flags"] & ref.FLAG_NONFINITE == 0).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_rigid_rotation_about_each_axis(axis):
    """u = W x (x) + a translation: vort = 2 W, q = |W|^2, l2 = -|W|^2, div = 0, all exactly."""
    rate = 0.75
    Wv = np.zeros(3)
    Wv[axis] = rate
    A = np.array([[0, -Wv[2], Wv[1]], [Wv[2], 0, -Wv[0]], [-Wv[1], Wv[0], 0]])
    r = ref.velgrad(_linear(A, (4, 5, 6)))
    p, o = r["planes"], r["out"][0]
    for c in range(3):
        np.testing.assert_array_equal(o[p["vort"]][c], np.float32(2 * Wv[c]))
    np.testing.assert_array_equal(o[p["vmag"]][0], np.float32(2 * rate))
    np.testing.assert_array_equal(o[p["q"]][0], np.float32(rate * rate))
    np.testing.assert_array_equal(o[p["l2"]][0], np.float32(-rate * rate))
    assert (o[p["div"]][0] == 0).all() and (r["flags"] == ref.FLAG_Q | ref.FLAG_L2).all()


def test_rigid_rotation_in_the_plane():
    rate = 1.25
    r = ref.velgrad(_linear(np.array([[0, -rate], [rate, 0]]), (5, 6)))
    p, o = r["planes"], r["out"][0]
    np.testing.assert_array_equal(o[p["vort"]][0], np.float32(2 * rate))
    np.testing.assert_array_equal(o[p["q"]][0], np.float32(rate * rate))
    np.testing.assert_array_equal(o[p["l2"]][0], np.float32(-rate * rate))
    assert (o[p["div"]][0] == 0).all() and (r["flags"] == 3).all()


@pytest.mark.parametrize("A,sp", [(np.diag([0.5, -0.5]), (4, 5)), (np.diag([1.0, -0.25, -0.75]), (3, 4, 5)),
                                  (np.array([[0, 0.5, 0], [0.5, 0, 0], [0, 0, 0.0]]), (3, 4, 5))])
def test_pure_strain(A, sp):
    r = ref.velgrad(_linear(A, sp))
    p, o = r["planes"], r["out"][0]
    assert (o[p["q"]][0] < 0).all() and (o[p["vmag"]][0] == 0).all() and (r["flags"] == 0).all()
    assert (o[p["l2"]][0] > 0).all()  # M = S^2 has two positive eigenvalues at least (2-D: the plane's two, and 0)


@pytest.mark.parametrize("sp", [(3, 4), (2, 3, 4)])
def test_constant_field_is_all_zero(sp):
    u = np.full((2, len(sp)) + sp, 2.5, np.float32)
    r = ref.velgrad(u)
    assert (r["out"] == 0).all() and (r["flags"] == 0).all()


def _random(sp, K=1, seed=0):
    rng = np.random.default_rng([seed, len(sp)] + list(sp))
    x = _coords(sp)
    C = len(sp)
    k = rng.uniform(0.3, 1.1, size=(C, C))
    u = 1.5 * np.sin(np.einsum("rc,c...->r...", k, x) + rng.uniform(0, 6.28, size=(C,) + (1,) * C))
    return (u[None] + 0.3 * rng.normal(size=(K, C) + sp)).astype(np.float32)


@pytest.mark.parametrize("sp", [(9, 12), (5, 6, 7)])
def test_trace_identity(sp):
    """l1 + l2 + l3 = tr M = -2 q, to 1e-12 ||M||_F: the restatement's M and q hang together."""
    u = _random(sp)
    r = ref.velgrad(u)
    C = len(sp)
    J = r["J"][0]
    S, O = 0.5 * (J + J.swapaxes(0, 1)), 0.5 * (J - J.swapaxes(0, 1))
    M = np.einsum("ab...,bc...->...ac", S, S) + np.einsum("ab...,bc...->...ac", O, O)
    ev = np.linalg.eigvalsh(M)
    q64 = 0.5 * ((O * O).sum((0, 1)) - (S * S).sum((0, 1)))
    nM = np.sqrt((M * M).sum((-1, -2)))
    np.testing.assert_allclose(nM, r["normM"][0], rtol=1e-12)
    assert (np.abs(ev.sum(-1) + 2 * q64) <= 1e-12 * nM).all()
    # the restatement's own lambda2 (from its M, in the header's order) agrees with the one from this M
    lam = ev[..., 1] if C == 3 else np.sort(np.concatenate([ev, np.zeros(sp + (1,))], -1), -1)[..., 1]
    assert (np.abs(lam - r["l2_64"][0]) <= 1e-12 * nM).all()
    q32 = r["out"][0, r["planes"]["q"]][0]
    np.testing.assert_allclose(q32, q64, rtol=2e-7, atol=1e-12)


def test_incompressible_2d_fields_have_equal_criteria():
    """u = a x + f(y), v = -a y + g(x): J00 + J11 == 0 exactly, so M = -q I and q > 0 <=> l2 < 0 at every node."""
    sp = (11, 13)
    rng = np.random.default_rng(4)
    x = _coords(sp)
    f, g = rng.integers(-16, 17, size=sp[0]) / 8.0, rng.integers(-16, 17, size=sp[1]) / 8.0  # dyadic: fp32 holds u, v exactly
    u64 = np.stack([0.5 * x[0] + f[:, None], -0.5 * x[1] + g[None, :]])
    u = u64.astype(np.float32)[None]
    assert (u[0].astype(np.float64) == u64).all()
    r = ref.velgrad(u)
    assert (r["out"][0, r["planes"]["div"]][0] == 0).all()
    f = r["flags"][0]
    assert ((f & 1) == ((f >> 1) & 1)).all() and (f & 1).sum() >= 10 and (f == 0).sum() >= 10
    # a compressible one does not
    f2 = ref.velgrad(_random(sp))["flags"][0]
    assert ((f2 & 1) != ((f2 >> 1) & 1)).any()


def test_every_difference_is_one_sided_at_an_extent_2_axis():
    r = ref.velgrad(_random((2, 5, 2)))
    k = r["kinds"]
    assert set(np.unique(k[0])) == {ref.FORWARD, ref.BACKWARD} == set(np.unique(k[2]))  # x and z: extent 2
    assert (k[0][..., 0] == ref.FORWARD).all() and (k[0][..., 1] == ref.BACKWARD).all()
    assert (k[1][:, 1:-1] == ref.CENTRAL).all() and (k[1][:, 0] == ref.FORWARD).all() and (k[1][:, -1] == ref.BACKWARD).all()
    assert (r["flags"] & ref.FLAG_NONFINITE == 0).all()


@pytest.mark.parametrize("sp,at", [((7, 8), (3, 4)), ((5, 6, 7), (2, 3, 3)), ((5, 6, 7), (0, 3, 6))])
def test_a_nan_poisons_exactly_its_stencil_neighbours(sp, at):
    u = _random(sp)
    u[(0, 1) + at] = np.nan
    r = ref.velgrad(u)
    want = np.zeros(sp, bool)
    for ax in range(len(sp)):
        for d in (-1, 1):
            j = list(at)
            j[ax] += d
            if 0 <= j[ax] < sp[ax]:
                want[tuple(j)] = True
                # a border neighbour differentiates one-sidedly through itself and the far side: still poisoned
    # the node itself reads its own value only in a one-sided difference, i.e. when it lies on a border
    want[at] = any(a == 0 or a == s - 1 for a, s in zip(at, sp))
    bad = (r["flags"][0] & ref.FLAG_NONFINITE) != 0
    np.testing.assert_array_equal(bad, want)
    assert np.isnan(r["out"][0][:, bad]).all() and np.isfinite(r["out"][0][:, ~bad]).all()
    assert (r["flags"][0][bad] == ref.FLAG_NONFINITE).all()


def test_field_selection_and_plane_layout():
    u = _random((4, 5, 6), K=2)
    full = ref.velgrad(u, scale=(1.0, 0.5))
    assert full["out"].shape == (2, 16, 4, 5, 6)
    assert {n: (s.start, s.stop) for n, s in full["planes"].items()} == {
        "div": (0, 1), "vort": (1, 4), "vmag": (4, 5), "q": (5, 6), "l2": (6, 7), "grad": (7, 16)}
    part = ref.velgrad(u, "q,div", scale=(1.0, 0.5))
    assert part["out"].shape[1] == 2 and list(part["planes"]) == ["div", "q"]
    for n, s in part["planes"].items():
        np.testing.assert_array_equal(part["out"][:, s].view(np.uint32), full["out"][:, full["planes"][n]].view(np.uint32))
    assert ((part["flags"] & ref.FLAG_L2) == 0).all() and ((part["flags"] & 1) == (full["flags"] & 1)).all()
    np.testing.assert_array_equal(full["J"][1], ref.velgrad(u[1:], scale=0.5)["J"][0])
    assert ref.velgrad(_random((4, 5)))["out"].shape == (1, 9, 4, 5)


def test_costs_planes_stats_and_operand_errors():
    from opticalflowscivis_amd import ops
    assert ops.VG_K == 20 and ops.VG_FIELDS == ref.FIELDS and ops.VG_DEFAULT == ("div", "vmag", "q", "l2")
    assert (ops.VG_FLAG_Q, ops.VG_FLAG_L2, ops.VG_FLAG_NONFINITE) == (1, 2, 128)
    n = 128 ** 3
    b, f = ops.velgrad_cost((128, 128, 128))
    assert b == n * (4 * 3 + 4 * 4 + 1) and f > 0
    assert ops.velgrad_cost((128, 128, 128), K=3, fields="div,vort,q", with_flags=False)[0] == 3 * n * (12 + 4 * 5)
    assert ops.velgrad_cost((64, 32), fields=ref.ALL)[0] == 64 * 32 * (8 + 4 * 9 + 1)
    assert ops.velgrad_cost((8, 8, 8), fields="div,q")[1] < ops.velgrad_cost((8, 8, 8), fields="div,q,l2")[1]
    for bad in ((5,), (5, 1), (1, 4, 4), (2048, 2048, 1024)):
        with pytest.raises(ValueError):
            ops.velgrad_cost(bad)
    for bad in ("", "div,curl", [], 0, 64):
        with pytest.raises(ValueError):
            ops.velgrad_cost((8, 8), fields=bad)
    with pytest.raises(ValueError):
        ops.velgrad_cost((8, 8), K=0)
    for nd in (2, 3):
        for fields in (ref.ALL, ("l2", "div"), "vort,grad"):
            got = ops.velgrad_planes(fields, nd)
            names = fields.split(",") if isinstance(fields, str) else fields
            assert got == ref.planes(names, nd) and list(got) == [k for k in ref.FIELDS if k in names]
    assert ops.velgrad_planes(63, 3) == ref.planes(ref.ALL, 3)
    # operands
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.velgrad(torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError):
        ops.velgrad(np.zeros((1, 2, 4, 4), np.float32))
    with pytest.raises(ValueError):
        ops.velgrad(torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        ops.velgrad(torch.zeros(1, 2, 4, 4), fields="nothing")
    # statistics out of a summary
    s = torch.full((2, 20), float("nan"), dtype=torch.float64)
    s[0] = torch.tensor([2, 3, 4, 1, 1.0, 9.0, -1.0, 2.0, 8.0, 16.0, 0.0, 3.0, 4.0, 6.0, -1.0, 2.0, -4.0, 6.0, -2.0, 0.5])
    s[1, 0] = 10
    s[1, 6], s[1, 7] = math.inf, -math.inf
    st = ops.velgrad_stats(s, 10)
    a = st[0]
    assert (a["n_finite"], a["n_nonfinite"], a["frac_q_pos"], a["frac_l2_neg"], a["frac_both"]) == (8, 2, 0.3, 0.4, 0.1)
    assert a["rms_div"] == math.sqrt(9.0 / 8) and a["enstrophy"] == 1.0 and a["div_mean"] == 0.125
    assert a["vmag_mean"] == 1.0 and a["vmag_std"] == 1.0 and (a["q_min"], a["q_max"], a["l2_max"]) == (-1.0, 2.0, 0.5)
    b = st[1]
    assert b["n_finite"] == 0 and all(math.isnan(b[k]) for k in ("rms_div", "enstrophy", "div_mean", "div_min", "q_max"))
    assert math.isnan(b["frac_q_pos"])


def test_driver_arguments():
    from opticalflowscivis_amd import vortex as drv
    assert drv.step_scales([0, 1, 2], 1.0) == [1.0, 1.0] and drv.step_scales([4, 2, 1], 0.5) == [1.0, 2.0]
    for bad in (([0, 1], 0.0), ([0, 1], float("inf")), ([0, 0], 1.0)):
        with pytest.raises(ValueError):
            drv.step_scales(*bad)
    ap = drv._args(3, "x", "rife")
    ok = drv.check_args(ap.parse_args(["--flows", "f.npy"]))
    assert (ok.fields, ok.spacing, ok.dt, ok.chunk, ok.direction, ok.gap) == ("div,vmag,q,l2", [1.0], 1.0, 4, "fwd", 2)
    assert drv.check_args(ap.parse_args(["--flows", "f.npy", "--spacing", "0.5", "1", "2", "--fields", "vort,grad"]))
    assert drv._args(2, "x", "upflow").parse_args(["--dataset", "rectangle2d"]).gap == 1
    for argv in ([], ["--dataset", "droplet3d", "--seq", "s.npy"], ["--flows", "f.npy", "--chunk", "0"],
                 ["--flows", "f.npy", "--dt", "0"], ["--flows", "f.npy", "--start", "-1"],
                 ["--flows", "f.npy", "--spacing", "1", "2"], ["--flows", "f.npy", "--spacing", "0"],
                 ["--flows", "f.npy", "--fields", "div,curl"], ["--flows", "f.npy", "--fields", ""]):
        with pytest.raises(SystemExit):
            drv.check_args(ap.parse_args(argv))
    ap2 = drv._args(2, "x", "rife")
    with pytest.raises(SystemExit):
        drv.check_args(ap2.parse_args(["--flows", "f.npy", "--spacing", "1", "2", "3"]))


def test_kernel_refuses_bad_arguments_before_any_launch():
    """Argument validation happens before the launch: testable without a GPU, with dummy non-NULL device pointers."""
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    d3 = lambda *v: (ctypes.c_double * len(v))(*v)
    one, half = d3(1.0, 1.0, 1.0), d3(0.5, 0.5, 0.5)
    f3 = lambda fl=16, K=2, C=3, D=4, H=4, W=4, ss=192, ih=one, i2h=half, sc=d3(1.0, 2.0), fields=63, out=16, flags=None, \
        ws=None, summ=None: L.fs_velgrad3d(fl, K, C, D, H, W, ss, ih, i2h, sc, fields, out, flags, ws, summ, None)
    f2 = lambda fl=16, K=2, C=2, H=4, W=4, ss=32, ih=one, i2h=half, sc=d3(1.0, 2.0), fields=63, out=16, flags=None, \
        ws=None, summ=None: L.fs_velgrad2d(fl, K, C, H, W, ss, ih, i2h, sc, fields, out, flags, ws, summ, None)
    for fn, low in ((f2, 31), (f3, 191)):
        for ptr in ("fl", "ih", "i2h", "sc", "out"):
            assert fn(**{ptr: None}) == 1, ptr                                        # FS_ERR_NULLPTR
        assert fn(summ=16) == 1                                                       # a summary needs its workspace
        for kw in (dict(H=1), dict(W=1), dict(H=0), dict(C=4), dict(C=1), dict(ss=low)):
            assert fn(**kw) == 2, kw                                                  # FS_ERR_SHAPE
        for kw in (dict(fields=0), dict(fields=64), dict(fields=1 << 31), dict(K=0), dict(K=-1)):
            assert fn(**kw) == 3, kw                                                  # FS_ERR_ARG
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(sc=d3(1.0, bad)) == 3 and fn(ih=d3(1.0, bad, 1.0)) == 3 and fn(i2h=d3(bad, 0.5, 0.5)) == 3, bad
    assert f3(D=1) == 2 and f3(C=2) == 2 and f2(C=3) == 2 and f3(D=2048, H=2048, W=1024, ss=1 << 40) == 2
    assert L.fs_velgrad2d_ws_bytes(1, 2, 4, 4) == 20 * 8 and L.fs_velgrad3d_ws_bytes(3, 3, 64, 64, 64) == 3 * 1024 * 20 * 8
    assert L.fs_velgrad3d_ws_bytes(1, 3, 256, 256, 256) == 2048 * 20 * 8
    assert L.fs_velgrad2d_ws_bytes(1, 3, 4, 4) == -2 and L.fs_velgrad3d_ws_bytes(1, 3, 1, 4, 4) == -2
    assert L.fs_velgrad2d_ws_bytes(0, 2, 4, 4) == -3


def test_the_kernels_use_no_scratch_and_the_cheap_ones_fewer_registers():
    """hipcc cross-compiles gfx950 without a GPU: no kernel of velgrad.hip spills, and the instantiations without
    lambda2 do not carry the Jacobi's registers."""
    import os
    import re
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "opticalflowscivis_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("needs hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(root, "include"),
                        "-I" + csrc, "-c", os.path.join(csrc, "velgrad.hip"), "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    main = {k: v for k, v in usage.items() if "velgrad_kernel" in k}
    assert len(main) == 4 and any("velgrad_final_kernel" in k for k in usage), sorted(usage)
    for name, u in usage.items():
        if "velgrad" in name:
            assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["VGPRs"] <= 128, (name, u)
    for C in (2, 3):
        with_l2 = [u for k, u in main.items() if "ILi%dELb1E" % C in k]
        without = [u for k, u in main.items() if "ILi%dELb0E" % C in k]
        assert len(with_l2) == 1 == len(without) and without[0]["VGPRs"] < with_l2[0]["VGPRs"], (C, main)
