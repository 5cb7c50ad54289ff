"""CPU: the fp64 restatement of line integral convolution (tests/lic_ref.py) on fields whose answer is known, and the
host-only parts of the feature: weights, noise, cost, argument checks of ops.lic and of the `lic` command lines, and the
error codes fs_lic2d / fs_lic3d return before anything is launched."""
import math
import os
import re

import numpy as np
import pytest
import torch

import lic_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH_STAGNANT = ref.STAGNANT | ref.STAGNANT << 2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _codes():
    """The restatement's end codes are the product's: ops.LIC_* and the header's FS_LIC_* enum."""
    from opticalflowscivis_amd import ops
    hdr = open(os.path.join(ROOT, "include", "flowsci_hip.h")).read()
    enum = re.search(r"enum \{ FS_LIC_FULL = (\d), FS_LIC_OUT = (\d), FS_LIC_STAGNANT = (\d), FS_LIC_NONFINITE = (\d) \};", hdr)
    want = (ref.FULL, ref.OUT, ref.STAGNANT, ref.NONFINITE)
    assert tuple(int(g) for g in enum.groups()) == want == (ops.LIC_FULL, ops.LIC_OUT, ops.LIC_STAGNANT, ops.LIC_NONFINITE)
    assert int(re.search(r"#define FS_LIC_MAX_L (\d+)", hdr).group(1)) == ops.LIC_MAX_L


def test_zero_field_returns_the_texture():
    _codes()
    sp = (5, 7)
    tex = np.random.default_rng(1).random(sp).astype(np.float32)
    for method in (ref.EULER, ref.RK2):
        out, ends, count = ref.lic_field(np.zeros((2,) + sp, np.float32), tex, ref.box(8), 0.5, 0.0, method)
        np.testing.assert_array_equal(_bits(out), _bits(tex))
        assert (ends == BOTH_STAGNANT).all() and (count == 1).all()


def test_ramp_along_a_constant_field_is_exact():
    """tex = 0.25 x along the constant field (0.75, 0, 0): every value and partial sum is exact in fp64, the symmetric
    box average of a ramp is the node's value, and the lines are cut where they leave the grid (the border is inside: the
    node x = 4 reaches x = 0 with its 8th half step)."""
    _codes()
    sp = (6, 9, 24)
    field = np.zeros((3,) + sp, np.float32)
    field[0] = 0.75
    x = np.arange(24, dtype=np.float32)
    tex = np.broadcast_to(0.25 * x, sp).astype(np.float32)
    out, ends, count = ref.lic_field(field, tex, ref.box(8), 0.5, 0.0, ref.RK2)
    np.testing.assert_array_equal(_bits(out[..., 4:20]), _bits(tex[..., 4:20]))
    assert (ends[..., 4:20] == 0).all() and (count[..., 4:20] == 17).all()
    assert (count[..., 4] == 17).all()
    assert (count[..., 3] == 15).all() and (ends[..., 3] == ref.OUT << 2).all()
    assert (count[..., 0] == 9).all() and (ends[..., 0] == ref.OUT << 2).all()
    assert (count[..., 23] == 9).all() and (ends[..., 23] == ref.OUT).all()


def test_rigid_rotation_and_the_order_of_the_integrators():
    """v = omega x r about the centre of a 33 x 33 grid (linear, so the bilinear sample is exact up to rounding),
    tex = x: the streamline through a node at radius r is its circle, the i-th sample sits at the angle i h / r, and the
    box average of x over the symmetric arc is c + (x - c) mean_i cos(i h / r).  An Euler step along the tangent grows
    r^2 by h^2; a midpoint step by h^2 (1 - cos atan(h / 2 r)) -- at least 4 times less error for 3 <= r <= 10."""
    _codes()
    n, c, omega, L, h = 33, 16.0, 0.25, 8, 0.5
    yy, xx = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    field = np.stack([-omega * (yy - c), omega * (xx - c)]).astype(np.float32)
    tex = xx.astype(np.float32)
    r = np.hypot(xx - c, yy - c)
    ring = (r >= 3) & (r <= 10)
    i = np.arange(-L, L + 1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = c + (xx - c) * np.cos(i[:, None, None] * h / r).mean(0)
    err = {}
    for method in (ref.EULER, ref.RK2):
        out, ends, count = ref.lic_field(field, tex, ref.box(L), h, 0.0, method)
        assert (ends[ring] == 0).all() and (count[ring] == 2 * L + 1).all()
        err[method] = np.abs(out.astype(np.float64) - want)[ring].max()
    print("max error: euler %.4g, rk2 %.4g" % (err[ref.EULER], err[ref.RK2]))
    assert err[ref.RK2] * 4 <= err[ref.EULER]
    assert err[ref.EULER] < 0.5


def test_nonfinite_values_end_a_side_or_propagate():
    _codes()
    sp = (4, 6)
    field = np.zeros((2,) + sp, np.float32)
    field[0] = 1.0
    field[1, 2, 3] = np.nan
    tex = np.ones(sp, np.float32)
    tex[0, 1] = np.inf
    out, ends, count = ref.lic_field(field, tex, ref.box(2), 1.0, 0.0, ref.EULER)
    # the four nodes whose corner set holds the NaN (two of them with weight 0) go nowhere
    assert (ends[1:3, 2:4] == (ref.NONFINITE | ref.NONFINITE << 2)).all() and (count[1:3, 2:4] == 1).all()
    assert ends[2, 1] == (ref.NONFINITE | ref.OUT << 2) and count[2, 1] == 3  # one step towards them, one to the border
    assert ends[2, 4] == (ref.OUT | ref.NONFINITE << 2) and count[2, 4] == 3
    # the texture's inf: NaN where it is a corner of weight 0 (the sample at x = 0), inf where it is the sample itself
    assert np.isnan(out[0, :3]).all() and np.isposinf(out[0, 3]) and (out[0, 4:] == 1.0).all()
    assert (out[1:] == 1.0).all()


def test_hann_weights_equal_the_formula():
    from opticalflowscivis_amd import ops
    for L in (0, 1, 8, 16):
        w = ops.lic_weights(L, "hann", "cpu")
        assert w.dtype == torch.float64 and w.shape == (L + 1,)
        assert w.tolist() == [0.5 * (1.0 + math.cos(math.pi * i / (L + 1))) for i in range(L + 1)]
        np.testing.assert_allclose(w.numpy(), ref.hann(L), rtol=0, atol=2.5e-16)
        assert w[0] == 1.0 and (w > 0).all()
        assert ops.lic_weights(L, "box", "cpu").tolist() == [1.0] * (L + 1)
    for bad in (-1, ops.LIC_MAX_L + 1, 1.5):
        with pytest.raises(ValueError, match="length"):
            ops.lic_weights(bad, "box", "cpu")
    with pytest.raises(ValueError, match="kernel"):
        ops.lic_weights(4, "gauss", "cpu")


def test_noise_is_reproducible():
    from opticalflowscivis_amd import ops
    a, b = ops.lic_noise((5, 6, 7), 3, "cpu"), ops.lic_noise((5, 6, 7), 3, "cpu")
    assert a.dtype == torch.float32 and a.shape == (5, 6, 7) and torch.equal(a, b)
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0 and a.unique().numel() > 100
    assert not torch.equal(a, ops.lic_noise((5, 6, 7), 4, "cpu"))
    torch.manual_seed(99)  # the global generator plays no part
    assert torch.equal(a, ops.lic_noise((5, 6, 7), 3, "cpu"))
    with pytest.raises(ValueError):
        ops.lic_noise((4, 0), 0, "cpu")


def test_cost():
    from opticalflowscivis_amd import ops
    nb, fl = ops.lic_cost((256, 256, 256), 1, 16, "rk2")
    n = 256 ** 3
    assert nb == n * (12 + 4 + 4 + 1 + 4) + 8 * 17
    assert ops.lic_cost((256, 256, 256), 1, 16, "rk2", with_ends=False, with_count=False)[0] == n * 20 + 8 * 17
    assert ops.lic_cost((8, 8), 3, 4, "euler", shared_tex=True)[0] == 64 * (3 * 8 + 4 + 3 * 9) + 8 * 5
    # 64 field samples and 33 texture samples per node
    vs, ts = 8 * 2 + 2 * 8 * 3 + 12 + 9 + 6, 8 * 2 + 2 * 8 + 12 + 3 + 6
    assert fl == n * (64 * vs + 33 * ts + 5)
    assert ops.lic_cost((256, 256, 256), 1, 16, "euler")[1] == n * (32 * vs + 33 * ts + 5)
    assert ops.lic_cost((8, 8), 2, 0, "rk2")[1] == 2 * 64 * ((4 + 8 + 8 + 3 + 4) + 5)
    for bad in (dict(method="rk4"), dict(L=-1), dict(shape=(8,)), dict(shape=(8, 0))):
        kw = dict(shape=(8, 8), K=1, L=4, method="rk2")
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.lic_cost(**kw)


def test_op_refuses_bad_arguments_and_cpu_tensors():
    from opticalflowscivis_amd import ops
    fl, tex = torch.zeros(1, 2, 4, 4), torch.zeros(4, 4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.lic(fl, tex)
    for kw, what in ((dict(method="rk4"), "method"), (dict(length=-1), "length"), (dict(length=1025), "length"),
                     (dict(h=0.0), "h must"), (dict(h=float("inf")), "h must"), (dict(vmin=-1.0), "vmin"),
                     (dict(vmin=float("nan")), "vmin")):
        with pytest.raises(ValueError, match=what):
            ops.lic(fl, tex, **kw)
    with pytest.raises(ValueError, match="flows must be"):
        ops.lic(torch.zeros(2, 4, 4), tex)
    assert (ops.LIC_FULL, ops.LIC_OUT, ops.LIC_STAGNANT, ops.LIC_NONFINITE, ops.LIC_MAX_L) == (0, 1, 2, 3, 1024)


def test_command_lines():
    from opticalflowscivis_amd import lic
    ap = lic._args(2, "x", "rife")
    a = lic.check_args(ap.parse_args(["--flows", "f.npy"]))
    assert (a.length, a.h, a.method, a.kernel, a.passes, a.vmin, a.noise_seed, a.texture, a.out, a.ends, a.png_dir,
            a.save_flows, a.chunk) == (16, 0.5, "rk2", "box", 1, 0.0, 0, None, None, None, None, None, 4)
    a = lic.check_args(lic._args(3, "x", "rife").parse_args(
        ["--flows", "f.npy", "--length", "8", "--h", "0.25", "--method", "euler", "--kernel", "hann", "--passes", "2",
         "--vmin", "0.1", "--noise-seed", "7", "--texture", "t.npy", "--out", "o.npy", "--ends", "e.npy"]))
    assert (a.length, a.h, a.method, a.kernel, a.passes, a.vmin, a.noise_seed, a.texture, a.out, a.ends) == (
        8, 0.25, "euler", "hann", 2, 0.1, 7, "t.npy", "o.npy", "e.npy")
    assert not hasattr(a, "png_dir")  # pictures of 3-D fields are `render`'s
    for bad in (["--length", "-1"], ["--length", "1025"], ["--h", "0"], ["--h", "nan"], ["--vmin", "-1"],
                ["--passes", "0"], ["--method", "rk4"], ["--kernel", "gauss"], ["--chunk", "0"]):
        with pytest.raises(SystemExit):
            lic.check_args(lic._args(2, "x", "upflow").parse_args(["--flows", "f.npy"] + bad))
    with pytest.raises(SystemExit):
        lic.check_args(lic._args(2, "x", "rife").parse_args([]))
    with pytest.raises(SystemExit):
        lic._args(3, "x", "rife").parse_args(["--flows", "f.npy", "--png-dir", "d"])


def test_error_codes_without_gpu():
    """Argument validation happens before any launch, so it is testable on the CPU (the pointers are never followed)."""
    from opticalflowscivis_amd import _lib
    lib = _lib.lib()

    def c3(flows=1, K=2, C=3, D=4, H=4, W=4, fss=192, tex=1, tss=64, w=1, L=2, h=0.5, vmin=0.0, m=1, out=1, ws=16):
        return lib.fs_lic3d(flows, K, C, D, H, W, fss, tex, tss, w, L, h, vmin, m, out, None, None, ws, None)

    def c2(flows=1, K=2, C=2, H=4, W=4, fss=32, tex=1, tss=0, w=1, L=2, h=0.5, vmin=0.0, m=0, out=1, ws=16):
        return lib.fs_lic2d(flows, K, C, H, W, fss, tex, tss, w, L, h, vmin, m, out, None, None, ws, None)

    for c in (c2, c3):
        assert [c(flows=None), c(tex=None), c(w=None), c(out=None), c(ws=None)] == [1] * 5              # NULLPTR
        assert [c(K=0), c(C=1), c(C=4), c(H=0), c(W=0), c(fss=c.__defaults__[6 if c is c3 else 5] - 1),
                c(tss=15), c(tss=-1)] == [2] * 8                                                      # SHAPE
        assert [c(L=-1), c(L=1025), c(h=0.0), c(h=-0.5), c(h=float("inf")), c(h=float("nan")), c(vmin=-0.25),
                c(vmin=float("inf")), c(vmin=float("nan")), c(m=2), c(m=-1), c(ws=24)] == [3] * 12     # ARG
    assert c3(D=0) == 2 and c3(C=2) == 2 and c2(C=3) == 2
    assert c3(tss=63) == 2
    # the workspace: 16 bytes per node and step
    assert lib.fs_lic3d_ws_bytes(2, 4, 5, 6) == 16 * 2 * 120 and lib.fs_lic2d_ws_bytes(3, 5, 7) == 16 * 3 * 35
    assert lib.fs_lic3d_ws_bytes(0, 4, 4, 4) == -2 and lib.fs_lic3d_ws_bytes(1, 4, 0, 4) == -2
    assert lib.fs_lic2d_ws_bytes(1, 0, 4) == -2 and lib.fs_lic2d_ws_bytes(1, 2 ** 30, 2 ** 30) == -2
