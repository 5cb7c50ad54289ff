"""-m gpu: fs_iso_count3d / fs_iso_emit3d through ops.isosurface against the numpy restatement (tests/isosurface_ref.py).
Offsets and faces must be equal as arrays and the vertices equal bit for bit.  For normals and values E32 = max
|restatement in fp32 - restatement in fp64| is computed here on the CPU and the kernel must satisfy |gpu - fp64| <= 8 E32 +
2^-22 scale at every vertex and component (scale 1 for normals, max |w| for values): the kernel works in fp32 like the
fp32 restatement but may fuse its multiply-adds.
A single cell with all 254 mixed corner patterns as 254 volumes of one launch; (3,4,9), (5,6,70) -- a row longer than a
wave, so the in-row prefix crosses chunks -- and (9,17,33); anisotropic spacing; white noise, an integer field with nodes
exactly on the isovalue, about 1 % planted NaN and +-inf, an isovalue above the maximum, three volumes read in place from
a stack's every other step; two calls compared bit for bit; the sphere and the torus closed and oriented from the GPU's
own arrays.
Measured on an MI355X: the largest |gpu - fp64| over its bound was 0.140 for normals (the 254 single cells) and 0.089
for values across the 10 accuracy cases (about one E32 of the 8 allowed): the kernel's error is the fp32 restatement's
own; no vertex of any case was left out."""
import functools

import numpy as np
import pytest
import torch

import isosurface_ref as R

pytestmark = pytest.mark.gpu

CASES = [((3, 4, 9), 1.0), ((5, 6, 70), 1.0), ((9, 17, 33), 1.0), ((5, 6, 70), (0.5, 1.0, 2.0))]
ids = lambda c: "x".join(map(str, c[0])) + ("" if c[1] == 1.0 else "-aniso")


def xyz(spacing):
    """ops takes the spacing as one value or (D,H,W); the restatement as (x, y, z)."""
    return tuple(float(v) for v in np.broadcast_to(np.float64(spacing), (3,))[::-1])


@functools.lru_cache(maxsize=None)
def field(shape, kind, K=2):
    rng = np.random.default_rng([shape[0], shape[1], shape[2], K, len(kind)])
    v = rng.standard_normal((K,) + shape).astype(np.float32)
    if kind == "planted":
        flat = v.reshape(-1)
        at = rng.permutation(flat.size)[:max(3, flat.size // 100)]  # about 1 % of the nodes
        flat[at] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(at.size) % 3]
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def colours(shape, K=2):
    """Two planes: noise of magnitude about 3 and a ramp along x."""
    rng = np.random.default_rng([7, shape[0], shape[1], shape[2], K])
    w = np.empty((K, 2) + shape, np.float32)
    w[:, 0] = 3.0 * rng.standard_normal((K,) + shape)
    w[:, 1] = np.arange(shape[2], dtype=np.float32) * 0.25 - 1.0
    w.setflags(write=False)
    return w


def gpu_iso(vols, iso, spacing=1.0, values=None, normals=True):
    from opticalflowscivis_amd import ops
    v = vols if isinstance(vols, torch.Tensor) else torch.from_numpy(np.array(vols, np.float32)).cuda()
    w = None if values is None else torch.from_numpy(np.array(values, np.float32)).cuda()
    r = ops.isosurface(v, iso, spacing, normals, w)
    torch.cuda.synchronize()
    ops.isosurface_check(r)
    return {k: t.cpu().numpy() for k, t in r.items()}


def check(vols, iso, spacing=1.0, values=None):
    """Compares ops.isosurface with the restatement; returns (reference, result, the largest |gpu - fp64| over its bound
    for normals, and for values)."""
    ref = R.extract_series(np.asarray(vols), iso, xyz(spacing), values)
    got = gpu_iso(vols, iso, spacing, values)
    assert got["status"].tolist() == [0]
    np.testing.assert_array_equal(got["vertex_offsets"], ref["vertex_offsets"])
    np.testing.assert_array_equal(got["face_offsets"], ref["face_offsets"])
    assert got["vertex_offsets"].dtype == np.int64 and got["faces"].dtype == np.int32
    np.testing.assert_array_equal(got["faces"], ref["faces"])
    assert got["vertices"].shape == ref["vertices"].shape and got["vertices"].dtype == np.float32
    np.testing.assert_array_equal(got["vertices"].view(np.uint32), ref["vertices"].view(np.uint32))
    ratios = []
    for name, scale in (("normals", 1.0), ("values", None)):
        if name == "values" and values is None:
            ratios.append(0.0)
            continue
        r64, r32 = ref[name + "64"], ref[name + "32"].astype(np.float64)
        assert got[name].shape == r64.shape  # every vertex and component is compared
        if r64.size == 0:
            ratios.append(0.0)
            continue
        if scale is None:
            scale = float(np.abs(np.asarray(values)).max())
        e32 = float(np.abs(r32 - r64).max())
        bound = 8.0 * e32 + 2.0 ** -22 * scale
        err = float(np.abs(got[name].astype(np.float64) - r64).max())
        print("%s: E32 %.3e  |gpu - fp64| %.3e  bound %.3e  ratio %.3f" % (name, e32, err, bound, err / bound))
        assert err <= bound, (name, err, bound, e32)
        ratios.append(err / bound)
    return ref, got, ratios[0], ratios[1]


def test_every_corner_pattern_of_a_single_cell():
    rng = np.random.default_rng(3)
    mag = 0.25 + rng.random((254, 8), dtype=np.float32)
    bits = (np.arange(1, 255)[:, None] >> np.arange(8)) & 1
    vols = np.where(bits == 1, mag, -mag).astype(np.float32).reshape(254, 2, 2, 2)
    ref, got, _, _ = check(vols, 0.0)
    assert (np.diff(got["face_offsets"]) >= 2).all() and (np.diff(got["vertex_offsets"]) >= 3).all()


@pytest.mark.parametrize("case", CASES, ids=ids)
@pytest.mark.parametrize("kind", ["noise", "planted"])
def test_against_the_restatement(case, kind):
    shape, spacing = case
    vols = field(shape, kind)
    ref, got, _, _ = check(vols, 0.1, spacing, colours(shape))
    assert got["faces"].shape[0] > 0
    if kind == "planted":  # no face comes from a cell with a corner that is not finite
        bad = ~np.isfinite(vols)
        for k in range(vols.shape[0]):
            cell = ref["face_cell"][ref["face_offsets"][k]:ref["face_offsets"][k + 1]]
            z, y, x = np.unravel_index(cell, shape)
            for c in range(8):
                assert not bad[k, z + (c >> 2 & 1), y + (c >> 1 & 1), x + (c & 1)].any()
        assert np.isfinite(got["vertices"]).all() and np.isfinite(got["normals"]).all()


def test_integer_field_with_nodes_on_the_isovalue():
    f = R.integer_field()
    ref, got, _, _ = check(f[None], 0.0, 1.0, np.stack([f * 0.5])[None])
    t = R.topology(got["faces"], got["vertices"].shape[0])
    assert t["bad_edges"] == 0 and got["vertices"].shape[0] - t["edges"] + got["faces"].shape[0] == 2


def test_isovalue_above_the_maximum_launches_nothing_more():
    from opticalflowscivis_amd import ops
    vols = field((5, 6, 70), "noise")
    ops.enable_kernel_timing(True)
    try:
        got = gpu_iso(vols, 100.0, values=colours((5, 6, 70)))
        launched = sorted(ops.kernel_timings())
    finally:
        ops.enable_kernel_timing(False)
    assert launched == ["fs_iso_count3d"]
    assert got["vertices"].shape == (0, 3) and got["normals"].shape == (0, 3) and got["values"].shape == (0, 2)
    assert got["faces"].shape == (0, 3) and got["faces"].dtype == np.int32
    assert got["vertex_offsets"].tolist() == [0, 0, 0] and got["face_offsets"].tolist() == [0, 0, 0]
    assert got["status"].tolist() == [0]


def test_every_other_step_is_read_in_place():
    stack = field((3, 4, 9), "noise", 5)
    dev = torch.from_numpy(np.array(stack)).cuda()
    view = dev[::2]
    assert not view.is_contiguous() and view.stride(0) == 2 * 3 * 4 * 9
    ref = R.extract_series(stack[::2], 0.1)
    got = gpu_iso(view, 0.1)
    np.testing.assert_array_equal(got["faces"], ref["faces"])
    np.testing.assert_array_equal(got["vertices"].view(np.uint32), ref["vertices"].view(np.uint32))
    np.testing.assert_array_equal(got["vertex_offsets"], ref["vertex_offsets"])
    assert len(got["vertex_offsets"]) == 4


def test_two_calls_return_the_same_bits():
    vols, w = field((9, 17, 33), "planted"), colours((9, 17, 33))
    a, b = gpu_iso(vols, 0.1, (0.5, 1.0, 2.0), w), gpu_iso(vols, 0.1, (0.5, 1.0, 2.0), w)
    assert sorted(a) == sorted(b) == ["face_offsets", "faces", "normals", "status", "values", "vertex_offsets", "vertices"]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = gpu_iso(vols, 0.1, (0.5, 1.0, 2.0), None, normals=False)
    assert "normals" not in c and "values" not in c and c["vertices"].tobytes() == a["vertices"].tobytes()


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0)])
def test_closed_and_oriented_on_the_gpu(name, euler):
    f = R.sphere_field(16)[0] if name == "sphere" else R.torus_field()
    got = gpu_iso(f[None], 0.0)
    V, T = got["vertices"].shape[0], got["faces"].shape[0]
    t = R.topology(got["faces"], V)
    assert t["bad_edges"] == 0 and t["degenerate"] == 0 and t["used_vertices"] == V
    assert V - t["edges"] + T == euler
    area, vol = R.area_volume(got["vertices"], got["faces"])
    assert vol > 0
    v, fc, n = got["vertices"].astype(np.float64), got["faces"], got["normals"].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-5
    g = np.cross(v[fc[:, 1]] - v[fc[:, 0]], v[fc[:, 2]] - v[fc[:, 0]])
    assert ((g * n[fc].sum(1)).sum(1) >= 0).all()  # the winding agrees with the gradient's normals
    if name == "sphere":  # away from the centre
        assert ((n * (v - np.array([7.4, 7.6, 7.2]))).sum(1) > 0).all()
