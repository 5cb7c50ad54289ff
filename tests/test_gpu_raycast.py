"""-m gpu: fs_raycast3d / fs_brick_range3d through ops.raycast and ops.brick_ranges against the numpy restatement
(tests/raycast_ref.py).  For every case E32 = max |restatement in fp32 - restatement in fp64| is computed here on the CPU
and the kernel must satisfy |gpu - fp64| <= 8 E32 + 2^-22 at every pixel and channel: the kernel works in fp32 like the
fp32 restatement (same sample positions, bit for bit) but fuses the multiply-adds of its interpolations and blends, and
its exp is the device's.
Volumes of one, two and exactly two bricks per axis, anisotropic spacing, pictures of 12 x 16, 1 x 1 and 9 x 70 pixels
(a partial 8 x 8 tile in both directions, more than one workgroup), both cameras and both modes; a view straight down an
axis (two direction components exactly 0), a perspective eye inside the volume, a camera whose rays all miss, three
frames with three cameras, and a volume with about 1 % planted NaN and +-inf.  Jumps over empty bricks, batching and
early termination are compared between the kernel's own results, bit for bit where the header promises it.
Measured on an MI355X: the largest |gpu - fp64| over its bound was 0.151 across the 74 accuracy cases (about 1.2 E32 of the
8 E32 allowed): the kernel's error is the fp32 restatement's own; no pixel of any case was left out."""
import functools

import numpy as np
import pytest
import torch

import raycast_ref as ref

pytestmark = pytest.mark.gpu

VOLUMES = [((2, 2, 2), 1.0), ((5, 6, 7), (0.5, 1.0, 2.0)), ((3, 4, 9), 1.0), ((8, 8, 8), 1.0), ((9, 17, 10), 1.0)]
IMAGES = [(12, 16), (1, 1), (9, 70)]
MODES = [ref.DVR, ref.MIP]
LO, HI = 0.125, 0.875
ids = lambda v: "x".join(map(str, v[0])) if isinstance(v[0], tuple) else "x".join(map(str, v))


@functools.lru_cache(maxsize=None)
def volume(shape, kind="random", K=1):
    rng = np.random.default_rng([shape[0], shape[1], shape[2], K, len(kind)])
    v = rng.random((K,) + shape, dtype=np.float32)
    if kind == "planted":
        flat = v.reshape(-1)
        at = rng.permutation(flat.size)[:max(3, flat.size // 100)]  # about 1 % of the nodes
        flat[at] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(at.size) % 3]
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def table():
    """Seven rows; row 0 is zero (a ray that meets nothing is black and clear in both modes), A up to 1.5."""
    rng = np.random.default_rng(11)
    t = rng.random((7, 4), dtype=np.float32)
    t[:, 3] *= 1.5
    t[0] = 0
    t.setflags(write=False)
    return t


def camera(kind, shape, spacing, image):
    from opticalflowscivis_amd import render
    Hi, Wi = image
    if kind == "ortho":
        return render.orbit_camera(shape, spacing, 30.0, 20.0, None, image)
    if kind == "persp":
        return render.orbit_camera(shape, spacing, -50.0, 35.0, None, image, fov=40.0)
    if kind == "inside":  # the eye at the volume's centre, looking towards the far +x +y +z corner
        return render.orbit_camera(shape, spacing, -140.0, -23.0, 0.0, image, fov=70.0)
    if kind == "miss":  # the orthographic camera turned round
        c = render.orbit_camera(shape, spacing, 30.0, 20.0, None, image).copy()
        c[9:12] = -c[9:12]
        return c
    if kind == "axis":  # straight down z from below: the picture spans the volume and a margin that misses
        h = np.broadcast_to(np.float64(spacing), (3,))[::-1]
        size = [(n - 1) * s for n, s in zip(shape[::-1], h)]
        px, py = (size[0] + 3.0 * h[0]) / Wi, (size[1] + 3.0 * h[1]) / Hi
        return np.float32([-1.4 * h[0], -1.3 * h[1], -3.0 * h[2], px, 0, 0, 0, py, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
    raise KeyError(kind)


def gpu_render(vols, cams, image, spacing, mode, dt=None, t_min=0.0, bricks=False, counts=False, tf=None, lo=LO, hi=HI):
    from opticalflowscivis_amd import ops
    v = torch.from_numpy(np.array(vols, np.float32)).cuda()
    br = ops.brick_ranges(v) if bricks else None
    r = ops.raycast(v, np.stack(cams), table() if tf is None else tf, lo, hi, dt, spacing, mode, t_min, br, counts, image)
    torch.cuda.synchronize()
    return (r["image"].cpu().numpy(), r["counts"].cpu().numpy()) if counts else r["image"].cpu().numpy()


def check_accuracy(vols, cams, image, spacing, mode, dt=None):
    """The largest |gpu - fp64| over its bound 8 E32 + 2^-22 (asserted <= 1)."""
    h = np.broadcast_to(np.float64(spacing), (3,))
    step = 0.5 * float(h.min()) if dt is None else dt
    r64 = ref.raycast_frames(vols, cams, table(), LO, HI, step, spacing, image, mode, dtype=np.float64)
    r32 = ref.raycast_frames(vols, cams, table(), LO, HI, step, spacing, image, mode, dtype=np.float32)
    e32 = float(np.abs(r32.astype(np.float64) - r64).max())
    got = gpu_render(vols, cams, image, spacing, mode, dt)
    assert got.shape == r64.shape and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - r64).max())
    bound = 8.0 * e32 + 2.0 ** -22
    print("raycast accuracy: E32 %.3e  err %.3e  ratio %.3f" % (e32, err, err / bound))
    assert np.isfinite(got).all()
    assert err <= bound, (err, e32, bound)
    return err / bound, r64


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cam", ["ortho", "persp"])
@pytest.mark.parametrize("image", IMAGES, ids=ids)
@pytest.mark.parametrize("vol", VOLUMES, ids=ids)
def test_accuracy(vol, image, cam, mode):
    shape, spacing = vol
    _, r64 = check_accuracy(volume(shape), [camera(cam, shape, spacing, image)], image, spacing, mode)
    if image != (1, 1):
        assert r64.max() > 0.05  # the picture shows the volume


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cam", ["axis", "inside"])
@pytest.mark.parametrize("vol", [VOLUMES[1], VOLUMES[4]], ids=ids)
def test_accuracy_axis_view_and_eye_inside(vol, cam, mode):
    shape, spacing = vol
    c = camera(cam, shape, spacing, (12, 16))
    if cam == "axis":
        assert c[9] == 0 and c[10] == 0 and c[11] == 1
    _, r64 = check_accuracy(volume(shape), [c], (12, 16), spacing, mode)
    assert r64.max() > 0.05
    if cam == "axis":
        assert (r64[0, 0] == 0).all()  # the margin misses: the slab test's zero direction components reject it


@pytest.mark.parametrize("mode", MODES)
def test_accuracy_three_frames_three_cameras(mode):
    shape, spacing = VOLUMES[1]
    image = (9, 70)
    cams = [camera(k, shape, spacing, image) for k in ("ortho", "persp", "axis")]
    check_accuracy(volume(shape, K=3), cams, image, spacing, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cam", ["ortho", "persp"])
def test_accuracy_with_planted_nonfinite_values(cam, mode):
    shape, spacing = VOLUMES[4]
    v = volume(shape, "planted")
    assert 0.005 < (~np.isfinite(v)).mean() < 0.02
    _, r64 = check_accuracy(v, [camera(cam, shape, spacing, (12, 16))], (12, 16), spacing, mode)
    assert r64.max() > 0.05


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("image", IMAGES, ids=ids)
def test_rays_that_all_miss_give_exactly_zero(image, mode):
    shape, spacing = VOLUMES[1]
    got, counts = gpu_render(volume(shape), [camera("miss", shape, spacing, image)], image, spacing, mode, counts=True)
    assert (got == 0).all() and (counts == 0).all()


def skip_cases():
    """(volumes, table): zero but for a blob in the far corner; a ramp that falls along x, whose lower half (the far half,
    the one the eye inside the volume looks into) the table leaves clear; the ramp with two planted values."""
    shape = (17, 20, 33)
    z, y, x = np.indices(shape).astype(np.float32)
    blob = np.exp(-((z - 13) ** 2 + (y - 16) ** 2 + (x - 28) ** 2) / 8.0).astype(np.float32)
    blob[blob < 0.05] = 0
    assert (blob[:9, :9, :17] == 0).all() and blob.max() > 0.9
    ramp = (1.0 - x / 32.0 + 0.01 * np.sin(y + z)).astype(np.float32)
    planted = ramp.copy()
    planted[3, 4, 5], planted[12, 15, 30] = np.nan, np.inf
    tf = np.random.default_rng(2).random((8, 4), dtype=np.float32)
    tf[:4, 3] = 0  # A = 0 on the lower half
    return {"blob": blob, "ramp": ramp, "planted": planted}, tf


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cam", ["ortho", "persp", "axis", "inside"])
@pytest.mark.parametrize("name", ["blob", "ramp", "planted"])
def test_jumping_over_empty_bricks_changes_no_bit(name, cam, mode):
    vols, tf = skip_cases()
    v = vols[name][None]
    image, spacing = (12, 16), 1.0
    c = [camera(cam, v.shape[1:], spacing, image)]
    # mip jumps where nothing exceeds lo: put lo inside the ramp's range
    lo, hi = (0.0, 1.0) if mode == ref.DVR or name == "blob" else (0.5, 1.0)
    plain, n_plain = gpu_render(v, c, image, spacing, mode, counts=True, tf=tf, lo=lo, hi=hi)
    jumped, n_jumped = gpu_render(v, c, image, spacing, mode, bricks=True, counts=True, tf=tf, lo=lo, hi=hi)
    assert plain.max() > 0.05
    np.testing.assert_array_equal(plain.view(np.uint32), jumped.view(np.uint32))
    assert (n_jumped <= n_plain).all()
    assert n_jumped.sum() < n_plain.sum(), (n_jumped.sum(), n_plain.sum())


def test_a_table_that_is_opaque_everywhere_jumps_nothing():
    vols, _ = skip_cases()
    v = vols["blob"][None]
    c = [camera("ortho", v.shape[1:], 1.0, (12, 16))]
    plain, n_plain = gpu_render(v, c, (12, 16), 1.0, ref.DVR, counts=True, lo=-1.0, hi=1.0)
    jumped, n_jumped = gpu_render(v, c, (12, 16), 1.0, ref.DVR, bricks=True, counts=True, lo=-1.0, hi=1.0)
    np.testing.assert_array_equal(plain.view(np.uint32), jumped.view(np.uint32))
    np.testing.assert_array_equal(n_plain, n_jumped)


@pytest.mark.parametrize("kind", ["random", "planted"])
def test_brick_ranges_match_the_restatement(kind):
    from opticalflowscivis_amd import ops
    for shape in [(2, 2, 2), (9, 17, 10), (17, 20, 33)]:
        v = volume(shape, kind, K=2)
        stack = torch.from_numpy(np.repeat(v, 2, axis=0)).cuda()[::2]  # a step stride of two volumes, read in place
        r = ops.brick_ranges(stack)
        for k in range(2):
            rng, bad = ref.brick_ranges(v[k])
            np.testing.assert_array_equal(r["range"][k].cpu().numpy(), rng)
            np.testing.assert_array_equal(r["nonfinite"][k].cpu().numpy(), bad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bricks", [False, True])
def test_a_batch_equals_single_launches_bit_for_bit(mode, bricks):
    from opticalflowscivis_amd import ops
    shape, spacing = VOLUMES[4]
    image = (9, 70)
    v = volume(shape, "planted", K=3)
    cams = [camera(k, shape, spacing, image) for k in ("ortho", "persp", "inside")]
    together, n_together = gpu_render(v, cams, image, spacing, mode, bricks=bricks, counts=True)
    for k in range(3):
        alone, n_alone = gpu_render(v[k:k + 1], cams[k:k + 1], image, spacing, mode, bricks=bricks, counts=True)
        np.testing.assert_array_equal(together[k].view(np.uint32), alone[0].view(np.uint32))
        np.testing.assert_array_equal(n_together[k], n_alone[0])
    # every other volume of a stack, read in place
    stack = torch.from_numpy(np.repeat(v, 2, axis=0)).cuda()[::2]
    assert stack.stride(0) == 2 * v[0].size
    r = ops.raycast(stack, np.stack(cams), table(), LO, HI, None, spacing, mode, image=image)
    np.testing.assert_array_equal(r["image"].cpu().numpy().view(np.uint32), together.view(np.uint32))


@pytest.mark.parametrize("cam", ["ortho", "inside"])
def test_early_termination_stays_within_t_min(cam):
    shape, spacing = VOLUMES[4]
    image, t_min = (12, 16), 1.0 / 256
    tf = table().copy()
    tf[1:, 3] += 2.0  # dense enough for rays to end early
    c = [camera(cam, shape, spacing, image)]
    full, n_full = gpu_render(volume(shape), c, image, spacing, ref.DVR, counts=True, tf=tf)
    cut, n_cut = gpu_render(volume(shape), c, image, spacing, ref.DVR, t_min=t_min, counts=True, tf=tf)
    assert n_cut.sum() < n_full.sum() and (n_cut <= n_full).all()
    bound = t_min * max(1.0, float(tf[:, :3].max()))
    assert np.abs(full.astype(np.float64) - cut.astype(np.float64)).max() <= bound
    assert (1.0 - cut[..., 3]).min() < t_min  # some ray did end early


def test_ops_validate_their_operands():
    from opticalflowscivis_amd import ops
    shape, spacing = VOLUMES[3]
    v = torch.from_numpy(volume(shape).copy()).cuda()
    cam = camera("ortho", shape, spacing, (4, 4))
    ok = dict(volumes=v, cameras=cam, tf=table(), lo=0.0, hi=1.0, image=(4, 4))
    assert ops.raycast(**ok)["image"].shape == (1, 4, 4, 4)
    bad_tf = table().copy()
    bad_tf[2, 3] = -1
    for bad in (dict(image=None), dict(image=(0, 4)), dict(mode="xray"), dict(lo=1.0), dict(dt=0.0), dict(dt=1e-7),
                dict(t_min=1.0), dict(spacing=(1.0, 2.0)), dict(cameras=np.zeros((2, 18), np.float32)),
                dict(cameras=np.zeros(17, np.float32)), dict(tf=np.zeros((1, 4), np.float32)), dict(tf=bad_tf),
                dict(tf=np.zeros((4, 3), np.float32)), dict(volumes=v[0]), dict(volumes=v.double()),
                dict(volumes=v[:, :1]), dict(bricks={"range": v}), dict(bricks=ops.brick_ranges(torch.cat([v, v])))):
        with pytest.raises(ValueError):
            ops.raycast(**{**ok, **bad})
