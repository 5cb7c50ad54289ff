"""-m gpu: fs_velgrad2d / fs_velgrad3d through ops.velgrad against the numpy fp64 restatement (tests/velgrad_ref.py):
div, the vorticity components, q and the gradient bit for bit, flags bits 0 and 7 exactly, |vort| to one fp32 rounding,
lambda2 to 2^-23 |ref| + 1e-12 ||M||_F (the Jacobi stop leaves at most 2^-45 of a scale <= 2 ||M||_F off the diagonal,
ten sweeps of fp64 rounding add about 1e-14 ||M||_F: 1e-12 leaves about 20 x headroom); the summary against the
kernel's own stored planes.  The grids are the smallest at which a stencil can go wrong: extent 2 (every difference
one-sided), rows that cross a wave (64) and a workgroup (256), odd extents.  The kernel does not tile space; its two
other paths have cases of their own: the grid-stride loop past 2048 workgroups of 256 nodes per step, and a call of more
than 256 steps, which goes out in two launches.
flags bit 1 (l2 < 0) is compared wherever the eigenvalue that decides it is farther from 0 than lambda2's bound: lambda2
itself in 3-D; in 2-D the larger of the plane's two, because the median with the embedding's 0 is exactly 0 at every
node whose two eigenvalues straddle it (most nodes of a generic field), and there bit 1 must be clear.
Measured on an MI355X: the largest lambda2 error over its bound was 0.499 on every grid -- the stored value's own fp32
rounding (2^-24 |ref| of the 2^-23 allowed); what the Jacobi adds stayed below it.  No node of any case was left out of
the bit 1 comparison."""
import functools

import numpy as np
import pytest
import torch

import velgrad_ref as ref

pytestmark = pytest.mark.gpu

GRIDS = [(2, 2), (3, 3), (5, 7), (9, 12), (2, 130), (2, 2, 2), (5, 6, 7), (3, 4, 65), (8, 8, 8), (17, 9, 33)]
KINDS = ["linear", "smooth", "noise", "constant", "planted"]
AXIS_SPACING = {2: (0.5, 2.0), 3: (0.5, 1.0, 2.0)}
# (K, spacing: one value or "axes", scale: one value or "steps")
CONFIGS = [(1, 1.0, 1.0), (3, "axes", "steps"), (3, 1.0, 0.75), (1, "axes", 1.0)]
STEP_SCALES = (2.0, 1.0 / 3.0, 1.7)
ids = lambda g: "x".join(map(str, g))


def _nodes(grid):
    return int(np.prod(grid))


@functools.lru_cache(maxsize=None)
def make_flows(grid, kind, K):
    """[K, C, *grid] fp32 step flows of one kind; seeded by its arguments."""
    C, P = len(grid), _nodes(grid)
    rng = np.random.default_rng([C, P, grid[-1], KINDS.index(kind), K])
    x = np.indices(grid)[::-1].astype(np.float64)  # component 0 = x
    one = (1,) * C
    if kind == "linear":
        A = 0.4 * rng.normal(size=(K, C, C))
        u = np.einsum("krc,c...->kr...", A, x) + rng.normal(size=(K, C) + one)
    elif kind == "constant":
        u = np.broadcast_to(rng.normal(size=(K, C) + one), (K, C) + grid)
    else:
        # 2-D: weaker waves and a rigid rotation about the grid's centre on top -- l2 < 0 needs both of the plane's
        # eigenvalues negative, which few nodes of a small grid of plain waves have
        amp, kmax = (1.5, 1.6) if C == 3 else (1.1, 1.4)
        k1 = rng.uniform(0.5, kmax, size=(K, C, C)) * rng.choice([-1.0, 1.0], size=(K, C, C))
        k2 = rng.uniform(0.5, kmax, size=(K, C, C)) * rng.choice([-1.0, 1.0], size=(K, C, C))
        ph = rng.uniform(0, 6.28, size=(2, K, C) + one)
        u = amp * np.sin(np.einsum("krc,c...->kr...", k1, x) + ph[0]) + 0.5 * amp * np.cos(np.einsum("krc,c...->kr...", k2, x) + ph[1])
        if C == 2:
            rate = rng.uniform(0.6, 1.0, size=(K, 1, 1)) * np.array([[0.0, -1.0], [1.0, 0.0]])
            ctr = np.array([(s - 1) / 2.0 for s in grid[::-1]]).reshape((C,) + one)
            u = u + np.einsum("krc,c...->kr...", rate, x - ctr)
        if kind in ("noise", "planted"):
            u = u + 0.3 * rng.normal(size=(K, C) + grid)
    u = np.ascontiguousarray(u, np.float32)
    if kind == "planted":
        flat = u.reshape(-1)
        at = rng.permutation(flat.size)[:max(1, flat.size // (100 * C))]  # about 1 % of the nodes
        flat[at] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, size=at.size)]
    u.setflags(write=False)
    return u


def _cfg(grid, cfg):
    K, spacing, scale = cfg
    return (K, AXIS_SPACING[len(grid)] if spacing == "axes" else spacing, STEP_SCALES[:K] if scale == "steps" else scale)


@functools.lru_cache(maxsize=None)
def reference(grid, kind, cfg):
    K, spacing, scale = _cfg(grid, cfg)
    r = ref.velgrad(make_flows(grid, kind, K), ref.ALL, spacing, scale)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def run(grid, kind, cfg, fields=ref.ALL, **kw):
    from opticalflowscivis_amd import ops
    K, spacing, scale = _cfg(grid, cfg)
    return ops.velgrad(torch.from_numpy(make_flows(grid, kind, K).copy()).cuda(), fields, spacing, scale, **kw)


def l2_bound(want):
    return 2.0 ** -23 * np.abs(want["l2_64"]) + 1e-12 * want["normM"]


def check(got, want, tag):
    """-> the largest lambda2 error over its bound."""
    o = got["out"].cpu().numpy()
    p = got["planes"]
    assert {n: (s.start, s.stop) for n, s in p.items()} == {n: (s.start, s.stop) for n, s in want["planes"].items()}, tag
    assert o.shape == want["out"].shape, tag
    for name in ("div", "vort", "q", "grad"):
        np.testing.assert_array_equal(o[:, p[name]].view(np.uint32), want["out"][:, p[name]].view(np.uint32),
                                      err_msg="%s %s" % (tag, name))
    flags = got["flags"].cpu().numpy()
    np.testing.assert_array_equal(flags & 129, want["flags"] & 129, err_msg=str(tag))
    bad = (want["flags"] & 128) != 0
    assert np.isnan(o[:, :][np.broadcast_to(bad[:, None], o.shape)]).all() and (flags[bad] == 128).all(), tag
    ok = ~bad
    a, b = o[:, p["vmag"]][:, 0][ok].astype(np.float64), want["out"][:, p["vmag"]][:, 0][ok].astype(np.float64)
    assert (np.abs(a - b) <= 2.0 ** -23 * np.abs(b)).all(), (tag, "vmag")
    lam = o[:, p["l2"]][:, 0].astype(np.float64)
    bound = l2_bound(want)
    err = np.abs(lam - want["l2_64"])[ok]
    ratio = float((err / np.maximum(bound[ok], 1e-300)).max()) if err.size else 0.0
    print("%s: %d finite nodes, max |l2 - ref| %.3g, max err / bound %.3g" % (tag, int(ok.sum()), err.max() if err.size else 0.0, ratio))
    assert (err <= bound[ok]).all(), (tag, "l2", float(err.max()))
    sure = ok & (np.abs(want["l2_decides"]) > bound)
    np.testing.assert_array_equal(flags[sure] & 2, want["flags"][sure] & 2, err_msg=str(tag))
    return ratio


def check_summary(got, tag):
    """The summary against the kernel's own stored planes and flags."""
    s = got["summary"].cpu().numpy()
    o = got["out"].cpu().numpy().astype(np.float64)
    flags = got["flags"].cpu().numpy()
    p = got["planes"]
    K = o.shape[0]
    assert s.shape == (K, 20), tag
    for k in range(K):
        f = flags[k]
        fin = (f & 128) == 0
        want = [(~fin).sum(), ((f & 1) != 0).sum() if "q" in p else np.nan, ((f & 2) != 0).sum() if "l2" in p else np.nan,
                ((f & 3) == 3).sum() if "q" in p and "l2" in p else np.nan]
        np.testing.assert_array_equal(s[k, :4], np.array(want, np.float64), err_msg=str(tag))
        for i, name in enumerate(("div", "vmag", "q", "l2")):
            got4 = s[k, 4 + 4 * i:8 + 4 * i]
            if name not in p:
                assert np.isnan(got4).all(), (tag, name)
                continue
            x = o[k, p[name]][0][fin]
            if x.size:
                assert got4[2] == x.min() and got4[3] == x.max(), (tag, name)
            else:
                assert got4[2] == np.inf and got4[3] == -np.inf, (tag, name)
            n = max(1, x.size)
            assert abs(got4[0] - x.sum()) <= n * 2.0 ** -52 * np.abs(x).sum(), (tag, name)
            assert abs(got4[1] - (x * x).sum()) <= n * 2.0 ** -52 * (x * x).sum(), (tag, name)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", GRIDS, ids=ids)
def test_against_the_restatement(grid, kind):
    worst = 0.0
    for cfg in CONFIGS:
        got = run(grid, kind, cfg)
        K, C = cfg[0], len(grid)
        assert got["out"].shape == (K, 5 + C * C + (C == 3) * 2) + grid and got["flags"].shape == (K,) + grid
        assert got["flags"].dtype == torch.uint8 and got["summary"].dtype == torch.float64
        worst = max(worst, check(got, reference(grid, kind, cfg), (grid, kind, cfg)))
        check_summary(got, (grid, kind, cfg))
    print("%s %s: largest lambda2 error over bound %.3g" % (ids(grid), kind, worst))
    want = reference(grid, kind, CONFIGS[0])
    if kind == "constant":
        assert (want["out"] == 0).all() and (want["flags"] == 0).all()
    if kind == "planted":
        assert (want["flags"] & 128).any()
    else:
        assert not (want["flags"] & 128).any()


@pytest.mark.parametrize("kind", ["smooth", "noise", "planted"])
@pytest.mark.parametrize("grid", [g for g in GRIDS if _nodes(g) >= 35], ids=ids)
def test_the_inputs_test_something(grid, kind):
    """On the restatement alone: both outcomes of both criteria occur, the criteria disagree somewhere, every kind of
    difference occurs, and (almost) no node's lambda2 is too close to 0 for its sign to be compared."""
    for cfg in CONFIGS:
        want = reference(grid, kind, cfg)
        fin = (want["flags"] & 128) == 0
        q = want["out"][:, want["planes"]["q"]][:, 0]
        unsure = fin & ~(np.abs(want["l2_decides"]) > l2_bound(want))
        counts = [int((fin & (q > 0)).sum()), int((fin & (q <= 0)).sum()), int((fin & (want["l2_64"] < 0)).sum()),
                  int((fin & (want["l2_64"] >= 0)).sum())]
        differ = int((fin & (((want["flags"] & 1) != 0) != ((want["flags"] & 2) != 0))).sum())
        print(grid, kind, cfg, "q > 0 / q <= 0 / l2 < 0 / l2 >= 0:", counts, "criteria differ at", differ, "unsure", int(unsure.sum()))
        assert unsure.sum() <= 0.01 * fin.size
        if kind != "planted":
            assert min(counts) >= 4 and differ >= 1
        else:
            nbad = int((~fin).sum())
            assert nbad >= 2 and fin.sum() >= 0.5 * fin.size  # the planted values poison their neighbours, not the grid
    kinds = reference(grid, kind, CONFIGS[0])["kinds"]
    present = set(np.unique(kinds).tolist())
    assert {ref.FORWARD, ref.BACKWARD} <= present and (ref.CENTRAL in present) == (max(grid) > 2)


def test_grid_stride_loop():
    """More than 2048 * 256 nodes per step: every workgroup takes a second node per thread, the last ones only some."""
    grid, cfg = (2, 513, 513), CONFIGS[0]
    assert _nodes(grid) > 2048 * 256
    got = run(grid, "noise", cfg)
    check(got, reference(grid, "noise", cfg), (grid, "noise"))
    check_summary(got, grid)


def _same(a, b, keys=("out", "flags", "summary")):
    for k in keys:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        elif x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), k


def test_step_strided_view_and_steps_in_one_launch():
    from opticalflowscivis_amd import ops
    grid = (5, 6, 7)
    stack = torch.from_numpy(make_flows(grid, "planted", 3).copy()).cuda()
    both = torch.stack([stack, stack.flip(0)], 1).reshape((6, 3) + grid)  # steps 1, 3, 5 are stack[2], stack[1], stack[0]
    view = both[1::2]
    assert view.stride(0) == 2 * 3 * _nodes(grid) and not view.is_contiguous()
    scale = STEP_SCALES
    a = ops.velgrad(view, ref.ALL, AXIS_SPACING[3], scale)
    b = ops.velgrad(view.contiguous(), ref.ALL, AXIS_SPACING[3], scale)
    _same(a, b)
    assert torch.equal(view.contiguous().view(torch.int32), stack.flip(0).view(torch.int32))  # (bits: the NaNs too)
    # K = 3 in one launch equals three launches of one step, the summary too
    for k in range(3):
        one = ops.velgrad(view[k:k + 1], ref.ALL, AXIS_SPACING[3], scale[k])
        for key in ("out", "flags", "summary"):
            _same({key: a[key][k:k + 1]}, one, (key,))


def test_other_stream_without_summary_or_flags_and_field_subsets():
    from opticalflowscivis_amd import ops
    for grid in ((17, 9, 33), (9, 12)):
        cfg = CONFIGS[1]
        full = run(grid, "planted", cfg)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            other = run(grid, "planted", cfg)
        s.synchronize()
        _same(full, other)
        bare = run(grid, "planted", cfg, with_flags=False, summary=False)
        assert sorted(bare) == ["out", "planes"]
        _same(full, bare, ("out",))
        _same(full, run(grid, "planted", cfg, summary=False), ("out", "flags"))
        for fields in ("div", "div,vort,q", ("l2",), "vmag,grad", ops.VG_DEFAULT):
            part = run(grid, "planted", cfg, fields=fields)
            names = fields.split(",") if isinstance(fields, str) else fields
            assert list(part["planes"]) == [n for n in ref.FIELDS if n in names]
            for n, sl in part["planes"].items():
                assert torch.equal(part["out"][:, sl].view(torch.int32), full["out"][:, full["planes"][n]].view(torch.int32)), (fields, n)
            want_bits = (1 if "q" in names else 0) | (2 if "l2" in names else 0) | 128
            assert torch.equal(part["flags"], full["flags"] & want_bits), fields
            check_summary(part, (grid, fields))


def test_more_steps_than_one_launch_carries():
    """The scales travel in the launch's arguments, 256 steps at a time: step 256 and later go out in a second launch."""
    from opticalflowscivis_amd import ops
    grid, K = (3, 5), 258
    rng = np.random.default_rng(11)
    u = rng.normal(size=(K, 2) + grid).astype(np.float32)
    scale = tuple(0.5 + 0.01 * k for k in range(K))
    got = ops.velgrad(torch.from_numpy(u).cuda(), ref.ALL, (0.5, 2.0), scale)
    check(got, ref.velgrad(u, ref.ALL, (0.5, 2.0), scale), "258 steps")
    check_summary(got, "258 steps")
    tail = ops.velgrad(torch.from_numpy(u[255:]).cuda(), ref.ALL, (0.5, 2.0), scale[255:])
    for key in ("out", "flags", "summary"):
        _same({key: got[key][255:]}, tail, (key,))
