"""-m gpu: fs_ftle2d / fs_ftle3d through ops.ftle against the numpy fp64 restatement (tests/ftle_ref.py): classes equal,
the Cauchy-Green tensor bit for bit, the exponent to one fp32 rounding; the summary against the kernel's own stored
outputs.  The lattices are the smallest at which a stencil can go wrong: extent 2 (every difference one-sided), rows that
cross a wave (64) and a workgroup (256), odd extents.  The kernel does not tile space; its one other path, the
grid-stride loop past 2048 workgroups of 256 nodes, has a lattice of its own.  Measured on an MI355X: the stored exponents
equalled the restatement's at every OK node of every case (largest error over bound: 0)."""
import functools

import numpy as np
import pytest
import torch

import ftle_ref as ref

pytestmark = pytest.mark.gpu

LATTICES = [(2, 2), (3, 3), (5, 7), (9, 12), (2, 130), (2, 2, 2), (5, 6, 7), (3, 4, 65), (8, 8, 8), (17, 9, 33)]
KINDS = ["linear", "smooth", "noise", "collapsed", "status"]
# (spacing, T, valid mask, accept_out)
CONFIGS = [(1.0, 2.0, False, False), (0.5, 0.75, True, True), (1.0, 1.0, False, True), (0.5, 3.0, True, False)]


def _nodes(lattice):
    return int(np.prod(lattice))


@functools.lru_cache(maxsize=None)
def make_map(lattice, kind, spacing):
    """(pos [C,P] fp32, status uint8 [P]) of one kind of map on a lattice of the given spacing; seeded by its arguments."""
    C, P = len(lattice), _nodes(lattice)
    rng = np.random.default_rng([C, P, lattice[-1], KINDS.index(kind), int(spacing * 4)])
    idx = np.indices(lattice).reshape(C, P)[::-1].astype(np.float64)  # component 0 = x
    s = idx * spacing
    st = np.zeros(P, np.uint8)
    if kind == "linear":
        A = np.eye(C) + 0.4 * rng.normal(size=(C, C))
        pos = A @ s + rng.normal(size=(C, 1))
    elif kind == "collapsed":
        pos = np.broadcast_to(rng.normal(size=(C, 1)), (C, P))
    else:
        k = rng.uniform(0.3, 1.1, size=(C, C))
        ph = rng.uniform(0, 6.28, size=(C, 1))
        pos = s + 0.8 * np.sin(np.einsum("rc,cp->rp", k, s) + ph)
        if kind in ("noise", "status"):
            pos = pos + 0.3 * rng.normal(size=(C, P))
    pos = np.ascontiguousarray(pos, np.float32)
    if kind == "status":
        dead = rng.permutation(P)[:max(1, P // 4)]
        st[dead] = np.where(rng.random(dead.size) < 0.5, ref.OUT, 2).astype(np.uint8)  # OUT / NONFINITE
        junk = np.array([np.nan, np.inf, -np.inf], np.float32)
        pos[:, dead] = junk[rng.integers(0, 3, size=(C, dead.size))]
        alive = np.flatnonzero(st == 0)
        pos[rng.integers(0, C), alive[rng.integers(0, alive.size)]] = np.nan  # one ALIVE node carries a NaN
    pos.setflags(write=False)
    st.setflags(write=False)
    return pos, st


@functools.lru_cache(maxsize=None)
def valid_mask(lattice):
    rng = np.random.default_rng([7, _nodes(lattice)])
    v = (rng.random(_nodes(lattice)) < 0.8).astype(np.uint8)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(lattice, kind, cfg):
    spacing, T, masked, acc = cfg
    pos, st = make_map(lattice, kind, spacing)
    r = ref.ftle(pos, st, lattice, spacing, T, valid=valid_mask(lattice) if masked else None, accept_out=acc)
    for a in r.values():
        a.setflags(write=False)
    return r


def run(lattice, kind, cfg, **kw):
    from opticalflowscivis_amd import ops
    spacing, T, masked, acc = cfg
    pos, st = make_map(lattice, kind, spacing)
    valid = torch.from_numpy(valid_mask(lattice).copy()).cuda() if masked else None
    return ops.ftle(torch.from_numpy(pos.copy()).cuda(), torch.from_numpy(st.copy()).cuda(), lattice, spacing, T,
                    valid=valid, accept_out=acc, **kw)


def check(got, want, T, tag):
    cls = got["cls"].cpu().numpy()
    np.testing.assert_array_equal(cls, want["cls"], err_msg=str(tag))
    if "cg" in got:
        np.testing.assert_array_equal(got["cg"].cpu().numpy().view(np.uint32), want["cg"].view(np.uint32), err_msg=str(tag))
    e = got["ftle"].cpu().numpy()
    ok = cls == ref.OK
    assert np.isnan(e[~ok]).all(), tag
    a, b = e[ok].astype(np.float64), want["ftle"][ok].astype(np.float64)
    err = np.abs(a - b)
    bound = 2.0 ** -23 * np.abs(b) + 1e-12 / abs(T)
    print("%s: %d ok nodes, max |ftle - ref| %.3g, max err / bound %.3g" % (
        tag, int(ok.sum()), err.max() if err.size else 0.0, (err / bound).max() if err.size else 0.0))
    assert (err <= bound).all(), (tag, float(err.max()))


def check_summary(got, tag):
    s = got["summary"].cpu().numpy()
    cls = got["cls"].cpu().numpy()
    e = got["ftle"].cpu().numpy()
    assert s.shape == (9,) and s[:5].tolist() == [float((cls == k).sum()) for k in range(5)], tag
    x = e[cls == ref.OK].astype(np.float64)
    if x.size:
        assert s[7] == x.min() and s[8] == x.max(), tag
    else:
        assert s[7] == np.inf and s[8] == -np.inf, tag
    n = max(1, x.size)
    assert abs(s[5] - x.sum()) <= n * 2.0 ** -52 * np.abs(x).sum(), tag
    assert abs(s[6] - (x * x).sum()) <= n * 2.0 ** -52 * (x * x).sum(), tag


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lattice", LATTICES, ids=lambda l: "x".join(map(str, l)))
def test_against_the_restatement(lattice, kind):
    for cfg in CONFIGS:
        got = run(lattice, kind, cfg, with_cg=True)
        assert got["ftle"].shape == lattice and got["cls"].dtype == torch.uint8
        assert got["cg"].shape == (len(lattice) * (len(lattice) + 1) // 2,) + lattice
        check(got, reference(lattice, kind, cfg), cfg[1], (lattice, kind, cfg))
        check_summary(got, (lattice, kind, cfg))
    want = reference(lattice, kind, CONFIGS[0])
    if kind == "collapsed":
        assert (want["cls"] == ref.COLLAPSED).all()
    elif kind != "status":
        assert (want["cls"] == ref.OK).all()


@pytest.mark.parametrize("lattice", [l for l in LATTICES if _nodes(l) >= 35], ids=lambda l: "x".join(map(str, l)))
def test_the_status_kind_tests_something(lattice):
    """On the restatement alone: every per-axis outcome occurs, and enough nodes keep a value to compare."""
    want = reference(lattice, "status", CONFIGS[0])
    counts = [int((want["kinds"] == k).sum()) for k in (ref.CENTRAL, ref.FORWARD, ref.BACKWARD, ref.NONE)]
    n_ok = int((want["cls"] == ref.OK).sum())
    print(lattice, "central / forward / backward / none:", counts, "ok", n_ok, "of", _nodes(lattice))
    assert min(counts) >= 8 and n_ok >= 20
    assert (want["cls"] == ref.NONFINITE).any() and (want["cls"] == ref.ENDED).any()
    # with the exit points accepted, their NaN and inf values are used and must not leak past the class
    acc = reference(lattice, "status", CONFIGS[2])
    assert (acc["cls"] == ref.NONFINITE).sum() > (want["cls"] == ref.NONFINITE).sum()


def test_grid_stride_loop():
    """More than 2048 * 256 nodes: every workgroup takes a second node per thread, the last ones only some."""
    lattice, cfg = (2, 513, 513), CONFIGS[0]
    assert _nodes(lattice) > 2048 * 256
    got = run(lattice, "noise", cfg, with_cg=True)
    check(got, reference(lattice, "noise", cfg), cfg[1], (lattice, "noise"))
    check_summary(got, lattice)


def test_strided_slice_of_a_recorded_trajectory():
    """pos as a [C,P] slice whose rows are P + 5 apart and start off a 16-byte boundary, read in place."""
    from opticalflowscivis_amd import ops
    sp = (6, 7, 9)
    seeds, lattice, h = ops.lattice_seeds(sp, 2, "cuda")
    P = seeds.shape[1]
    g = torch.Generator().manual_seed(5)
    flows = (0.6 * torch.randn((2, 3) + sp, generator=g)).cuda()
    more = torch.cat([seeds.new_full((3, 3), 1.5), seeds, seeds.new_full((3, 2), 2.5)], 1)
    traj, status, _ = ops.advect(more, flows, method="rk2", record=True)
    pos = traj[-1][:, 3:3 + P]
    assert pos.stride(0) == P + 5 and not pos.is_contiguous() and pos.data_ptr() % 16 != 0
    got = ops.ftle(pos, status[3:3 + P], lattice, h, 2.0, with_cg=True)
    want = ref.ftle(pos.cpu().numpy(), status[3:3 + P].cpu().numpy(), lattice, h, 2.0)
    check(got, want, 2.0, "strided")
    check_summary(got, "strided")
    assert (want["cls"] == ref.OK).sum() >= 100 and (want["cls"] == ref.ENDED).sum() >= 10
    same = ops.ftle(pos.contiguous(), status[3:3 + P].clone(), lattice, h, 2.0, with_cg=True)
    for k in ("ftle", "cg"):
        assert torch.equal(got[k].view(torch.int32), same[k].view(torch.int32)), k
    assert torch.equal(got["cls"], same["cls"]) and torch.equal(got["summary"], same["summary"])


def test_without_summary_and_tensor_and_on_another_stream():
    lattice, cfg = (17, 9, 33), CONFIGS[1]
    full = run(lattice, "status", cfg, with_cg=True)
    bare = run(lattice, "status", cfg, with_cg=False, summary=False)
    assert sorted(bare) == ["cls", "ftle"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = run(lattice, "status", cfg, with_cg=True)
    s.synchronize()
    for r in (bare, other):
        assert torch.equal(r["ftle"].view(torch.int32), full["ftle"].view(torch.int32)) and torch.equal(r["cls"], full["cls"])
    assert torch.equal(other["cg"].view(torch.int32), full["cg"].view(torch.int32))
    assert torch.equal(other["summary"], full["summary"])
    # spacing per axis, in the lattice's order, equals the scalar form
    from opticalflowscivis_amd import ops
    pos, st = make_map(lattice, "noise", 0.5)
    a = ops.ftle(torch.from_numpy(pos.copy()).cuda(), torch.from_numpy(st.copy()).cuda(), lattice, 0.5, 1.0)
    b = ops.ftle(torch.from_numpy(pos.copy()).cuda(), torch.from_numpy(st.copy()).cuda(), lattice, (0.5, 0.5, 0.5), 1.0)
    assert torch.equal(a["ftle"].view(torch.int32), b["ftle"].view(torch.int32))
