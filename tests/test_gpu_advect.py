"""GPU: fs_advect{2,3}d / ops.advect against the fp64 restatement in tests/advect_ref.py, bit for bit: positions as fp32
bit patterns, status and step counts.  No case provokes a fault: every index the kernel forms comes from a finite value
clamped to the grid, and the non-finite cases check exactly that."""
import functools

import numpy as np
import pytest
import torch

import advect_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(2, 2, 2), (1, 5, 9), (5, 6, 7), (4, 5, 16), (8, 8, 8), (3, 3), (5, 7), (9, 12), (1, 8)]
COUNTS = (1, 63, 64, 65, 257)
METHODS = ((ref.EULER, 1), (ref.RK2, 2), (ref.RK4, 3))
KINDS = ("noise", "smooth", "zero", "nonfinite")
KMAX = 3


def _seed(sp, kind, P):
    return 300000 + 1000 * KINDS.index(kind) + 10 * sum(s * (i + 1) for i, s in enumerate(sp)) + P


@functools.lru_cache(maxsize=None)
def _inputs(sp, kind, P):
    """(pos [C,P], flows [KMAX,C,*sp]) as read-only fp32 numpy arrays."""
    C = len(sp)
    S = np.array(sp[::-1], np.float64)  # extents along x, y(, z)
    rng = np.random.default_rng(_seed(sp, kind, P))
    pos = (rng.random((C, P)) * (S - 1)[:, None]).astype(np.float32)  # uniform in the box
    if kind in ("noise", "nonfinite"):
        flows = (0.6 * rng.standard_normal((KMAX, C) + sp)).astype(np.float32)
        for c in range(C):  # along an axis of extent 1 any motion leaves the box at once
            if S[c] == 1:
                flows[:, c] = 0
    elif kind == "smooth":
        ax = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sp], indexing="ij")[::-1]  # x, y(, z)
        flows = np.stack([np.stack([0.7 * np.sin(0.9 * ax[(c + 1) % C] + 0.5 * k + c) * (S[c] > 1) for c in range(C)])
                          for k in range(KMAX)]).astype(np.float32)
    else:
        flows = np.zeros((KMAX, C) + sp, np.float32)
    if kind == "nonfinite":
        n = flows[0, 0].size
        flat = flows.reshape(KMAX, C, n)
        for k in range(KMAX):  # a NaN, a +inf and a -inf in every step's field
            for j, v in enumerate((np.nan, np.inf, -np.inf)):
                flat[k, (k + j) % C, (7 * k + 3 * j + 1) % n] = v
        # particle 0 sits exactly on element (0, .., 0), whose +x neighbour is NaN: a corner of weight 0
        flat[0, :, 0] = 0.25
        flat[0, 0, 1] = np.nan
        pos[:, 0] = 0
        special = [np.nan, np.inf, -0.5, None, "far"]  # per particle 1..: a bad x, x = W (outside), the far border
        for i, v in enumerate(special):
            if 1 + i < P:
                if v == "far":
                    pos[:, 1 + i] = (S - 1).astype(np.float32)
                else:
                    pos[0, 1 + i] = S[0] if v is None else v
    pos.setflags(write=False)
    flows.setflags(write=False)
    return pos, flows


@functools.lru_cache(maxsize=None)
def _expected(sp, kind, P, K, method, substeps):
    pos, flows = _inputs(sp, kind, P)
    out = ref.advect(pos, flows[:K], method=method, substeps=substeps)
    for a in out:
        a.setflags(write=False)
    return out


def _dev(a):
    return torch.tensor(a, device=DEV)  # (a copy: the cached inputs are read-only)


def _bits(t):
    return (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def _same(got, want, what=""):
    traj, st, n = got
    np.testing.assert_array_equal(_bits(traj), _bits(want[0]), err_msg="positions " + what)
    np.testing.assert_array_equal(st.cpu().numpy(), want[1], err_msg="status " + what)
    if n is not None:
        np.testing.assert_array_equal(n.cpu().numpy(), want[2], err_msg="steps " + what)


def _run(sp, kind, P, K, method, substeps, **kw):
    pos, flows = _inputs(sp, kind, P)
    from opticalflowscivis_amd import ops
    traj, st, n = ops.advect(_dev(pos), _dev(flows[:K]), method=method,
                             substeps=substeps, record=True, **kw)
    assert traj.shape == (K + 1, len(sp), P) and st.dtype == torch.uint8 and st.shape == (P,)
    np.testing.assert_array_equal(_bits(traj[0]), _bits(pos))
    return traj[1:], st, n


@pytest.mark.parametrize("sp", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_kind_and_method_bitwise(sp):
    for kind in KINDS:
        for method, S in METHODS:
            want = _expected(sp, kind, 257, KMAX, method, S)
            if kind == "noise":  # the comparison is not empty: both classes occur (on the restatement alone)
                assert (want[1] == ref.ALIVE).sum() >= 8 and (want[1] == ref.OUT).sum() >= 8, (sp, method, want[1])
            if kind == "zero":
                assert (want[1] == ref.ALIVE).all() and (want[2] == KMAX).all()
            if kind == "nonfinite":
                assert want[1][0] == ref.NONFINITE and want[2][0] == 0  # the NaN corner of weight 0
                assert want[1][1:4].tolist() == [ref.NONFINITE, ref.NONFINITE, ref.OUT] and want[1][4] == ref.OUT
                assert (want[1] == ref.NONFINITE).sum() >= 3
            _same(_run(sp, kind, 257, KMAX, method, S), want, "%s %s %s" % (sp, kind, method))


@pytest.mark.parametrize("sp", [(5, 6, 7), (9, 12)], ids=lambda s: "x".join(map(str, s)))
def test_particle_and_step_counts_bitwise(sp):
    for P in COUNTS:
        for K in (1, 3):
            for method, S in METHODS:
                for kind in ("noise", "nonfinite"):
                    _same(_run(sp, kind, P, K, method, S), _expected(sp, kind, P, K, method, S),
                          "%s P=%d K=%d %s %s" % (sp, P, K, method, kind))


@pytest.mark.parametrize("sp", [(4, 5, 16), (5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_one_launch_equals_single_steps_and_repeats(sp):
    from opticalflowscivis_amd import ops
    P = 257
    for kind in ("noise", "nonfinite"):
        pos, flows = _inputs(sp, kind, P)
        fl = _dev(flows)
        for method, S in METHODS:
            want = _expected(sp, kind, P, KMAX, method, S)
            p, st, n = _dev(pos), None, None
            for k in range(KMAX):
                p, st, n = ops.advect(p, fl[k:k + 1], st, n, method, S)
                np.testing.assert_array_equal(_bits(p), _bits(want[0][k]))
            _same((p, st, n), (want[0][-1], want[1], want[2]), "chained")
            a = _run(sp, kind, P, KMAX, method, S)
            b = _run(sp, kind, P, KMAX, method, S)
            _same(a, want)
            _same(b, want)
            # without record the last position alone comes back; steps=False counts nothing
            last, st2, n2 = ops.advect(_dev(pos), fl, None, False, method, S)
            assert n2 is None and last.shape == (len(sp), P)
            _same((last, st2, None), (want[0][-1], want[1], want[2]), "unrecorded")


def _raw(sp, flows, fss, pos_ptr, pcs, P, traj_ptr, tss, tcs, status, steps, method=0, substeps=1, scale=1.0, K=None):
    from opticalflowscivis_amd import _lib
    nd = len(sp)
    fn = getattr(_lib.lib(), "fs_advect%dd" % nd)
    return fn(flows.data_ptr() if isinstance(flows, torch.Tensor) else flows, flows.shape[0] if K is None else K, nd,
              *sp, fss, pos_ptr, pcs, P, traj_ptr, tss, tcs,
              status.data_ptr() if isinstance(status, torch.Tensor) else status,
              None if steps is None else steps.data_ptr(), method, substeps, scale,
              torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("sp", [(5, 6, 7), (9, 12)], ids=lambda s: "x".join(map(str, s)))
def test_strides_aliasing_and_ended_particles(sp):
    from opticalflowscivis_amd import ops
    C, P, K = len(sp), 65, KMAX
    pos, flows = _inputs(sp, "noise", P)
    plane = int(np.prod(sp))
    want = _expected(sp, "noise", P, K, ref.RK2, 2)
    # strided operands through the op: every other field of a larger stack, rows of a wider position array
    big = torch.full((2 * K, C) + sp, float("nan"), device=DEV)
    big[::2] = _dev(flows)
    wide = torch.full((C, P + 5), float("nan"), device=DEV)
    wide[:, :P] = _dev(pos)
    assert not big[::2].is_contiguous() and not wide[:, :P].is_contiguous()
    traj, st, n = ops.advect(wide[:, :P], big[::2], method="rk2", substeps=2, record=True)
    _same((traj[1:], st, n), want, "strided")
    # the C-ABI directly: a trajectory with padded step and component strides whose last slot is pos_in's memory
    tcs, tss = P + 3, C * (P + 3) + 7
    buf = torch.full((K * tss,), -7.0, device=DEV)
    slot = lambda k: buf[k * tss:k * tss + C * tcs].view(C, tcs)
    slot(K - 1)[:, :P] = _dev(pos)
    st = torch.zeros(P, dtype=torch.uint8, device=DEV)
    n = torch.zeros(P, dtype=torch.int32, device=DEV)
    fl = big[::2]
    rc = _raw(sp, fl, fl.stride(0), slot(K - 1).data_ptr(), tcs, P, buf.data_ptr(), tss, tcs, st, n, 1, 2)
    assert rc == 0
    got = torch.stack([slot(k)[:, :P] for k in range(K)])
    _same((got, st, n), want, "aliased")
    pad = torch.ones(K * tss, dtype=torch.bool, device=DEV)
    for k in range(K):
        for c in range(C):
            pad[k * tss + c * tcs:k * tss + c * tcs + P] = False
    assert bool((buf[pad] == -7.0).all())  # nothing written between the rows
    # steps = NULL, and a status that is not ALIVE on entry: passed through, the position copied to every slot
    st_in = (np.arange(P) % 3).astype(np.uint8)
    n_in = np.arange(P, dtype=np.int32)
    want2 = ref.advect(pos, flows, st_in, n_in, ref.RK4, 3)
    ended = st_in != ref.ALIVE
    assert (want2[1][ended] == st_in[ended]).all() and (want2[2][ended] == n_in[ended]).all()
    for k in range(K):
        np.testing.assert_array_equal(_bits(want2[0][k][:, ended]), _bits(pos[:, ended]))
    p = _dev(pos)
    out = ops.advect(p, _dev(flows), _dev(st_in), _dev(n_in),
                     "rk4", 3, record=True)
    _same((out[0][1:], out[1], out[2]), want2, "ended on entry")
    traj3 = torch.empty(K, C, P, device=DEV)
    st3 = _dev(st_in)
    flc = _dev(flows)
    assert _raw(sp, flc, C * plane, p.data_ptr(), P, P, traj3.data_ptr(), C * P, P, st3, None, 2, 3) == 0
    _same((traj3, st3, None), want2, "steps NULL")
    # scale: -1 through the negated fields is the same chain of operations with both signs flipped
    want4 = ref.advect(pos, -flows, method=ref.EULER, scale=-1.0)
    out = ops.advect(p, -flc, scale=-1.0, record=True)
    _same((out[0][1:], out[1], out[2]), want4, "scale")
    _same((out[0][1:], out[1], out[2]), _expected(sp, "noise", P, K, ref.EULER, 1), "scale, mirrored")


def test_errors_come_back_without_a_launch():
    sp, P = (4, 4, 4), 8
    fl = torch.zeros(2, 3, 4, 4, 4, device=DEV)
    pos = torch.ones(3, P, device=DEV)
    traj = torch.full((2, 3, P), -7.0, device=DEV)
    st = torch.zeros(P, dtype=torch.uint8, device=DEV)
    n = torch.zeros(P, dtype=torch.int32, device=DEV)
    call = lambda flows=fl, K=2, fss=192, pos_ptr=pos.data_ptr(), pcs=P, Pn=P, traj_ptr=traj.data_ptr(), tss=3 * P, \
        tcs=P, status=st, m=0, S=1, scale=1.0, shape=sp: _raw(shape, flows, fss, pos_ptr, pcs, Pn, traj_ptr, tss, tcs,
                                                              status, n, m, S, scale, K=K)
    assert [call(flows=None), call(pos_ptr=None), call(traj_ptr=None), call(status=None)] == [1] * 4
    assert [call(K=0), call(Pn=0), call(shape=(4, 0, 4)), call(fss=191), call(pcs=P - 1), call(tcs=P - 1),
            call(tss=P - 1)] == [2] * 7
    assert [call(S=0), call(m=3), call(scale=float("nan")), call(scale=float("-inf"))] == [3] * 4
    torch.cuda.synchronize()
    assert bool((traj == -7.0).all()) and int(st.sum()) == 0 and int(n.sum()) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((traj == 1.0).all()) and int(n.sum()) == 2 * P


def test_dense_map_of_a_known_motion():
    """Dense seeds through the ground-truth steps of the integer-velocity droplet: several workgroups, the grid-seed
    layout, and the composed map equal to gt(0, 5) on the sphere (tests/test_advect_cpu.py has the reasoning)."""
    from opticalflowscivis_amd import ops
    from opticalflowscivis_amd.data import synthetic
    T, S = 6, 32
    frames, gt = synthetic.droplet3d_motion(T, S, seed=3, v=(1, -2, 1), device=DEV)
    flows = torch.stack([gt(t, t + 1)[0] for t in range(T - 1)])
    seeds = ops.grid_seeds((S, S, S), 1, 0, DEV)
    pos, st, n = ops.advect(seeds, flows)
    disp = (pos - seeds).view(3, S, S, S)
    inside = frames[0] > 0
    assert int(inside.sum()) >= 100
    assert torch.equal(disp[:, inside], gt(0, T - 1)[0][:, inside])
    want = ref.advect(seeds.cpu().numpy(), flows.cpu().numpy())
    _same((pos, st, n), (want[0][-1], want[1], want[2]), "dense")
