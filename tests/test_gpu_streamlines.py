"""GPU: fs_streamlines{2,3}d / ops.streamlines against the fp64 restatement in tests/streamline_ref.py, bit for bit:
verts[0 .. length] as fp32 bit patterns, length, end and hit of every line; nothing is left out.  No case provokes a
fault: every index the kernel forms comes from a finite value clamped to the grid, `step` is checked before it selects a
field, the non-finite and out-of-range inputs check exactly that, and the argument errors come back before anything is
launched."""
import functools

import numpy as np
import pytest
import torch

import streamline_fields as fields
import streamline_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(5, 6, 7), (3, 4, 70), (9, 9, 9), (7, 9), (5, 130)]
KMAX, STACK = 3, 5
# (S, M, method, h, vmin): every S of {1, 63, 65, 300}, every M of {1, 40, 300} and every method occurs, the longest lines
# (M = 300) with each method; 63 / 65 lines are one lane short of a wave and one lane into the second
COMBOS = ((1, 1, ref.EULER, 0.5, 0.0), (63, 40, ref.RK2, 0.37, 0.0), (65, 300, ref.RK4, 0.5, 0.0),
          (300, 40, ref.RK4, 1.0, 0.3), (300, 1, ref.RK2, 0.5, 0.0), (65, 300, ref.EULER, 0.25, 0.0),
          (63, 300, ref.RK2, 0.5, 0.3), (1, 40, ref.RK4, 0.5, 0.0))
IDS = lambda s: "x".join(map(str, s))


def _seed(sp, kind):
    return 810000 + 1000 * fields.KINDS.index(kind) + 10 * sum(s * (i + 1) for i, s in enumerate(sp))


def _dev(a):
    return torch.tensor(a, device=DEV)  # (a copy: the cached inputs are read-only)


def _capture_planes(flows):
    """uint8 [K, *sp]: 1 at the cell of every critical point ops.critical_points finds in `flows` (a device tensor)."""
    from opticalflowscivis_amd import ops
    r = ops.critical_points(flows)
    K = flows.shape[0]
    cap = torch.zeros((K, flows[0, 0].numel()), dtype=torch.uint8, device=flows.device)
    step = torch.repeat_interleave(torch.arange(K, device=flows.device), r["offsets"][1:] - r["offsets"][:-1])
    cap[step, r["cell"].to(torch.int64)] = 1
    return cap.view((K,) + tuple(flows.shape[2:])).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(sp, kind):
    """(stack [STACK,C,*sp] whose every other field is used, capture uint8 [KMAX,*sp]) as read-only numpy arrays."""
    stack = fields.stack_of(sp, kind, STACK, _seed(sp, kind))
    cap = _capture_planes(_dev(stack)[::2])
    stack.setflags(write=False)
    cap.setflags(write=False)
    return stack, cap


@functools.lru_cache(maxsize=None)
def _lines(sp, S):
    out = fields.lines_of(sp, KMAX, S, 5 * S + sum(sp))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(sp, kind, combo, with_home=True, with_capture=True):
    S, M, method, h, vmin = combo
    stack, cap = _inputs(sp, kind)
    seeds, step, sign, home = _lines(sp, S)
    out = ref.streamlines(stack[::2], seeds.T, step, sign, home if with_home else None, cap if with_capture else None, M, h,
                          vmin, method)
    for a in out:
        a.setflags(write=False)
    return out


def _run(sp, kind, combo, with_home=True, with_capture=True):
    from opticalflowscivis_amd import ops
    S, M, method, h, vmin = combo
    stack, cap = _inputs(sp, kind)
    seeds, step, sign, home = _lines(sp, S)
    flows = _dev(stack)[::2]  # a view: the step stride is twice the field
    assert not flows.is_contiguous()
    r = ops.streamlines(flows, _dev(seeds), _dev(step), _dev(sign), _dev(home) if with_home else None,
                        _dev(cap) if with_capture else None, M, h, vmin, method)
    assert r["verts"].shape == (M + 1, len(sp), S) and r["verts"].dtype == torch.float32
    assert r["length"].dtype == torch.int32 and r["end"].dtype == torch.uint8 and r["hit"].dtype == torch.int32
    return r


def _same(got, want, what=""):
    verts, length, end, hit = want
    np.testing.assert_array_equal(got["length"].cpu().numpy(), length, err_msg="length " + what)
    np.testing.assert_array_equal(got["end"].cpu().numpy(), end, err_msg="end " + what)
    np.testing.assert_array_equal(got["hit"].cpu().numpy(), hit, err_msg="hit " + what)
    gv = got["verts"].cpu().numpy()
    defined = np.arange(verts.shape[0])[:, None, None] <= length[None, None, :]  # slots 0 .. length of every line
    defined = np.broadcast_to(defined, verts.shape)
    np.testing.assert_array_equal(gv.view(np.uint32)[defined], verts.view(np.uint32)[defined], err_msg="verts " + what)


@pytest.mark.parametrize("kind", fields.KINDS)
@pytest.mark.parametrize("sp", SHAPES, ids=IDS)
def test_every_shape_field_and_method_bitwise(sp, kind):
    for combo in COMBOS:
        want = _expected(sp, kind, combo)
        _same(_run(sp, kind, combo), want, "%s %s %s" % (sp, kind, combo))
        if kind == "ball" and combo[0] >= 63:
            assert (want[2] == ref.STAGNANT).any()
        if kind == "nonfinite" and combo[0] >= 63 and combo[1] >= 40:
            assert (want[2] == ref.NONFINITE).sum() >= 2


@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)], ids=IDS)
def test_optional_operands_and_single_fields(sp):
    from opticalflowscivis_amd import ops
    combo = (65, 40, ref.RK4, 0.5, 0.0)
    for with_home, with_capture in ((False, True), (True, False), (False, False)):
        want = _expected(sp, "noise", combo, with_home, with_capture)
        a = _run(sp, "noise", combo, with_home, with_capture)
        _same(a, want, "home %s capture %s" % (with_home, with_capture))
        if not with_capture:
            assert (want[3] == -1).all() and not (want[2] == ref.CAPTURED).any()
    # two calls give identical bits where the lines are defined, and a line's result does not depend on its neighbours:
    # the lines of one step alone, on that field alone (K = 1), equal their rows of the full call
    stack, cap = _inputs(sp, "noise")
    seeds, step, sign, home = _lines(sp, 65)
    want = _expected(sp, "noise", combo)
    for k in range(KMAX):
        sel = np.nonzero(step == k)[0]
        r = ops.streamlines(_dev(stack)[2 * k:2 * k + 1], _dev(seeds[sel]), torch.zeros(len(sel), dtype=torch.int32, device=DEV),
                            _dev(sign[sel]), _dev(home[sel]), _dev(cap[k:k + 1]), 40, 0.5, 0.0, "rk4")
        _same(r, (want[0][:, :, sel], want[1][sel], want[2][sel], want[3][sel]), "single field %d" % k)


def test_every_end_code_occurs():
    """On the restatement alone: the cases above hold lines of every end code, and plenty of the common ones."""
    count = np.zeros(6, np.int64)
    for sp, kind, combo in (((5, 6, 7), "noise", COMBOS[2]), ((7, 9), "noise", COMBOS[4]), ((7, 9), "ball", COMBOS[3]), ((9, 9, 9), "nonfinite", COMBOS[2]),
                            ((5, 130), "smooth", COMBOS[5]), ((3, 4, 70), "smooth", COMBOS[6])):
        count += np.bincount(_expected(sp, kind, combo)[2], minlength=6)
    print(dict(zip(ref.END_NAMES, count.tolist())))
    assert (count > 0).all(), count
    assert count[ref.OUT] >= 20 and count[ref.CAPTURED] >= 20 and count[ref.STAGNANT] >= 8 and count[ref.INVALID] >= 8


@pytest.mark.parametrize("nd", [2, 3])
def test_the_real_chain_equals_the_restatement(nd):
    """critical_points -> seed_lines -> streamlines on a band-limited field, as skeleton_series chains them."""
    from opticalflowscivis_amd import ops, skeleton
    sp = (17, 19) if nd == 2 else (10, 11, 12)
    flows = fields.stack_of(sp, "smooth", 2, 77)
    fd = _dev(flows)
    r = ops.critical_points(fd)
    off = r["offsets"].cpu().numpy()
    cap = torch.zeros((2, int(np.prod(sp))), dtype=torch.uint8, device=DEV)
    cols = []
    for k in range(2):
        tab = {c: r[c][off[k]:off[k + 1]].cpu().numpy() for c in ("cell", "pos", "jac", "cls")}
        cap[k, torch.from_numpy(tab["cell"].astype(np.int64)).to(DEV)] = 1
        v0 = fd[k].reshape(nd, -1)[:, torch.from_numpy(tab["cell"].astype(np.int64)).to(DEV)].t().cpu().numpy()
        sd = skeleton.seed_lines(tab, nd, 1.0, 1.0, eps=0.5, surface_seeds=5 if nd == 3 else 0, shape=sp, node_values=v0)
        sd["step"] = np.full(len(sd["sign"]), k, np.int32)
        cols.append(sd)
    sd = {n: np.concatenate([c[n] for c in cols]) for n in cols[0]}
    S = len(sd["sign"])
    assert S >= 8, S  # (a few saddles in each step)
    got = ops.streamlines(fd, _dev(sd["seeds"]), _dev(sd["step"]), _dev(sd["sign"]), _dev(sd["home"]), cap.view((2,) + sp),
                          120, 0.5, 0.0, "rk4")
    want = ref.streamlines(flows, sd["seeds"].T, sd["step"], sd["sign"], sd["home"], cap.cpu().numpy(), 120, 0.5, 0.0, ref.RK4)
    _same(got, want, "chain %d-D" % nd)
    assert (want[1] > 0).sum() >= S // 2  # (a saddle within eps of the border has seeds outside: OUT with length 0)
    assert (want[2] == ref.CAPTURED).sum() >= 8 and (want[2] == ref.OUT).sum() >= 8


def test_errors_come_back_without_a_launch():
    from opticalflowscivis_amd import _lib, ops
    sp = (4, 4, 4)
    S, M = 5, 3
    fl = torch.ones(2, 3, 4, 4, 4, device=DEV)
    seeds = torch.full((3, S), 1.5, dtype=torch.float64, device=DEV)
    step = torch.zeros(S, dtype=torch.int32, device=DEV)
    sign = torch.ones(S, dtype=torch.int8, device=DEV)
    cap = torch.zeros((2, 64), dtype=torch.uint8, device=DEV)
    verts = torch.full((M + 1, 3, S), -7.0, device=DEV)
    length = torch.full((S,), 99, dtype=torch.int32, device=DEV)
    end = torch.full((S,), 99, dtype=torch.uint8, device=DEV)
    hit = torch.full((S,), 99, dtype=torch.int32, device=DEV)
    fn = _lib.lib().fs_streamlines3d

    def call(flows=fl.data_ptr(), K=2, C=3, shape=sp, fss=192, sd=seeds.data_ptr(), scs=S, n=S, st=step.data_ptr(),
             sg=sign.data_ptr(), css=64, m=M, h=0.5, vmin=0.0, method=2, v=verts.data_ptr(), vss=3 * S, vcs=S,
             ln=length.data_ptr(), e=end.data_ptr(), ht=hit.data_ptr()):
        return fn(flows, K, C, *shape, fss, sd, scs, n, st, sg, None, cap.data_ptr(), css, m, h, vmin, method, v, vss, vcs,
                  ln, e, ht, torch.cuda.current_stream().cuda_stream)

    assert [call(flows=None), call(sd=None), call(st=None), call(sg=None), call(v=None), call(ln=None), call(e=None),
            call(ht=None)] == [1] * 8
    assert [call(K=0), call(n=0), call(C=2), call(shape=(4, 1, 4)), call(shape=(1, 4, 4)), call(fss=191), call(scs=S - 1),
            call(css=63), call(vcs=S - 1), call(vss=3 * S - 1)] == [2] * 10
    assert [call(m=0), call(h=0.0), call(h=-1.0), call(h=float("inf")), call(h=float("nan")), call(vmin=-0.1),
            call(vmin=float("nan")), call(vmin=float("inf")), call(method=3), call(method=-1)] == [3] * 10
    assert _lib.lib().fs_streamlines2d(fl.data_ptr(), 2, 3, 4, 4, 192, seeds.data_ptr(), S, S, step.data_ptr(), sign.data_ptr(),
                                       None, None, 0, M, 0.5, 0.0, 2, verts.data_ptr(), 3 * S, S, length.data_ptr(),
                                       end.data_ptr(), hit.data_ptr(), None) == 2  # (C = 3 in 2-D)
    torch.cuda.synchronize()
    assert bool((verts == -7.0).all()) and bool((length == 99).all()) and bool((end == 99).all()) and bool((hit == 99).all())
    # the op refuses on the host what the library would refuse, and what it cannot see
    ok = dict(flows=fl, seeds=seeds.t().contiguous(), step=step, sign=sign)
    for bad in (dict(max_steps=0), dict(max_steps=2.5), dict(h=0.0), dict(h=float("nan")), dict(vmin=-1.0), dict(method="rk3"),
                dict(seeds=seeds), dict(seeds=seeds.t().float()), dict(seeds=seeds.t().cpu()), dict(step=step.long()),
                dict(sign=sign[:-1]), dict(home=step.long()), dict(capture=cap), dict(flows=fl[:, :, :1]),
                dict(flows=fl.cpu()), dict(capture=cap.view(2, 4, 4, 4).cpu())):
        with pytest.raises(ValueError):
            ops.streamlines(**dict(ok, **bad))
    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    # a constant field along (1,1,1) / sqrt(3): the lines run straight to the border, 2.5 elements away
    assert bool((length == M).all()) and bool((end == 0).all()) and bool((hit == -1).all())
    want = 1.5 + 0.5 * np.arange(M + 1) / np.sqrt(3.0)
    assert np.allclose(verts.cpu().numpy(), want[:, None, None], atol=1e-6)
    assert ops.streamline_end_names == ref.END_NAMES
    nbytes, flops = ops.streamlines_cost(sp, S, M, "rk4")
    assert nbytes > 0 and flops > 0 and ops.streamlines_cost(sp, S, M, "euler")[1] < flops
