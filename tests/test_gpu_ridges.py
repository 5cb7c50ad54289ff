"""GPU: ops.ridge_nodes / ops.ridge_surfaces (fs_ridge_nodes3d, fs_ridge_count3d, fs_ridge_emit3d) against the numpy
restatement tests/ridge_ref.py, bit for bit: the class bytes, all five operand planes, the per-row counts, the edge
masks, vertices and faces.  The per-vertex values may be formed with fused multiply-adds, so they go to a tolerance
against the restatement's fp64 column.  A value is wa + t (wb - wa) with the same fp32 t in [0, 1]: in fp32 the
difference, the product and the sum each round once (a fused form drops one rounding), each by at most 2^-24 of a
magnitude that |wa| + |wb| bounds, so the error is below 3 * 2^-24 (|wa| + |wb|); the test allows 4 * 2^-24 of it and
prints what the kernel and the restatement's own fp32 column use of that (0.05 to 0.5 of it)."""
import ctypes

import numpy as np
import pytest
import torch

import ridge_fields as RF
import ridge_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def build(kind, shape):
    if kind == "noise":
        return RF.noise(shape, seed=3)[0], 0.0, -np.inf
    if kind == "nan":
        return RF.noise_nan(shape, seed=4, n=4)[0], 0.0, -np.inf
    if kind == "plane":
        return RF.plane(shape, c=shape[2] - 3.75)[0], 0.25, -np.inf  # (lam = -2 / h_x^2 >= -0.5 for the spacings used)
    if kind == "shell":  # a Gaussian sphere shell that fits the shape
        x, y, z = RF._grid(shape)
        c = (shape[2] / 2 + 0.4, shape[1] / 2 - 0.4, shape[0] / 2 + 0.2)
        r = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        rad = 0.5 * min(shape) - 1.8
        return np.exp(-(r - rad) ** 2 / (2 * 1.0 ** 2)).astype(np.float32), 0.05, 0.4
    raise ValueError(kind)


def check(vols, spacing, strength, fmin, valley=False):
    """vols: numpy [K,D,H,W] or a CUDA tensor view (for strides)"""
    from opticalflowscivis_amd import ops
    t = vols if isinstance(vols, torch.Tensor) else torch.from_numpy(vols).cuda()
    host = t.cpu().numpy()
    K, D, H, W = host.shape
    res = ops.ridge_surfaces(t, spacing, strength, fmin, valley)
    ops.ridge_surfaces_check(res)
    assert int(res["status"]) == 0
    hs = (spacing,) * 3 if np.isscalar(spacing) else tuple(spacing)
    xyz = hs[::-1]
    vo, fo = res["vertex_offsets"].cpu().numpy(), res["face_offsets"].cpu().numpy()
    got_ops, got_cls = res["operands"].cpu().numpy(), res["cls"].cpu().numpy()
    ws, _ = ops.ridge_count(res["operands"], res["cls"])
    rows = ws[:16 * K * D * H].view(torch.int32).view(4, K, D * H).cpu().numpy()
    mask = ws[16 * K * D * H:].view(K, D, H, W).cpu().numpy()
    out = []
    for k in range(K):
        want = R.ridges(host[k], xyz, strength, fmin, valley)
        assert np.array_equal(got_cls[k], want["cls"]), (k, np.argwhere(got_cls[k] != want["cls"])[:5])
        assert np.array_equal(_bits(got_ops[k]), _bits(want["operands"])), k
        assert np.array_equal(rows[:, k].T, want["rows"]), k
        assert np.array_equal(mask[k], want["mask"]), k
        v = res["vertices"][vo[k]:vo[k + 1]].cpu().numpy()
        f = res["faces"][fo[k]:fo[k + 1]].cpu().numpy()
        assert v.shape == want["vertices"].shape and f.shape == want["faces"].shape, (k, v.shape, f.shape)
        assert np.array_equal(_bits(v), _bits(want["vertices"])), k
        assert np.array_equal(f, want["faces"]), k
        counts = res["counts"][k].cpu().numpy()
        assert counts.tolist() == [len(v), len(f), want["twisted"], want["tets"]], (counts, want["twisted"], want["tets"])
        assert res["classes"][k].cpu().numpy().tolist() == np.bincount(want["cls"].reshape(-1), minlength=5).tolist()
        if len(v):
            vals = res["values"][vo[k]:vo[k + 1]].cpu().numpy().astype(np.float64)
            f64 = want["values64"]
            fneg = -host[k] if valley else host[k]
            z, y, x = np.unravel_index(want["owner"], (D, H, W))
            off = np.asarray(R.EDGE_OFFSETS)[want["edge"]]
            ends = []
            for w in (fneg, want["operands"][4]):
                ends.append(np.abs(w[z, y, x]).astype(np.float64) + np.abs(w[z + off[:, 0], y + off[:, 1], x + off[:, 2]]))
            tol = 4 * 2.0 ** -24 * np.stack(ends, 1)
            print("values: kernel %.3g, restated fp32 %.3g of the tolerance" % (
                (np.abs(vals - f64) / np.maximum(tol, 1e-300)).max(),
                (np.abs(want["values32"].astype(np.float64) - f64) / np.maximum(tol, 1e-300)).max()))
            assert (np.abs(vals - f64) <= tol).all()
        out.append(want)
    return res, out


CASES = [((5, 6, 7), 1.0), ((9, 12, 67), (1.0, 0.5, 2.0)), ((4, 5, 130), 0.25)]


@pytest.mark.parametrize("shape,spacing", CASES, ids=["5x6x7", "9x12x67", "4x5x130"])
@pytest.mark.parametrize("kind", ["noise", "nan", "plane", "shell"])
def test_against_the_restatement(shape, spacing, kind):
    f, strength, fmin = build(kind, shape)
    g, _, _ = build("noise" if kind != "noise" else "nan", shape)
    res, want = check(np.stack([f, g]), spacing, strength, fmin)
    if kind == "noise":
        assert want[0]["twisted"] > 0 and len(want[0]["faces"]) > 0  # both branches
    if kind == "plane":
        assert want[0]["twisted"] == 0 and len(want[0]["faces"]) > 0


def test_two_steps_with_a_stride_above_the_volume():
    stack = torch.from_numpy(np.stack([RF.noise((5, 6, 70), seed=s)[0] for s in range(4)])).cuda()
    view = stack[::2]
    assert view.stride(0) == 2 * 5 * 6 * 70
    check(view, 1.0, 0.0, -np.inf)
    check(stack[:, :, :, :67][1:3], 1.0, 0.0, -np.inf)  # rows that are not contiguous: copied, same answer


@pytest.mark.parametrize("shape", [(3, 6, 70), (6, 3, 70), (6, 70, 3)], ids=["D3", "H3", "W3"])
def test_a_single_interior_layer_has_vertices_and_no_tetrahedron(shape):
    f = RF.noise(shape, seed=8)[0]
    res, want = check(f[None], 1.0, 0.0, -np.inf)
    assert want[0]["tets"] == 0 and len(want[0]["faces"]) == 0 and len(want[0]["vertices"]) > 0


def test_extent_two_is_all_border():
    from opticalflowscivis_amd import ops
    res = ops.ridge_surfaces(torch.randn(1, 2, 5, 6, device="cuda"))
    assert res["vertices"].shape == (0, 3) and res["faces"].shape == (0, 3) and int(res["status"]) == 0
    assert res["classes"].cpu().tolist() == [[60, 0, 0, 0, 0]] and bool(torch.isnan(res["operands"]).all())


def test_valleys_are_the_ridges_of_the_negated_field():
    from opticalflowscivis_amd import ops
    f = RF.noise_nan((9, 12, 67), seed=5)[0]
    f[3, 4, 5] = 0.0  # (and -0.0 on the other side)
    t = torch.from_numpy(f[None]).cuda()
    a = ops.ridge_surfaces(t, (1.0, 0.5, 2.0), 0.1, -0.5, valley=True)
    b = ops.ridge_surfaces(-t, (1.0, 0.5, 2.0), 0.1, -0.5, valley=False)
    assert a["vertices"].shape[0] > 0 and a["faces"].shape[0] > 0
    for key in ("cls", "operands", "vertices", "values", "faces", "counts", "classes"):
        x, y = a[key].cpu().numpy(), b[key].cpu().numpy()
        assert x.shape == y.shape and np.array_equal(_bits(x) if x.dtype.kind == "f" else x,
                                                     _bits(y) if y.dtype.kind == "f" else y), key
    check(f[None], (1.0, 0.5, 2.0), 0.1, -0.5, valley=True)


def test_sentinel_tails_stay_untouched_and_a_wrong_offset_sets_status():
    from opticalflowscivis_amd import ops
    f = RF.noise((6, 7, 67), seed=6)[0]
    t = torch.from_numpy(f[None]).cuda()
    D, H, W = f.shape
    P = D * H * W
    operands, cls = ops.ridge_nodes(t)
    ws, off = ops.ridge_count(operands, cls)
    V, T = int(off[0, -1]), int(off[1, -1])
    assert V > 0 and T > 0
    want = R.ridges(f)
    one = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    PAD = 16
    row = int(np.nonzero(want["rows"][:, 0])[0][0])
    fewer = off.clone()
    fewer[0, row + 1:] -= 1
    for offsets, nv, status in ((off, V, 0), (fewer, V - 1, 1)):
        vert = torch.full(((nv + PAD) * 3,), 77.0, device="cuda")
        vals = torch.full(((nv + PAD) * 2,), 77.0, device="cuda")
        faces = torch.full(((T + PAD) * 3,), 77, dtype=torch.int32, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops._call("fs_ridge_emit3d", t.data_ptr(), 1, D, H, W, P, 0, operands.data_ptr(), cls.data_ptr(), one,
                  ws.data_ptr(), offsets.data_ptr(), nv, T, vert.data_ptr(), vals.data_ptr(), faces.data_ptr(),
                  st.data_ptr(), ops._stream(t))
        assert int(st) == status
        assert bool((vert[nv * 3:] == 77.0).all()) and bool((vals[nv * 2:] == 77.0).all()) and bool((faces[T * 3:] == 77).all())
        if status == 0:
            assert np.array_equal(_bits(vert[:V * 3].cpu().numpy().reshape(-1, 3)), _bits(want["vertices"]))
            assert np.array_equal(faces[:T * 3].cpu().numpy().reshape(-1, 3), want["faces"])
    with pytest.raises(ops._lib.FlowsciKernelError):
        ops.ridge_surfaces_check({"status": torch.ones(1, dtype=torch.int32)})


def test_two_calls_return_the_same_bits():
    from opticalflowscivis_amd import ops
    t = torch.from_numpy(RF.noise((9, 12, 67), seed=9)[0][None]).cuda()
    a, b = ops.ridge_surfaces(t), ops.ridge_surfaces(t)
    for key in ("vertices", "values", "faces", "operands", "cls"):
        assert torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), key


def test_every_error_code():
    from opticalflowscivis_amd import _lib
    lib = _lib.lib()
    OK, NULLPTR, SHAPE, ARG = 0, 1, 2, 3
    K, D, H, W = 2, 4, 5, 6
    P = D * H * W
    R_ = K * D * H
    assert lib.fs_ridge3d_ws_bytes(K, D, H, W) == 16 * R_ + K * P
    assert lib.fs_ridge3d_ws_bytes(0, D, H, W) == -SHAPE and lib.fs_ridge3d_ws_bytes(1, 1, H, W) == -SHAPE
    assert lib.fs_ridge3d_ws_bytes(1, 2048, 1024, 1024) == -SHAPE  # 2^31 nodes
    vols = torch.randn(K, D, H, W, device="cuda")
    operands = torch.zeros(K, 5, D, H, W, device="cuda")
    cls = torch.zeros(K, D, H, W, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(16 * R_ + K * P + 16, dtype=torch.uint8, device="cuda")
    off = torch.zeros(2, R_ + 1, dtype=torch.int64, device="cuda")
    vert = torch.zeros(8, 3, device="cuda")
    faces = torch.zeros(8, 3, dtype=torch.int32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    arr = lambda *v: (ctypes.c_double * 3)(*v)
    inf, nan = float("inf"), float("nan")

    def nodes(**kw):
        a = dict(v=vols.data_ptr(), K=K, D=D, H=H, W=W, ss=P, valley=0, i2=arr(.5, .5, .5), ihh=arr(1, 1, 1),
                 i4=arr(.25, .25, .25), strength=0.0, fmin=-inf, ops=operands.data_ptr(), cls=cls.data_ptr())
        a.update(kw)
        return lib.fs_ridge_nodes3d(a["v"], a["K"], a["D"], a["H"], a["W"], a["ss"], a["valley"], a["i2"], a["ihh"], a["i4"],
                                    a["strength"], a["fmin"], a["ops"], a["cls"], None)

    assert nodes() == OK and nodes(valley=7, fmin=0.5, strength=2.0) == OK
    for kw in (dict(v=None), dict(i2=None), dict(ihh=None), dict(i4=None), dict(ops=None), dict(cls=None)):
        assert nodes(**kw) == NULLPTR, kw
    for kw in (dict(K=0), dict(D=1), dict(H=1), dict(W=1), dict(ss=P - 1), dict(D=2048, H=1024, W=1024)):
        assert nodes(**kw) == SHAPE, kw
    for kw in (dict(i2=arr(.5, 0, .5)), dict(i2=arr(.5, .5, inf)), dict(ihh=arr(-1, 1, 1)), dict(ihh=arr(1, nan, 1)),
               dict(i4=arr(.25, .25, 0)), dict(i4=arr(nan, .25, .25)), dict(strength=-1.0), dict(strength=inf),
               dict(strength=nan), dict(fmin=inf), dict(fmin=nan)):
        assert nodes(**kw) == ARG, kw

    def count(**kw):
        a = dict(ops=operands.data_ptr(), cls=cls.data_ptr(), K=K, D=D, H=H, W=W, ws=ws.data_ptr())
        a.update(kw)
        return lib.fs_ridge_count3d(a["ops"], a["cls"], a["K"], a["D"], a["H"], a["W"], a["ws"], None)

    assert count() == OK
    for kw in (dict(ops=None), dict(cls=None), dict(ws=None)):
        assert count(**kw) == NULLPTR, kw
    for kw in (dict(K=0), dict(D=1), dict(H=1), dict(W=1), dict(D=2048, H=1024, W=1024)):
        assert count(**kw) == SHAPE, kw
    assert count(ws=ws.data_ptr() + 2) == ARG

    def emit(**kw):
        a = dict(v=vols.data_ptr(), K=K, D=D, H=H, W=W, ss=P, valley=0, ops=operands.data_ptr(), cls=cls.data_ptr(),
                 h=arr(1, 1, 1), ws=ws.data_ptr(), off=off.data_ptr(), V=0, T=0, vert=vert.data_ptr(), vals=None,
                 faces=faces.data_ptr(), st=st.data_ptr())
        a.update(kw)
        return lib.fs_ridge_emit3d(a["v"], a["K"], a["D"], a["H"], a["W"], a["ss"], a["valley"], a["ops"], a["cls"], a["h"],
                                   a["ws"], a["off"], a["V"], a["T"], a["vert"], a["vals"], a["faces"], a["st"], None)

    assert emit() == OK and emit(vert=None, faces=None) == OK  # V = T = 0: nothing launched, nothing needed
    for kw in (dict(v=None), dict(ops=None), dict(cls=None), dict(h=None), dict(ws=None), dict(off=None), dict(st=None),
               dict(V=1, vert=None), dict(T=1, faces=None)):
        assert emit(**kw) == NULLPTR, kw
    for kw in (dict(K=0), dict(D=1), dict(H=1), dict(W=1), dict(ss=P - 1), dict(D=2048, H=1024, W=1024)):
        assert emit(**kw) == SHAPE, kw
    for kw in (dict(h=arr(1, 0, 1)), dict(h=arr(1, 1, inf)), dict(h=arr(nan, 1, 1)), dict(h=arr(1, 1e39, 1)),
               dict(h=arr(1e-46, 1, 1)), dict(V=-1), dict(T=-1), dict(ws=ws.data_ptr() + 2)):
        assert emit(**kw) == ARG, kw
    torch.cuda.synchronize()
    assert int(st) == 0
