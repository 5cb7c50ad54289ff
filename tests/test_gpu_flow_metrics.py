"""GPU: fs_flow_metrics{2,3}d / ops.flow_metrics against the fp64 restatement in tests/flow_metrics_ref.py, the
special values, determinism, strided inputs, the C-ABI's refusals and the round trip through the HIP 3-D warp."""
import math

import numpy as np
import pytest
import torch

import flow_metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("epe", "epe_noc", "epe_occ", "rmse", "ae_deg", "fl", "fl_noc", "fl_occ", "max_epe", "n_valid", "n_noc",
        "n_nonfinite")
COUNTS = ("n_valid", "n_noc", "n_nonfinite")


def _flows(N, C, sp, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn((N, C) + sp, generator=g) * scale
    pred = gt + torch.randn((N, C) + sp, generator=g) * torch.rand((N, 1) + sp, generator=g) * scale
    return pred, gt


def _masks(N, sp, kind, seed):
    if kind == "absent":
        return None, None
    g = torch.Generator().manual_seed(seed + 99)
    if kind == "zero":
        return torch.zeros((N,) + sp, dtype=torch.bool), torch.zeros((N,) + sp, dtype=torch.bool)
    return torch.rand((N,) + sp, generator=g) < 0.8, torch.rand((N,) + sp, generator=g) < 0.6


def _check(res, want, n_elem_map=None):
    for k in KEYS:
        a, b = res[k].cpu().numpy(), want[k]
        assert a.dtype == np.float64 and a.shape == b.shape, k
        if k in COUNTS:
            assert np.array_equal(a, b, equal_nan=True), (k, a, b)
            continue
        assert np.array_equal(np.isnan(a), np.isnan(b)), (k, a, b)
        m = ~np.isnan(b)
        np.testing.assert_allclose(a[m], b[m], rtol=1e-6, atol=1e-12, err_msg=k)


def _run(pred, gt, valid, noc, convention="disp", tau=(3.0, 0.05)):
    from opticalflowscivis_amd import ops
    d = lambda t: None if t is None else t.to(DEV)
    res = ops.flow_metrics(d(pred), d(gt), d(valid), d(noc), convention, tau, return_map=True)
    want = ref.stats(pred.numpy(), gt.numpy(), None if valid is None else valid.numpy(),
                     None if noc is None else noc.numpy(), convention, tau)
    _check(res, want)
    m = res["epe_map"].cpu().numpy()
    wm = ref.epe_map(pred.numpy(), gt.numpy(), convention)
    assert np.array_equal(np.isnan(m), np.isnan(wm))
    ok = ~np.isnan(wm)
    ulp = np.abs(m[ok].view(np.int32).astype(np.int64) - wm[ok].view(np.int32).astype(np.int64))
    assert ulp.max(initial=0) <= 2
    return res


@pytest.mark.parametrize("masks", ["absent", "partial", "zero"])
@pytest.mark.parametrize("sp", [(1, 1), (3, 3), (17, 17), (13, 31), (64, 96), (7, 1), (1, 29)])
def test_2d_matches_restatement(sp, masks):
    pred, gt = _flows(3, 2, sp, seed=sum(sp))
    v, n = _masks(3, sp, masks, seed=sum(sp))
    _run(pred, gt, v, n)


@pytest.mark.parametrize("convention", ["disp", "rife3d"])
@pytest.mark.parametrize("masks", ["absent", "partial", "zero"])
@pytest.mark.parametrize("sp", [(3, 3, 3), (17, 17, 17), (5, 11, 13), (2, 3, 7), (8, 12, 16)])
def test_3d_matches_restatement(sp, masks, convention):
    pred, gt = _flows(2, 3, sp, seed=sum(sp) + 1, scale=1.5)
    v, n = _masks(2, sp, masks, seed=sum(sp))
    _run(pred, gt, v, n, convention)


@pytest.mark.parametrize("N,sp", [(1, (67, 71, 73)), (1, (128, 129, 131)), (2, (4, 6, 9)), (3, (4, 3, 3))])
def test_rife3d_grid_stride_and_row_carries(N, sp):
    """(d, h, w) advance by carries: across grid-stride steps that are not a multiple of a row or a plane ((67,71,73):
    single elements, two steps; (128,129,131): groups of 4, three steps) and inside groups of 4 that straddle rows
    (W = 9, 3, 131 are not multiples of 4; with H x W = 3 x 3 a group also straddles planes)."""
    pred, gt = _flows(N, 3, sp, seed=sum(sp), scale=1.5)
    _run(pred, gt, *_masks(N, sp, "partial", seed=sum(sp)), convention="rife3d")


@pytest.mark.parametrize("sp", [(150, 450), (12, 15), (6, 2)])
def test_2d_vector_path_with_rows_not_multiple_of_4(sp):
    """Rows of any length take the 16-byte path when the plane size is a multiple of 4 (the UPFlow C3 shape 150 x 450
    among them); the result equals the restatement and the copy that cannot take it (misaligned by one element)."""
    from opticalflowscivis_amd import ops
    pred, gt = _flows(4, 2, sp, seed=sum(sp))
    v, n = _masks(4, sp, "partial", seed=sum(sp))
    res = _run(pred, gt, v, n)
    buf = torch.empty(pred.numel() + 1, device=DEV)
    shifted = buf[1:].view(pred.shape)
    shifted.copy_(pred.to(DEV))
    r1 = ops.flow_metrics(shifted, gt.to(DEV), v.to(DEV), n.to(DEV), return_map=True)
    for k in COUNTS:
        assert torch.equal(res[k], r1[k]), k
    assert torch.equal(res["epe_map"], r1["epe_map"])


def test_3d_extent_1_disp():
    for sp in ((1, 1, 1), (1, 5, 8), (4, 1, 1)):
        pred, gt = _flows(2, 3, sp, seed=3)
        _run(pred, gt, *_masks(2, sp, "partial", seed=3))


def test_3d_256_cubed():
    sp = (256, 256, 256)
    pred, gt = _flows(2, 3, sp, seed=256, scale=2.0)
    valid, noc = _masks(2, sp, "partial", seed=256)
    for conv in ("disp", "rife3d"):
        _run(pred, gt, valid, noc, conv)


def test_thresholds_and_counts_exact():
    """Fl uses epe > tau_abs and epe > tau_rel |g|: counts follow the restatement exactly for other taus too."""
    pred, gt = _flows(4, 2, (40, 56), seed=8)
    v, n = _masks(4, (40, 56), "partial", seed=8)
    for tau in ((3.0, 0.05), (1.0, 0.5), (0.0, 0.0), (10.0, 0.0)):
        _run(pred, gt, v, n, tau=tau)


def test_equal_flows_give_zero():
    from opticalflowscivis_amd import ops
    for sp in ((33, 47), (9, 10, 11)):
        _, gt = _flows(2, len(sp), sp, seed=4)
        g = gt.to(DEV)
        r = ops.flow_metrics(g.clone(), g, return_map=True)
        for k in ("epe", "rmse", "ae_deg", "fl", "max_epe"):
            assert torch.all(r[k] == 0), k
        assert torch.all(r["epe_map"] == 0)


def test_strided_channel_slice_equals_contiguous_bitwise():
    from opticalflowscivis_amd import ops
    for C, sp, conv in ((2, (24, 36), "disp"), (3, (12, 16, 20), "rife3d"), (3, (5, 7, 9), "disp")):
        g = torch.Generator().manual_seed(C)
        full = torch.randn((3, 2 * C) + sp, generator=g).to(DEV)
        gt = torch.randn((3, C) + sp, generator=g).to(DEV)
        valid, noc = (m.to(DEV) for m in _masks(3, sp, "partial", seed=C))
        a = ops.flow_metrics(full[:, C:], gt, valid, noc, conv, return_map=True)
        b = ops.flow_metrics(full[:, C:].contiguous(), gt, valid, noc, conv, return_map=True)
        gfull = torch.cat([gt, gt], 1)
        c = ops.flow_metrics(full[:, :C], gfull[:, C:], valid, noc, conv, return_map=True)
        d = ops.flow_metrics(full[:, :C].contiguous(), gt, valid, noc, conv, return_map=True)
        for k in KEYS + ("epe_map",):
            assert torch.equal(a[k].nan_to_num(-7), b[k].nan_to_num(-7)), k
            assert torch.equal(c[k].nan_to_num(-7), d[k].nan_to_num(-7)), k


def test_two_runs_bitwise_equal():
    from opticalflowscivis_amd import ops
    pred, gt = _flows(2, 3, (40, 48, 64), seed=12)
    v, n = _masks(2, (40, 48, 64), "partial", seed=12)
    args = [t.to(DEV) for t in (pred, gt, v, n)]
    a = ops.flow_metrics(*args, convention="rife3d")
    b = ops.flow_metrics(*args, convention="rife3d")
    for k in KEYS:
        assert torch.equal(a[k].nan_to_num(-7), b[k].nan_to_num(-7)), k


@pytest.mark.parametrize("where", ["pred", "gt"])
def test_nonfinite_elements(where):
    """A non-finite pred or gt counts as an outlier and in n_nonfinite, is left out of the sums and the max, and maps
    to NaN; invalid elements do not count at all."""
    from opticalflowscivis_amd import ops
    sp = (16, 20)
    pred, gt = _flows(2, 2, sp, seed=21, scale=0.5)
    valid, noc = _masks(2, sp, "partial", seed=21)
    valid[:, :4, :4] = True
    valid[:, 4, 4] = False
    noc[:, 0, :4] = True
    t = pred if where == "pred" else gt
    t[0, 0, 0, 0] = float("nan")
    t[0, 1, 0, 1] = float("inf")
    t[0, 0, 0, 2] = -float("inf")
    t[1, 1, 3, 3] = float("nan")          # valid, not necessarily noc
    t[1, 0, 4, 4] = float("inf")          # invalid: ignored by the statistics, NaN in the map
    res = _run(pred, gt, valid, noc)
    assert res["n_nonfinite"].tolist() == [3.0, 1.0]
    m = res["epe_map"].cpu()
    assert math.isnan(m[0, 0, 0]) and math.isnan(m[0, 0, 1]) and math.isnan(m[0, 0, 2]) and math.isnan(m[1, 4, 4])
    for k in ("epe", "rmse", "ae_deg", "max_epe"):
        assert torch.isfinite(res[k]).all(), k
    # all elements non-finite: Fl = 1, the means NaN
    bad = torch.full((1, 2, 4, 4), float("nan"), device=DEV)
    r = ops.flow_metrics(bad, torch.zeros_like(bad))
    assert float(r["fl"][0]) == 1.0 and math.isnan(float(r["epe"][0])) and math.isnan(float(r["max_epe"][0]))


def test_empty_subsets_give_nan():
    from opticalflowscivis_amd import ops
    x = torch.rand(2, 2, 8, 8, device=DEV)
    z = torch.zeros(2, 8, 8, dtype=torch.bool, device=DEV)
    r = ops.flow_metrics(x, x * 0, valid=z, noc=z)
    for k in ("epe", "epe_noc", "epe_occ", "rmse", "ae_deg", "fl", "fl_noc", "fl_occ", "max_epe"):
        assert torch.isnan(r[k]).all(), k
    r = ops.flow_metrics(x, x * 0)  # no noc: the split is NaN, the rest is not
    assert torch.isnan(r["epe_noc"]).all() and torch.isnan(r["fl_occ"]).all() and torch.isfinite(r["epe"]).all()


def test_c_abi_errors_and_ws_query():
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    ws = torch.zeros(4096, dtype=torch.float64, device=DEV)
    out = torch.zeros(64, dtype=torch.float64, device=DEV)
    x = torch.zeros(2, 3, 4, 4, 4, device=DEV)
    p, w, o = x.data_ptr(), ws.data_ptr(), out.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    assert L.fs_flow_metrics3d(p, p, 2, 3, 4, 4, 4, 192, 192, None, None, 0, 3.0, 0.05, None, w, o, s) == 0
    assert L.fs_flow_metrics3d(p, p, 2, 2, 4, 4, 4, 192, 192, None, None, 0, 3.0, 0.05, None, w, o, s) == 2  # C
    assert L.fs_flow_metrics2d(p, p, 2, 3, 4, 4, 48, 48, None, None, 3.0, 0.05, None, w, o, s) == 2         # C
    assert L.fs_flow_metrics3d(p, p, 2, 3, 1, 8, 8, 192, 192, None, None, 1, 3.0, 0.05, None, w, o, s) == 2  # D < 2
    assert L.fs_flow_metrics3d(p, p, 2, 3, 8, 8, 1, 192, 192, None, None, 1, 3.0, 0.05, None, w, o, s) == 2  # W < 2
    assert L.fs_flow_metrics3d(p, p, 2, 3, 4, 4, 4, 100, 192, None, None, 0, 3.0, 0.05, None, w, o, s) == 2  # stride
    assert L.fs_flow_metrics3d(p, p, 2, 3, 4, 4, 4, 192, 192, None, None, 2, 3.0, 0.05, None, w, o, s) == 3  # conv
    assert L.fs_flow_metrics3d(p, p, 2, 3, 4, 4, 4, 192, 192, None, None, 0, -1.0, 0.05, None, w, o, s) == 3
    assert L.fs_flow_metrics3d(None, p, 2, 3, 4, 4, 4, 192, 192, None, None, 0, 3.0, 0.05, None, w, o, s) == 1
    assert L.fs_flow_metrics3d(p, None, 2, 3, 4, 4, 4, 192, 192, None, None, 0, 3.0, 0.05, None, w, o, s) == 1
    assert L.fs_flow_metrics2d(p, p, 2, 2, 4, 4, 32, 32, None, None, 3.0, 0.05, None, None, o, s) == 1      # ws
    assert L.fs_flow_metrics2d(p, p, 2, 2, 4, 4, 32, 32, None, None, 3.0, 0.05, None, w, None, s) == 1      # out
    torch.cuda.synchronize()


def test_gt_drives_the_hip_3d_warp():
    """Warping frame t+g with disp_to_rife3d(gt(mid, t+g)) through the model's HIP warp reproduces the mid frame on
    interior noc voxels (S = 32, an integer velocity so that the binary sphere moves by whole voxels)."""
    from opticalflowscivis_amd import ops
    from opticalflowscivis_amd.data import synthetic
    frames, gt = synthetic.droplet3d_motion(5, 32, seed=9, v=(1.0, 1.0, -1.0), device=DEV)
    t, g = 0, 4
    mid = (t + t + g) // 2
    disp, valid, noc = gt(mid, t + g)
    flow = ops.disp_to_rife3d(disp.unsqueeze(0))
    warped = ops.warp3d(frames[t + g].view(1, 1, 32, 32, 32), flow.contiguous())[0, 0]
    inside = disp.abs().sum(0) > 0
    pool = lambda m: torch.nn.functional.max_pool3d((~m).float()[None, None], 5, 1, 2)[0, 0] == 0
    far = pool(noc) & (pool(inside) | pool(~inside))
    assert int(far.sum()) > 1000
    assert float((warped - frames[mid])[far].abs().max()) < 1e-4
    # the kernel agrees: the converted flow scores ~0 against the displacement there
    r = ops.flow_metrics(flow, disp.unsqueeze(0), valid=far.unsqueeze(0), convention="rife3d")
    assert float(r["max_epe"][0]) < 1e-4 and float(r["fl"][0]) == 0.0
