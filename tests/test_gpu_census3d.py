"""-m gpu: fs_census3d_dist_{fwd,bwd} and fs_flow_smooth3d_{fwd,bwd} against the fp64 restatement of
tests/census3d_ref.py, every voxel compared.  Bounds: the project's own for the 2-D census against its oracle
(test_gpu_losses.py::test_census_vs_oracle_c3_shape) -- values within 1e-5, gradients within 2e-4 of the largest
reference entry; the kernels use the same v_rsq / v_rcp approximations."""
import pytest
import torch

import census3d_ref as ref
from ledger_harness import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VAL_TOL, GRAD_TOL = 1e-5, 2e-4

# the kernel's brick is 8 x 16 x 32 (z, y, x): one brick exactly, one brick + 1 along every axis, W % 4 != 0 with B = 2,
# extents smaller than every patch, a single voxel, several bricks with ragged ends
SHAPES = [(1, 8, 16, 32), (1, 9, 17, 33), (2, 5, 10, 19), (1, 2, 3, 4), (1, 1, 1, 1), (2, 11, 20, 37)]


def relerr(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / max(float(b.abs().max()), 1e-30)


def _volumes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    B, D, H, W = shape
    v1 = torch.rand(B, 1, D, H, W, generator=g)
    v2 = (v1 + 0.1 * torch.randn(B, 1, D, H, W, generator=g)).clamp(0, 1)
    G = torch.randn(B, 1, D, H, W, generator=g)
    return v1, v2, G


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_census3d_dist_and_gradients_vs_fp64(shape, radius):
    from opticalflowscivis_amd import ops
    v1, v2, G = _volumes(shape, 10 * radius + shape[1])
    a, b = v1.double().requires_grad_(), v2.double().requires_grad_()
    want = ref.census3d_dist(a, b, radius)
    w1, w2 = torch.autograd.grad((want * G.double()).sum(), [a, b])
    c, d = v1.to(DEV).requires_grad_(), v2.to(DEV).requires_grad_()
    got = ops.census3d_dist(c, d, radius)
    g1, g2 = torch.autograd.grad((got * G.to(DEV)).sum(), [c, d])
    e = relerr(got.detach(), want.detach())
    e1, e2 = relerr(g1, w1), relerr(g2, w2)
    print("census3d %s r=%d: dist %.3g  grad1 %.3g  grad2 %.3g" % (shape, radius, e, e1, e2))
    assert got.shape == v1.shape
    assert e <= VAL_TOL and e1 <= GRAD_TOL and e2 <= GRAD_TOL, (e, e1, e2)
    # one gradient only: the other pointer is NULL
    (h1,) = torch.autograd.grad((ops.census3d_dist(c, v2.to(DEV), radius) * G.to(DEV)).sum(), [c])
    assert torch.equal(h1, g1)
    # the loss on top of it
    lw = ref.census3d_loss(a, b, radius)
    lg = ops.census3d_loss(c, d, radius)
    assert abs(float(lg) - float(lw)) <= VAL_TOL * abs(float(lw)), (float(lg), float(lw))
    r1, r2 = torch.autograd.grad(lw, [a, b])
    k1, k2 = torch.autograd.grad(lg, [c, d])
    assert relerr(k1, r1) <= GRAD_TOL and relerr(k2, r2) <= GRAD_TOL, (relerr(k1, r1), relerr(k2, r2))


def test_z_constant_volume_is_seven_times_the_2d_kernel():
    """The pin of test_census3d_cpu.py through the HIP path: at r = 3 a z-constant volume gives 7 x the 2-D kernel's
    distance on the slices 3 <= z <= D - 4."""
    from opticalflowscivis_amd import ops
    g = torch.Generator().manual_seed(4)
    D, H, W = 10, 21, 45
    rgb1 = torch.rand(2, 3, H, W, generator=g).to(DEV)
    rgb2 = (rgb1 + 0.1 * torch.randn(2, 3, H, W, generator=g).to(DEV)).clamp(0, 1)
    want = 7 * ops.census_dist(rgb1, rgb2)
    gray = lambda t: 0.2989 * t[:, 0:1] + 0.5870 * t[:, 1:2] + 0.1140 * t[:, 2:3]
    v1 = gray(rgb1)[:, :, None].expand(2, 1, D, H, W).contiguous()
    v2 = gray(rgb2)[:, :, None].expand(2, 1, D, H, W).contiguous()
    got = ops.census3d_dist(v1, v2, 3)
    scale = float(want.abs().max())
    for z in range(3, D - 3):
        dev = float((got[:, :, z] - want).abs().max())
        print("z = %d: largest deviation %.3g of the largest value" % (z, dev / scale))
        assert dev <= VAL_TOL * scale, (z, dev, scale)


@pytest.mark.parametrize("radius", [1, 3])
def test_census3d_writes_stay_inside_and_backward_is_bit_reproducible(radius):
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    shape = (2, 9, 17, 35)
    v1, v2, G = (t.to(DEV) for t in _volumes(shape, 3))
    n = v1.numel()
    st = torch.cuda.current_stream().cuda_stream
    dist = Guarded(n)
    _lib.check(L.fs_census3d_dist_fwd(v1.data_ptr(), v2.data_ptr(), dist.t.data_ptr(), *shape, radius, st), "fwd")
    runs = []
    for _ in range(2):
        g1, g2 = Guarded(n), Guarded(n)
        _lib.check(L.fs_census3d_dist_bwd(v1.data_ptr(), v2.data_ptr(), G.data_ptr(), g1.t.data_ptr(), g2.t.data_ptr(),
                                          *shape, radius, st), "bwd")
        runs.append((g1, g2))
    torch.cuda.synchronize()
    assert dist.intact() and all(g.intact() for r in runs for g in r)
    assert torch.isfinite(dist.t).all() and all(torch.isfinite(g.t).all() for r in runs for g in r)  # every element written
    assert torch.equal(runs[0][0].t, runs[1][0].t) and torch.equal(runs[0][1].t, runs[1][1].t)


def _pairs(B, C, D, H, W):
    return B * C * ((D - 1) * H * W + D * (H - 1) * W + D * H * (W - 1))


# a 1 along each axis in turn (no pair along it), C = 6 and C = 1, a volume of several workgroups, one voxel
SMOOTH_SHAPES = [(2, 6, 1, 7, 9), (1, 6, 5, 1, 9), (1, 6, 5, 7, 1), (1, 1, 4, 6, 5), (2, 6, 12, 20, 37), (1, 3, 1, 1, 1)]


@pytest.mark.parametrize("shape", SMOOTH_SHAPES)
@pytest.mark.parametrize("kappa,with_guide", [(0.0, False), (0.0, True), (12.5, True), (12.5, False)])
def test_flow_smooth3d_vs_fp64(shape, kappa, with_guide):
    from opticalflowscivis_amd import _lib, ops
    B, C, D, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    flow = torch.randn(B, C, D, H, W, generator=g) * 2
    guide = torch.rand(B, 1, D, H, W, generator=g) if with_guide else None
    q, eps = 0.25, 1e-9
    a = flow.double().requires_grad_()
    want = ref.flow_smooth3d(a, None if guide is None else guide.double(), q, eps, kappa)
    c = flow.to(DEV).requires_grad_()
    gd = None if guide is None else guide.to(DEV)
    got = ops.flow_smooth3d(c, gd, q, eps, kappa)
    n = _pairs(*shape)
    # the pair count, exactly
    sums = torch.empty(2, device=DEV)
    ws = torch.empty(2 * 1024, device=DEV)
    _lib.check(_lib.lib().fs_flow_smooth3d_fwd(c.data_ptr(), 0 if gd is None else gd.data_ptr(), sums.data_ptr(),
                                               ws.data_ptr(), B, C, D, H, W, q, eps, kappa,
                                               torch.cuda.current_stream().cuda_stream), "fs_flow_smooth3d_fwd")
    assert float(sums[1]) == float(n), (float(sums[1]), n)
    if n == 0:
        assert float(got) == 0.0 and float(want) == 0.0
        (gg,) = torch.autograd.grad(got, [c])
        assert float(gg.abs().max()) == 0.0
        return
    s1, cnt = ref.flow_smooth3d_sums(a.detach(), None if guide is None else guide.double(), q, eps, kappa)
    assert cnt == n
    assert abs(float(sums[0]) - float(s1)) <= VAL_TOL * float(s1)
    assert abs(float(got) - float(want)) <= VAL_TOL * abs(float(want)), (float(got), float(want))
    (gw,) = torch.autograd.grad(want, [a])
    (gg,) = torch.autograd.grad(got * 3.0, [c])  # an upstream factor reaches the kernel through coef
    e = relerr(gg, 3.0 * gw)
    print("flow_smooth3d %s kappa=%g guide=%s: value %.3g  grad %.3g" % (
        shape, kappa, with_guide, abs(float(got) - float(want)) / abs(float(want)), e))
    assert e <= GRAD_TOL, e
    (gg2,) = torch.autograd.grad(ops.flow_smooth3d(c, gd, q, eps, kappa) * 3.0, [c])
    assert torch.equal(gg, gg2)


def test_flow_smooth3d_writes_stay_inside():
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    B, C, D, H, W = 2, 6, 9, 17, 35
    g = torch.Generator().manual_seed(2)
    flow = torch.randn(B, C, D, H, W, generator=g).to(DEV)
    guide = torch.rand(B, 1, D, H, W, generator=g).to(DEV)
    coef = torch.full((1,), 0.5, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    sums, ws, gf = Guarded(2), Guarded(2 * 1024), Guarded(flow.numel())
    _lib.check(L.fs_flow_smooth3d_fwd(flow.data_ptr(), guide.data_ptr(), sums.t.data_ptr(), ws.t.data_ptr(), B, C, D, H,
                                      W, 0.25, 1e-9, 5.0, st), "fwd")
    _lib.check(L.fs_flow_smooth3d_bwd(flow.data_ptr(), guide.data_ptr(), coef.data_ptr(), gf.t.data_ptr(), B, C, D, H, W,
                                      0.25, 1e-9, 5.0, st), "bwd")
    torch.cuda.synchronize()
    assert sums.intact() and ws.intact() and gf.intact()
    assert torch.isfinite(sums.t).all() and torch.isfinite(gf.t).all()


def test_wrappers_refuse_bad_operands():
    from opticalflowscivis_amd import ops
    v = torch.rand(1, 1, 4, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.census3d_dist(v, v, 4)
    with pytest.raises(ValueError):
        ops.census3d_dist(v, torch.rand(1, 1, 4, 4, 5, device=DEV), 1)
    with pytest.raises(ValueError):
        ops.census3d_dist(torch.rand(1, 2, 4, 4, 4, device=DEV), torch.rand(1, 2, 4, 4, 4, device=DEV), 1)
    f = torch.rand(1, 6, 4, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.flow_smooth3d(f, torch.rand(1, 1, 4, 4, 5, device=DEV), kappa=1.0)
    with pytest.raises(ValueError):
        ops.flow_smooth3d(f, None, eps=0.0)
    with pytest.raises(ValueError):
        ops.flow_smooth3d(f.double())
