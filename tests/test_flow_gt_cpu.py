"""CPU: the ground-truth motion of the synthetic sequences (data/synthetic.py *_motion) and the Flow-3D flow <->
displacement conversion (ops.rife3d_to_disp / disp_to_rife3d), checked with the oracle's closed-form warps."""
import pytest
import torch

from oracle.warps import warp2d_rife_closed, warp3d_closed
from opticalflowscivis_amd import ops
from opticalflowscivis_amd.data import synthetic


def test_motion_frames_equal_sequences_bitwise():
    assert torch.equal(synthetic.rectangle2d_motion(24, seed=7)[0], synthetic.rectangle2d_sequence(24, seed=7)[0])
    assert torch.equal(synthetic.droplet2d_motion(9, 48, 64, seed=3)[0], synthetic.droplet2d_sequence(9, 48, 64, seed=3))
    assert torch.equal(synthetic.droplet3d_motion(5, 24, seed=3)[0], synthetic.droplet3d_sequence(5, 24, seed=3))
    assert torch.equal(synthetic.jets3d_motion(5, 20, seed=3)[0], synthetic.jets3d_sequence(5, 20, seed=3))


@pytest.mark.parametrize("pair", [(0, 1), (5, 3), (10, 14), (13, 29)])
def test_rectangle2d_gt_warps_exactly(pair):
    frames, gt = synthetic.rectangle2d_motion(32, seed=11)
    a, b = pair
    disp, valid, noc = gt(a, b)
    assert valid.all() and disp.shape == (2, 128, 128)
    assert float(disp.abs().max()) > 0  # the box moves between these frames
    assert torch.equal(disp, disp.round())
    warped = warp2d_rife_closed(frames[b].view(1, 1, 128, 128), disp.unsqueeze(0))[0, 0]
    assert torch.equal(warped[noc], frames[a][noc])
    assert (~noc).any() or float(disp.abs().max()) == 0
    # occluded pixels are background that the box covers at t_to
    occ = ~noc
    assert torch.all(frames[a][occ] == 0) and torch.all(frames[b][occ] > 0)


def test_rectangle2d_gt_uses_clamped_positions():
    """At a wall the stored velocity is not the motion: the ground truth follows the box."""
    frames, vx, vy = synthetic.rectangle2d_sequence(64, seed=1234)
    _, gt = synthetic.rectangle2d_motion(64, seed=1234)
    mismatched = 0
    for t in range(63):
        disp, _, _ = gt(t, t + 1)
        box = frames[t + 1] > 0
        inside = frames[t] > 0
        mismatched += int(float(disp[0][inside][0]) != float(vx[t + 1][box][0]) or
                          float(disp[1][inside][0]) != float(vy[t + 1][box][0]))
        warped = warp2d_rife_closed(frames[t + 1].view(1, 1, 128, 128), disp.unsqueeze(0))[0, 0]
        assert torch.equal(warped[inside], frames[t][inside])
    assert mismatched > 0  # the sequence does hit a wall: stored velocities would be wrong there


def _interior(mask, k):
    """mask eroded by k pixels / voxels (max-pool of the complement)."""
    nd = mask.dim()
    x = (~mask).float().unsqueeze(0).unsqueeze(0)
    pool = torch.nn.functional.max_pool2d if nd == 2 else torch.nn.functional.max_pool3d
    return pool(x, 2 * k + 1, 1, k)[0, 0] == 0


def test_droplet2d_integer_velocity_warps_on_interior():
    frames, gt = synthetic.droplet2d_motion(7, 64, 80, seed=5, v=(2.0, -1.0))
    disp, valid, noc = gt(1, 4)
    assert float(disp[0].min()) == -3.0 and float(disp[1].max()) == 6.0
    inside = disp.abs().sum(0) > 0
    assert (~noc & valid).any()
    warped = warp2d_rife_closed(frames[4].view(1, 1, 64, 80), disp.unsqueeze(0))[0, 0]
    far = _interior(noc, 4) & (_interior(inside, 4) | _interior(~inside, 4))
    assert far.sum() > 500
    assert float((warped - frames[1])[far].abs().max()) < 1e-6


def test_droplet3d_integer_velocity_warps_on_interior():
    frames, gt = synthetic.droplet3d_motion(5, 32, seed=5, v=(1.0, -1.0, 2.0))
    disp, valid, noc = gt(3, 1)
    assert [float(disp[c].abs().max()) for c in range(3)] == [4.0, 2.0, 2.0]
    rife = ops.disp_to_rife3d(disp.unsqueeze(0).double())
    warped = warp3d_closed(frames[1].double().view(1, 1, 32, 32, 32), rife)[0, 0]
    inside = disp.abs().sum(0) > 0
    far = _interior(noc, 2) & (_interior(inside, 2) | _interior(~inside, 2))
    assert far.sum() > 1000
    assert float((warped - frames[3].double())[far].abs().max()) < 1e-9


def test_jets3d_gt_is_density_weighted_plume_velocity():
    frames, gt = synthetic.jets3d_motion(4, 24, seed=2, njets=1)
    disp, valid, noc = gt(0, 3)
    assert torch.equal(valid, noc) and torch.equal(valid, frames[0] > 0.05)
    # one plume: a uniform displacement, (S-1) * 3 * vel reversed into (x, y, z)
    g = synthetic._gen(2, "cpu")
    torch.rand(1, 3, generator=g), torch.rand(1, 3, generator=g)
    vel = (torch.rand(1, 3, generator=g) * 2 - 1) / 24
    want = torch.tensor([float(vel[0, 2 - c]) * 23 * 3 for c in range(3)])
    assert torch.allclose(disp[:, valid].mean(1), want, rtol=1e-5, atol=1e-6)
    assert float((disp[:, valid] - want.view(3, 1)).abs().max()) < 1e-5


@pytest.mark.parametrize("shape", [(6, 7, 9), (8, 8, 8), (3, 17, 5)])
def test_rife3d_round_trip(shape):
    g = torch.Generator().manual_seed(0)
    d = torch.randn((2, 3) + shape, generator=g) * 3
    back = ops.rife3d_to_disp(ops.disp_to_rife3d(d))
    assert float((back - d).abs().max()) < 1e-5
    f = torch.randn((2, 3) + shape, generator=g)
    assert float((ops.disp_to_rife3d(ops.rife3d_to_disp(f)) - f).abs().max()) < 1e-5


@pytest.mark.parametrize("shape", [(9, 9, 9), (7, 12, 10), (13, 6, 8)])
def test_rife3d_conversion_matches_warp3d_sample_points(shape):
    """warp3d_closed of a ramp along one axis returns the sample coordinate along that axis: with a small flow that
    stays inside the volume it equals (index + displacement) exactly as rife3d_to_disp says."""
    D, H, W = shape
    g = torch.Generator().manual_seed(1)
    flow = (torch.rand((1, 3) + shape, generator=g, dtype=torch.float64) - 0.5) * 0.6
    disp = ops.rife3d_to_disp(flow)[0]
    d = torch.arange(D, dtype=torch.float64).view(D, 1, 1).expand(D, H, W)
    h = torch.arange(H, dtype=torch.float64).view(1, H, 1).expand(D, H, W)
    w = torch.arange(W, dtype=torch.float64).view(1, 1, W).expand(D, H, W)
    ramps = torch.stack([w, h, d]).unsqueeze(0)  # channel 0 ramps along W, 1 along H, 2 along D
    out = warp3d_closed(ramps, flow)[0]
    want = torch.stack([w + disp[0], h + disp[1], d + disp[2]])
    lim = torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float64).view(3, 1, 1, 1)
    inside = ((want >= 0) & (want <= lim)).all(0)
    assert inside.float().mean() > 0.5
    assert float((out - want)[:, inside].abs().max()) < 1e-9
    assert float(ops.rife3d_to_disp(torch.zeros((1, 3) + shape, dtype=torch.float64)).abs().max()) > 0  # 0 is not rest


def test_rife3d_conversion_needs_extent_2():
    with pytest.raises(ValueError, match=">= 2"):
        ops.rife3d_to_disp(torch.zeros(1, 3, 1, 4, 4))


def test_flow_metrics_refuses_cpu_tensors():
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.flow_metrics(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8))


def test_flow_metrics_abi_refusals_and_ws_query_without_gpu():
    """Argument checks and the _ws_bytes queries run on the host before anything is launched: on a machine without a
    GPU they answer all the same (the queries launch nothing).  Only NULL pointers are passed here."""
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    assert L.fs_flow_metrics2d_ws_bytes(1, 2, 3, 3) == 13 * 8
    assert L.fs_flow_metrics3d_ws_bytes(2, 3, 256, 256, 256, 1) == 1024 * 13 * 8
    assert L.fs_flow_metrics3d_ws_bytes(2, 3, 1, 8, 8, 1) == -2 and L.fs_flow_metrics3d_ws_bytes(2, 3, 1, 8, 8, 0) > 0
    assert L.fs_flow_metrics2d_ws_bytes(2, 3, 8, 8) == -2 and L.fs_flow_metrics3d_ws_bytes(2, 3, 8, 8, 8, 5) == -3
    assert L.fs_flow_metrics2d_ws_bytes(0, 2, 8, 8) == -2 and L.fs_flow_metrics3d_ws_bytes(1, 2, 8, 8, 8, 0) == -2
    assert L.fs_flow_metrics2d(None, None, 1, 2, 8, 8, 128, 128, None, None, 3.0, 0.05, None, None, None, None) == 1
    assert L.fs_flow_metrics3d(None, None, 1, 3, 8, 8, 8, 192, 192, None, None, 1, 3.0, 0.05, None, None, None,
                               None) == 1


class _StubRife:
    """A RIFE stand-in whose final flow, at the padded extents it is given, is the model flow of the displacement
    `disp` (x, y, z) everywhere: what a perfect Flow-3D model would emit for that motion."""

    def __init__(self, disp):
        self.disp = disp

    def inference(self, a, b):
        B = a.shape[0]
        d = torch.tensor(self.disp, dtype=torch.float64).view(1, 3, 1, 1, 1).expand((B, 3) + tuple(a.shape[2:]))
        f = ops.disp_to_rife3d(d).float()
        return None, [f, f, torch.cat([f, f], 1)], None


@pytest.mark.parametrize("sp", [(20, 24, 40), (40, 64, 96), (33, 17, 50)])
def test_flow3d_eval_converts_at_the_padded_extents(sp):
    """The model ran on the volume padded to multiples of 32, so its warp used the padded extents' ratios: the
    displacement must come from the uncropped flow (crop-then-convert is off by voxels for non-cubic volumes)."""
    from opticalflowscivis_amd.flow_eval import rife_flows
    frames = torch.rand((4,) + sp)
    want = (0.5, -0.25, 0.75)
    out = rife_flows(_StubRife(want), frames, [(0, 2), (1, 3)], batch=2)
    assert out.shape == (4, 3) + sp
    for c in range(3):
        assert float((out[:, c] - want[c]).abs().max()) < 1e-4, c
