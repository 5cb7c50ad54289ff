"""CPU: the restatement of the 3-D census distance and of the flow smoothness (tests/census3d_ref.py) is pinned to the
reference-pinned 2-D oracle and to hand-written sums; the argument checks of the new entry points run before any
launch, so they are testable here too."""
import numpy as np
import pytest
import torch

import census3d_ref as ref
from oracle import losses as olosses


def _gray(rgb):
    R, G, B = torch.split(rgb, 1, 1)
    return 0.2989 * R + 0.5870 * G + 0.1140 * B  # as oracle.losses.census_dist forms it


def test_z_constant_volume_is_seven_times_the_2d_oracle():
    """A volume whose every z-slice is the grey image: each of the seven dz planes of the r = 3 patch repeats the 2-D
    sum, so on the slices 3 <= z <= D - 4 the 3-D distance is 7 x the 2-D oracle's, image borders included."""
    g = torch.Generator().manual_seed(4)
    D = 10
    rgb1 = torch.rand(1, 3, 12, 14, generator=g)
    rgb2 = (rgb1 + 0.1 * torch.randn(1, 3, 12, 14, generator=g)).clamp(0, 1)
    want = 7 * olosses.census_dist(rgb1, rgb2)  # [1,1,H,W]
    v1 = _gray(rgb1)[:, :, None].expand(1, 1, D, 12, 14).contiguous()
    v2 = _gray(rgb2)[:, :, None].expand(1, 1, D, 12, 14).contiguous()
    got = ref.census3d_dist(v1, v2, 3)
    scale = float(want.abs().max())
    for z in range(3, D - 3):
        dev = float((got[:, :, z] - want).abs().max())
        print("z = %d: largest deviation %.3g of the largest value" % (z, dev / scale))
        assert dev <= 1e-5 * scale, (z, dev, scale)


def test_census_restatement_gradcheck():
    g = torch.Generator().manual_seed(1)
    a = torch.rand(1, 1, 3, 4, 3, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.rand(1, 1, 3, 4, 3, generator=g, dtype=torch.float64).requires_grad_()
    for r in (1, 2):
        assert torch.autograd.gradcheck(lambda x, y: ref.census3d_dist(x, y, r), (a, b), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda x, y: ref.census3d_loss(x, y, 1), (a, b), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("kappa", [0.0, 7.5])
def test_smoothness_restatement_against_three_loops(kappa):
    rng = np.random.default_rng(8)
    flow = rng.standard_normal((2, 2, 3, 4, 5))
    guide = rng.random((2, 1, 3, 4, 5))
    q, eps = 0.25, 1e-3
    s1, n = 0.0, 0
    for b in range(2):
        for c in range(2):
            for z in range(3):
                for y in range(4):
                    for x in range(5):
                        for dz, dy, dx in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                            zz, yy, xx = z + dz, y + dy, x + dx
                            if zz >= 3 or yy >= 4 or xx >= 5:
                                continue
                            w = np.exp(-kappa * abs(guide[b, 0, zz, yy, xx] - guide[b, 0, z, y, x]))
                            s1 += w * ((flow[b, c, zz, yy, xx] - flow[b, c, z, y, x]) ** 2 + eps ** 2) ** q
                            n += 1
    got, cnt = ref.flow_smooth3d_sums(torch.from_numpy(flow), torch.from_numpy(guide), q, eps, kappa)
    assert cnt == n == 2 * 2 * (2 * 4 * 5 + 3 * 3 * 5 + 3 * 4 * 4)
    assert abs(float(got) - s1) <= 1e-12 * s1
    mean = ref.flow_smooth3d(torch.from_numpy(flow), torch.from_numpy(guide), q, eps, kappa)
    assert abs(float(mean) - s1 / n) <= 1e-12 * s1 / n
    f = torch.from_numpy(flow).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: ref.flow_smooth3d(t, torch.from_numpy(guide), q, eps, kappa), (f,),
                                    eps=1e-6, atol=1e-7)


def test_entry_points_refuse_bad_arguments_before_launching():
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    assert L.fs_census3d_dist_fwd(None, 1, 1, 1, 8, 8, 8, 1, None) == 1           # NULLPTR
    assert L.fs_census3d_dist_fwd(1, 1, 1, 1, 8, 8, 8, 0, None) == 3              # ARG: radius
    assert L.fs_census3d_dist_fwd(1, 1, 1, 1, 8, 8, 8, 4, None) == 3
    assert L.fs_census3d_dist_fwd(1, 1, 1, 1, 0, 8, 8, 1, None) == 2              # SHAPE
    assert L.fs_census3d_dist_fwd(1, 1, 1, 9000, 64, 8, 8, 1, None) == 2          # B * ceil(D / 8) > 65535
    assert L.fs_census3d_dist_bwd(1, 1, 1, None, None, 1, 8, 8, 8, 1, None) == 1  # no gradient asked for
    assert L.fs_census3d_dist_bwd(1, 1, 1, 1, None, 1, 8, 8, 8, 5, None) == 3
    assert L.fs_flow_smooth3d_fwd(1, None, 1, None, 1, 6, 8, 8, 8, 0.25, 1e-9, 0.0, None) == 1
    assert L.fs_flow_smooth3d_fwd(1, None, 1, 1, 1, 0, 8, 8, 8, 0.25, 1e-9, 0.0, None) == 2
    assert L.fs_flow_smooth3d_fwd(1, None, 1, 1, 1, 6, 8, 8, 8, 0.25, 0.0, 0.0, None) == 3    # eps = 0
    assert L.fs_flow_smooth3d_fwd(1, None, 1, 1, 1, 6, 8, 8, 8, 0.0, 1e-9, 0.0, None) == 3    # q = 0
    assert L.fs_flow_smooth3d_fwd(1, None, 1, 1, 1, 6, 8, 8, 8, 0.25, 1e-9, -1.0, None) == 3  # kappa < 0
    assert L.fs_flow_smooth3d_bwd(1, None, 1, None, 1, 6, 8, 8, 8, 0.25, 1e-9, 0.0, None) == 1


def test_ops_and_record_validate_on_the_host():
    from opticalflowscivis_amd import ops
    from opticalflowscivis_amd.rife import UnsupLoss
    v = torch.rand(1, 1, 4, 4, 4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.census3d_dist(v, v, 1)
    with pytest.raises(ValueError):
        ops.flow_smooth3d(torch.rand(1, 6, 4, 4, 4))
    assert UnsupLoss() == UnsupLoss(0., 0., 0., 1, 0.4, 0., 0.25, 1e-9)
    with pytest.raises(ValueError):
        UnsupLoss(census=1.0, census_radius=4)
    with pytest.raises(ValueError):
        UnsupLoss(photo=-1.0)
    with pytest.raises(AttributeError):
        UnsupLoss().photo = 1.0


def test_parsers_take_the_flags_in_3d_only():
    import argparse
    from opticalflowscivis_amd.trainer import add_common_args, unsup_from_args
    a = add_common_args(argparse.ArgumentParser(), 3).parse_args(
        "--dataset droplet3d --photo 1e-3 --census 1e-3 --smooth 1e-4 --census_radius 2 --smooth_kappa 10".split())
    u = unsup_from_args(a, 3)
    assert (u.photo, u.census, u.smooth, u.census_radius, u.smooth_kappa) == (1e-3, 1e-3, 1e-4, 2, 10.0)
    assert unsup_from_args(add_common_args(argparse.ArgumentParser(), 3).parse_args([]), 3) is None
    with pytest.raises(SystemExit):
        add_common_args(argparse.ArgumentParser(), 2).parse_args(["--census", "1"])
    with pytest.raises(SystemExit):
        add_common_args(argparse.ArgumentParser(), 3).parse_args(["--census_radius", "4"])
