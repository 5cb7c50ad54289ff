"""TEST INFRASTRUCTURE: the 3-D census distance and the first-order flow smoothness restated in plain torch ops
(fp64 unless the operands say otherwise), differentiable by autograd.  Census by padding and shifting: no tiling, no
pair symmetry, no approximated reciprocal -- what csrc/census3d.hip and csrc/flowsmooth3d.hip are held against."""
import torch
import torch.nn.functional as F


def census3d_dist(vol1, vol2, radius):
    """[B,1,D,H,W] x 2 -> [B,1,D,H,W]: sum over the zero-padded (2r+1)^3 neighbourhood of (t1 - t2)^2 / (0.1 +
    (t1 - t2)^2), t = u / sqrt(0.81 + u^2), u = v[neighbour] - v[centre] (UPFlow/utils/loss.py:59-71 on volumes).
    The taps are summed by torch.sum, plane by plane, not added one by one to a running sum: on float32 operands (the
    fp32 oracle of tests/unsup3d_ledger_inputs.py) a border voxel's hundreds of equal padding terms would otherwise be
    rounded the same way each time, an error of the summation order and not of the inputs."""
    r = radius
    D, H, W = vol1.shape[2:]
    p1, p2 = F.pad(vol1, [r] * 6), F.pad(vol2, [r] * 6)
    planes = []
    for dz in range(2 * r + 1):
        taps = []
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                u1 = p1[:, :, dz:dz + D, dy:dy + H, dx:dx + W] - vol1
                u2 = p2[:, :, dz:dz + D, dy:dy + H, dx:dx + W] - vol2
                t1, t2 = u1 / torch.sqrt(0.81 + u1 ** 2), u2 / torch.sqrt(0.81 + u2 ** 2)
                d = (t1 - t2) ** 2
                taps.append(d / (0.1 + d))
        planes.append(torch.stack(taps).sum(0))
    return torch.stack(planes).sum(0)


def census3d_loss(vol1, vol2, radius, q=0.4):
    """mean((|dist| + 0.01)^q) over every voxel (loss.py:44-48)."""
    return (census3d_dist(vol1, vol2, radius).abs() + 0.01).pow(q).mean()


def flow_smooth3d_sums(flow, guide=None, q=0.25, eps=1e-9, kappa=0.0):
    """(S1, number of pairs): S1 = sum over b, c, voxels p and axes a with p + e_a inside of
    exp(-kappa |guide[p + e_a] - guide[p]|) * ((flow[p + e_a] - flow[p])^2 + eps^2)^q."""
    s1, n = flow.new_zeros(()), 0
    for ax in (2, 3, 4):
        m = flow.shape[ax] - 1
        if m < 1:
            continue
        d = flow.narrow(ax, 1, m) - flow.narrow(ax, 0, m)
        pen = (d ** 2 + eps ** 2).pow(q)
        if guide is not None and kappa != 0:
            pen = pen * torch.exp(-kappa * (guide.narrow(ax, 1, m) - guide.narrow(ax, 0, m)).abs())
        s1 = s1 + pen.sum()
        n += d.numel()
    return s1, n


def flow_smooth3d(flow, guide=None, q=0.25, eps=1e-9, kappa=0.0):
    """The mean over the pairs counted (0 for a flow without any)."""
    s1, n = flow_smooth3d_sums(flow, guide, q, eps, kappa)
    return s1 / max(n, 1)


def charbonnier_mean(x, y, q=0.25, eps=1e-9):
    """mean(((x - y)^2 + eps^2)^q): the photometric term of one direction (Flow-3D/model/RIFE.py:147-148)."""
    return ((x - y) ** 2 + eps ** 2).pow(q).mean()
