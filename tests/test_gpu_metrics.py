"""-m gpu: ops.frame_metrics (fs_frame_metrics{2,3}d) against the fp64 restatement in tests/metrics_ref.py, and the
error.py drop-in on 255-range sequences.  Tolerances: |dSSIM| <= 2e-6 per frame, |dPSNR| <= 1e-4 dB."""
import numpy as np
import pytest
import torch

import metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_SSIM, TOL_PSNR = 2e-6, 1e-4


def _field(kind, shape, rng):
    """One frame / volume in [0, 1] of a data kind."""
    nd = len(shape)
    grids = np.meshgrid(*[np.linspace(0, 1, s) for s in shape], indexing="ij")
    if kind == "constant":
        return np.full(shape, 0.37)
    if kind == "droplet":
        c = rng.uniform(0.3, 0.7, nd)
        return (sum((g - ci) ** 2 for g, ci in zip(grids, c)) < rng.uniform(0.05, 0.1)).astype(np.float64)
    if kind in ("jets", "jets_noise"):
        f = np.zeros(shape)
        for _ in range(4):
            c, s = rng.uniform(0.2, 0.8, nd), rng.uniform(0.05, 0.15, nd)
            f += np.exp(-0.5 * sum(((g - ci) / si) ** 2 for g, ci, si in zip(grids, c, s)))
        f = f / f.max()
        if kind == "jets_noise":
            f = np.clip(f + 0.05 * rng.standard_normal(shape), 0, 1)
        return f
    if kind == "noise":
        return rng.random(shape)
    if kind == "offset":
        return 0.9 + 1e-3 * rng.random(shape)
    raise ValueError(kind)


def _pair(kind, n, c, sp, seed):
    rng = np.random.default_rng(seed)
    a = np.stack([np.stack([_field(kind, sp, rng) for _ in range(c)]) for _ in range(n)])
    if kind == "constant":
        b = np.full_like(a, 0.41)
    elif kind == "offset":
        b = a + 1e-3 * (rng.random(a.shape) - 0.5)
    else:
        b = np.clip(a + 0.1 * (rng.random(a.shape) - 0.5) * (1 + np.roll(a, 3, axis=-1)), 0, 1)
    return a.astype(np.float32), b.astype(np.float32)


def _check(a, b, nd, L=1.0):
    from opticalflowscivis_amd import ops
    p, s = ops.frame_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), L, "%dd" % nd)
    assert p.dtype == torch.float64 and s.dtype == torch.float64 and p.shape == (a.shape[0],)
    pr, sr = ref.frame_metrics(a, b, L, nd)
    p, s = p.cpu().numpy(), s.cpu().numpy()
    assert np.abs(s - sr).max() <= TOL_SSIM, (np.abs(s - sr).max(), s[:4], sr[:4])
    fin = np.isfinite(pr)
    assert np.array_equal(np.isfinite(p), fin)
    assert np.abs(p[fin] - pr[fin]).max(initial=0) <= TOL_PSNR, (p[:4], pr[:4])
    return p, s


KINDS = ["constant", "droplet", "jets", "jets_noise", "noise", "offset"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,c,h,w", [(3, 1, 11, 11), (2, 3, 37, 53), (4, 1, 11, 40), (2, 1, 29, 11),
                                     (64, 1, 40, 56), (5, 3, 160, 224)])
def test_frame_metrics_2d(kind, n, c, h, w):
    a, b = _pair(kind, n, c, (h, w), seed=h * 1000 + w + c)
    _check(a, b, 2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,c,sp", [(2, 1, (11, 11, 11)), (1, 1, (11, 27, 19)), (2, 1, (33, 24, 40)),
                                    (1, 1, (96, 128, 160)), (1, 2, (13, 30, 21))])
def test_frame_metrics_3d(kind, n, c, sp):
    if sp == (96, 128, 160) and kind not in ("jets_noise", "offset", "droplet"):
        pytest.skip("large volume: three kinds suffice")
    a, b = _pair(kind, n, c, sp, seed=sum(sp) + c)
    _check(a, b, 3)


def test_identical_and_deterministic():
    from opticalflowscivis_amd import ops
    x = torch.rand(3, 2, 45, 67, device=DEV)
    p, s = ops.frame_metrics(x, x.clone())
    assert torch.all(torch.isinf(p)) and torch.all(p > 0)
    assert float((s - 1).abs().max()) <= 1e-7
    v = torch.rand(2, 1, 40, 36, 52, device=DEV)
    p, s = ops.frame_metrics(v, v.clone(), window="3d")
    assert torch.all(torch.isinf(p)) and float((s - 1).abs().max()) <= 1e-7
    y = torch.rand_like(v)
    r1 = ops.frame_metrics(v, y, window="3d")
    r2 = ops.frame_metrics(v, y, window="3d")
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    z = torch.rand_like(x)
    assert all(torch.equal(u, w) for u, w in zip(ops.frame_metrics(x, z), ops.frame_metrics(x, z)))


def test_non_contiguous_and_layouts():
    from opticalflowscivis_amd import ops
    x = torch.rand(4, 30, 3, 50, device=DEV).permute(0, 2, 1, 3)  # [4,3,30,50], not contiguous
    y = torch.rand(4, 3, 30, 50, device=DEV)
    got = ops.frame_metrics(x, y)
    want = ops.frame_metrics(x.contiguous(), y)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    g1 = ops.frame_metrics(y[:, 0], x[:, 0])                 # [N,H,W] = one channel
    g2 = ops.frame_metrics(y[:, :1], x[:, :1])
    assert torch.equal(g1[1], g2[1])
    with pytest.raises(ValueError):
        ops.frame_metrics(y, y[:, :, :10])


def test_error_dropin_on_uint8_sequence():
    from opticalflowscivis_amd import error
    rng = np.random.default_rng(7)
    base = np.stack([_field("jets", (48, 64), rng) for _ in range(9)])
    orig = (base * 255).round().astype(np.uint8)
    interp = np.clip(orig.astype(np.int16) + rng.integers(-6, 7, orig.shape), 0, 255).astype(np.uint8)
    interp[::4] = orig[::4]
    pr, sr = ref.frame_metrics(orig[:, None], interp[:, None], 255.0, 2)
    mid = [i for i in range(9) if i % 4 != 0]
    p, s = error.calculate_metrics(orig, interp, 4)
    assert abs(p - np.mean(pr[mid])) <= TOL_PSNR and abs(s - np.mean(sr[mid])) <= TOL_SSIM
    # one frame, the reference's formula (20 log10(255 / sqrt(mse))) and shapes
    assert abs(error.calculate_psnr(orig[1], interp[1]) - pr[1]) <= TOL_PSNR
    assert error.calculate_psnr(orig[0], interp[0]) == float("inf")
    assert abs(error.calculate_ssim(orig[1], interp[1]) - sr[1]) <= TOL_SSIM
    rgb1 = np.stack([orig[1], orig[2], orig[3]], -1)
    rgb2 = np.stack([interp[1], interp[2], interp[3]], -1)
    assert abs(error.calculate_ssim(rgb1, rgb2) - np.mean(sr[1:4])) <= TOL_SSIM
    assert abs(error.calculate_ssim(orig[1][..., None], interp[1][..., None]) - sr[1]) <= TOL_SSIM
    sel = error.select_timesteps(orig, interp, 4)
    thr = np.mean(pr[mid]) - np.mean(pr[mid]) / 10
    assert sel == [i for i in mid if pr[i] < thr]
    # volumes: [T,D,H,W] takes the 3-D window
    vol = (np.stack([_field("jets", (12, 20, 16), rng) for _ in range(3)]) * 255).astype(np.float32)
    vol2 = np.clip(vol + rng.normal(0, 4, vol.shape), 0, 255).astype(np.float32)
    pv, sv = ref.frame_metrics(vol[:, None], vol2[:, None], 255.0, 3)
    p, s = error.calculate_metrics(vol, vol2, 2)
    assert abs(p - pv[1]) <= TOL_PSNR and abs(s - sv[1]) <= TOL_SSIM
