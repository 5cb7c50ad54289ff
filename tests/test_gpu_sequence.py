"""-m gpu: sequence interpolation (opticalflowscivis_amd.evaluate.interpolate_sequence), the `evaluate` entry points
and `inference_img --ratio` as fresh child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _model(nd, seed=3):
    from opticalflowscivis_amd.flow3d.model.RIFE import Model as M3
    from opticalflowscivis_amd.flow2d.model.RIFE import Model as M2
    torch.manual_seed(seed)
    m = (M3 if nd == 3 else M2)(local_rank=-1, device=DEV)
    m.eval()
    return m


def _infer(m, a, b):
    with torch.no_grad():
        r = m.inference(a, b)[0]
    return r[2] if isinstance(r, list) else r


def _pad(x, nd):
    pad = []
    for s in reversed(x.shape[-nd:]):
        pad += [0, ((s - 1) // 32 + 1) * 32 - s]
    return torch.nn.functional.pad(x, pad)


@pytest.mark.parametrize("nd,sp", [(3, (32, 32, 32)), (3, (40, 48, 64)), (2, (72, 100))])
def test_interpolate_sequence(nd, sp):
    from opticalflowscivis_amd.evaluate import interpolate_sequence
    m = _model(nd)
    seq = torch.rand((9,) + sp, generator=torch.Generator().manual_seed(1)).to(DEV)
    out1 = interpolate_sequence(m, seq, 4, batch=1)
    out3 = interpolate_sequence(m, seq, 4, batch=3)
    assert out1.shape == seq.shape and out3.shape == seq.shape
    assert torch.equal(out1[::4], seq[::4]) and torch.equal(out3[::4], seq[::4])
    assert float((out1 - out3).abs().max()) <= 1e-5
    # level 1: midpoints 2, 6 of the padded keyframes; level 2: 1, 3, 5, 7 from the padded level-1 results
    cut = (slice(None), 0) + tuple(slice(0, s) for s in sp)
    k = _pad(seq[::4].unsqueeze(1), nd)
    m2 = _infer(m, k[:2], k[1:3])                            # positions 2, 6
    np.testing.assert_allclose(out1[[2, 6]].cpu().numpy(), m2[cut].cpu().numpy(), rtol=0, atol=1e-5)
    m1 = _infer(m, k[0:1], m2[0:1])                          # position 1
    m7 = _infer(m, m2[1:2], k[2:3])                          # position 7
    np.testing.assert_allclose(out1[1].cpu().numpy(), m1[cut][0].cpu().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(out3[7].cpu().numpy(), m7[cut][0].cpu().numpy(), rtol=0, atol=1e-5)
    # a sequence whose length is not (K-1)*factor + 1 keeps the frames up to its last keyframe
    assert interpolate_sequence(m, seq[:8], 4, batch=2).shape[0] == 5


def _run(args, timeout=900):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return r.stdout.decode()


@pytest.mark.parametrize("nd", [3, 2])
def test_evaluate_cli(tmp_path, nd):
    from opticalflowscivis_amd.data import synthetic
    from opticalflowscivis_amd.evaluate import interpolate_sequence, linear_baseline
    if nd == 3:
        seq = synthetic.jets3d_sequence(9, 32, seed=5)
    else:
        seq = synthetic.droplet2d_sequence(9, 64, 72, seed=5)
    p = str(tmp_path / "seq.npy")
    np.save(p, seq.numpy())
    m = _model(nd, seed=0)
    m.save_model("flownet.pkl", str(tmp_path))
    out = str(tmp_path / "r.json")
    so = _run(["-m", "opticalflowscivis_amd.flow%dd.evaluate" % nd, "--seq", p, "--exp", "1", "2", "--batch", "2",
               "--model", str(tmp_path), "--baseline", "--out", out])
    assert "random-init" not in so and "factor   2" in so
    doc = json.load(open(out))
    assert doc["shape"] == list(seq.shape) and [r["factor"] for r in doc["results"]] == [2, 4]
    for r in doc["results"]:
        f = r["factor"]
        for key in ("psnr", "ssim", "psnr_mean", "ssim_mean"):
            assert key in r["model"] and key in r["baseline"]
        assert len(r["model"]["psnr"]) == r["frames"] == 9
        for v in (r["model"]["psnr_mean"], r["model"]["ssim_mean"], r["baseline"]["psnr_mean"],
                  r["baseline"]["ssim_mean"], r["threshold"], r["time_inference_s"], r["time_metrics_s"]):
            assert np.isfinite(v)
        assert all(np.isinf(r["model"]["psnr"][i]) for i in range(0, 9, f))  # keyframes are exact
        mid = [i for i in range(9) if i % f != 0]
        thr = np.mean([r["model"]["psnr"][i] for i in mid]) * 0.9
        assert abs(r["threshold"] - thr) < 1e-9
        assert r["selected"] == [i for i in mid if r["model"]["psnr"][i] < r["threshold"]]
        # the model's frames rebuilt here with the same weights, scored by the fp64 restatement
        pred = interpolate_sequence(m, seq.to(DEV), f, batch=1).cpu().numpy()
        pr, sr = ref.frame_metrics(pred[:, None], seq.numpy()[:, None], 1.0, nd)
        assert abs(r["model"]["psnr_mean"] - np.mean(pr[mid])) < 1e-3
        assert abs(r["model"]["ssim_mean"] - np.mean(sr[mid])) < 1e-5
        # the baseline against the restatement; at factor 2 it is the reference's blend t k0 + (1 - t) k1
        base = linear_baseline(seq, f).numpy()
        pr, sr = ref.frame_metrics(base[:, None], seq.numpy()[:, None], 1.0, nd)
        assert abs(r["baseline"]["psnr_mean"] - np.mean(pr[mid])) < 1e-4
        assert abs(r["baseline"]["ssim_mean"] - np.mean(sr[mid])) < 2e-6
        if f == 2:
            k = seq.numpy()[::2]
            theirs = 0.5 * k[:-1] + (1 - 0.5) * k[1:]
            np.testing.assert_array_equal(base[1::2], theirs)


@pytest.mark.parametrize("nd", [3, 2])
def test_inference_img_ratio(tmp_path, nd):
    from opticalflowscivis_amd.data import synthetic
    if nd == 3:
        d = synthetic.droplet3d_batch(1, 40, seed=3)
    else:
        d = synthetic.droplet2d_batch(1, 72, 100, seed=3, radius=(8, 16))
    a, b = str(tmp_path / "a.npy"), str(tmp_path / "b.npy")
    np.save(a, d[0, 0].numpy())
    np.save(b, d[0, 1].numpy())
    m = _model(nd, seed=11)
    m.save_model("flownet.pkl", str(tmp_path))
    mod = "opticalflowscivis_amd.flow%dd.inference_img" % nd
    o1 = str(tmp_path / "o1")
    _run(["-m", mod, "--img", a, b, "--ratio", "0.25", "--model", str(tmp_path), "--out", o1])
    f = [np.load(os.path.join(o1, "img%d.npy" % i)) for i in range(3)]
    assert not os.path.exists(os.path.join(o1, "img3.npy"))
    np.testing.assert_array_equal(f[0], d[0, 0].numpy())
    np.testing.assert_array_equal(f[2], d[0, 1].numpy())
    x, y = _pad(d[:, 0:1].to(DEV), nd), _pad(d[:, 1:2].to(DEV), nd)
    half = _infer(m, x, y)                                   # ratio 0.5
    quarter = _infer(m, x, half)                             # ratio 0.25: two bisection steps
    cut = (0, 0) + tuple(slice(0, s) for s in d.shape[2:])
    assert float(np.abs(f[1] - quarter[cut].cpu().numpy()).max()) < 1e-5
    o2 = str(tmp_path / "o2")
    _run(["-m", mod, "--img", a, b, "--ratio", "0.01", "--model", str(tmp_path), "--out", o2])
    np.testing.assert_array_equal(np.load(os.path.join(o2, "img1.npy")), d[0, 0].numpy())
