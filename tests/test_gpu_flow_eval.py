"""GPU: the flow-evaluation entry points (flow2d / flow3d evaluate_flow, upflow test) run as child processes at small
sizes and write JSON with the documented keys; the zero-flow baseline equals the mean ground-truth magnitude."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = {"epe", "epe_noc", "epe_occ", "rmse", "ae_deg", "fl", "fl_noc", "fl_occ", "max_epe", "n_valid", "n_noc",
         "n_nonfinite"}


def _run(args, timeout=900):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return r.stdout.decode()


def _mean_gt_magnitude(gt, t_from, t_to):
    """Mean |displacement| over the valid elements, fp64, on the CPU."""
    disp, valid, _ = gt(t_from, t_to)
    mag = torch.sqrt((disp.double().cpu() ** 2).sum(0))
    return float(mag[valid.cpu()].mean())


def _check_doc(doc, names, n_pairs):
    for k in ("sequence", "shape", "gap", "batch", "model", "convention", "pairs", "mean", "zero_baseline",
              "time_inference_s", "time_metrics_s"):
        assert k in doc, k
    assert set(doc["mean"]) == STATS and set(doc["zero_baseline"]["mean"]) == STATS
    assert len(doc["pairs"]) == n_pairs
    for p in doc["pairs"]:
        assert set(p["flows"]) == set(names)
        for f in p["flows"].values():
            assert STATS <= set(f) and "t_from" in f and "t_to" in f
            assert np.isfinite(f["epe"]) and f["n_valid"] > 0
    assert doc["time_inference_s"] > 0 and doc["time_metrics_s"] > 0


def test_flow2d_evaluate_flow_cli(tmp_path):
    from opticalflowscivis_amd.data import synthetic
    out = tmp_path / "r2.json"
    stdout = _run(["-m", "opticalflowscivis_amd.flow2d.evaluate_flow", "--dataset", "droplet2d", "--size", "64", "96",
                   "--frames", "5", "--gap", "2", "--batch", "2", "--zero-baseline", "--model", str(tmp_path / "none"),
                   "--save-flows", str(tmp_path / "flows"), "--out", str(out)])
    assert "random-init" in stdout and "EPE" in stdout
    doc = json.load(open(out))
    _check_doc(doc, ("mid->t0", "mid->t1"), 3)
    assert doc["convention"] == "disp" and doc["shape"] == [5, 64, 96]
    assert len(os.listdir(tmp_path / "flows")) == 6
    _, gt = synthetic.droplet2d_motion(5, 64, 96, 1234)
    zb = doc["zero_baseline"]["flows"]
    targets = [(1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (3, 4)]
    for z, (a, b) in zip(zb, targets):
        assert z["epe"] == pytest.approx(_mean_gt_magnitude(gt, a, b), rel=1e-6)
    for i, p in enumerate(doc["pairs"]):
        assert (p["t0"], p["t1"]) == (i, i + 2)
        assert (p["flows"]["mid->t0"]["t_from"], p["flows"]["mid->t0"]["t_to"]) == (i + 1, i)


def test_flow3d_evaluate_flow_cli(tmp_path):
    from opticalflowscivis_amd.data import synthetic
    out = tmp_path / "r3.json"
    _run(["-m", "opticalflowscivis_amd.flow3d.evaluate_flow", "--dataset", "jets3d", "--size", "32", "--frames", "4",
          "--gap", "2", "--zero-baseline", "--model", str(tmp_path / "none"), "--out", str(out)])
    doc = json.load(open(out))
    _check_doc(doc, ("mid->t0", "mid->t1"), 2)
    assert doc["convention"] == "disp" and doc["model_flow"].startswith("rife3d")
    _, gt = synthetic.jets3d_motion(4, 32, 1234)
    assert doc["zero_baseline"]["flows"][3]["epe"] == pytest.approx(_mean_gt_magnitude(gt, 2, 3), rel=1e-6)
    assert doc["zero_baseline"]["mean"]["epe"] == pytest.approx(
        np.mean([_mean_gt_magnitude(gt, a, b) for a, b in ((1, 0), (1, 2), (2, 1), (2, 3))]), rel=1e-6)


def test_upflow_test_cli(tmp_path):
    from opticalflowscivis_amd.data import synthetic
    out = tmp_path / "ru.json"
    _run(["-m", "opticalflowscivis_amd.upflow.test", "--dataset", "rectangle2d", "--frames", "4", "--gap", "1",
          "--batch", "2", "--zero-baseline", "--model", str(tmp_path / "none"), "--out", str(out)])
    doc = json.load(open(out))
    _check_doc(doc, ("t0->t1", "t1->t0"), 3)
    _, gt = synthetic.rectangle2d_motion(4)
    for z, (a, b) in zip(doc["zero_baseline"]["flows"], [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2)]):
        assert z["epe"] == pytest.approx(_mean_gt_magnitude(gt, a, b), rel=1e-6)


def test_flow2d_cli_with_user_sequence(tmp_path):
    """--seq / --gt: a user's frames and per-frame velocities (gt(a, b) = velocity[a] (b - a))."""
    from opticalflowscivis_amd.data import synthetic
    frames, gt = synthetic.droplet2d_motion(5, 64, 64, 7)
    vel = torch.stack([gt(t, t + 1)[0] for t in range(5)])
    np.save(tmp_path / "seq.npy", frames.numpy())
    np.save(tmp_path / "vel.npy", vel.numpy())
    out = tmp_path / "r.json"
    _run(["-m", "opticalflowscivis_amd.flow2d.evaluate_flow", "--seq", str(tmp_path / "seq.npy"), "--gt",
          str(tmp_path / "vel.npy"), "--gap", "2", "--zero-baseline", "--model", str(tmp_path / "none"), "--out",
          str(out)])
    doc = json.load(open(out))
    _check_doc(doc, ("mid->t0", "mid->t1"), 3)
    m = torch.sqrt((vel[1].double() ** 2).sum(0)).mean()
    assert doc["zero_baseline"]["flows"][0]["epe"] == pytest.approx(float(m), rel=1e-6)


def test_flow3d_cli_with_non_cubic_user_sequence(tmp_path):
    """--seq / --gt in 3-D with extents that are neither equal nor multiples of 32 (the model runs on 32 x 32 x 64):
    the JSON is complete, the zero baseline is the mean |gt|, and the saved displacements are finite and of the
    sequence's extent."""
    g = torch.Generator().manual_seed(3)
    T, sp = 5, (20, 24, 40)
    frames = torch.rand((T,) + sp, generator=g)
    vel = torch.randn((T, 3) + sp, generator=g)
    np.save(tmp_path / "seq.npy", frames.numpy())
    np.save(tmp_path / "vel.npy", vel.numpy())
    out = tmp_path / "r.json"
    _run(["-m", "opticalflowscivis_amd.flow3d.evaluate_flow", "--seq", str(tmp_path / "seq.npy"), "--gt",
          str(tmp_path / "vel.npy"), "--gap", "2", "--batch", "2", "--zero-baseline", "--model", str(tmp_path / "none"),
          "--save-flows", str(tmp_path / "flows"), "--out", str(out)])
    doc = json.load(open(out))
    _check_doc(doc, ("mid->t0", "mid->t1"), 3)
    assert doc["shape"] == [T] + list(sp)
    m = torch.sqrt((vel[1].double() ** 2).sum(0)).mean()
    assert doc["zero_baseline"]["flows"][0]["epe"] == pytest.approx(float(m), rel=1e-6)
    saved = sorted(os.listdir(tmp_path / "flows"))
    assert len(saved) == 6
    f = np.load(tmp_path / "flows" / saved[0])
    assert f.shape == (3,) + sp and np.isfinite(f).all()
