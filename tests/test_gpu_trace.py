"""-m gpu: the `trace` entry points as fresh child processes (each under its own timeout) -- traced with a
random-initialised model, traced through given flows with a known answer, the 2-D models and the backward direction --
and the driver's chunking in process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=300):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return r.stdout.decode()


def _check_report(doc, frames, P):
    assert doc["frames"] == frames and doc["n_particles"] == P and len(doc["steps"]) == len(frames) - 1
    for j, s in enumerate(doc["steps"]):
        assert (s["step"], s["t_from"], s["t_to"]) == (j + 1, frames[j], frames[j + 1])
        assert s["alive"] + s["out"] + s["nonfinite"] == P, s
    alive = [s["alive"] for s in doc["steps"]]
    assert alive == sorted(alive, reverse=True)  # nothing comes back
    assert doc["time_inference_s"] >= 0 and doc["time_advect_s"] > 0


def test_flow3d_trace_with_the_model(tmp_path):
    from opticalflowscivis_amd.stepflows import step_chain
    out, rep = str(tmp_path / "traj.npy"), str(tmp_path / "r.json")
    so = _run(["-m", "opticalflowscivis_amd.flow3d.trace", "--dataset", "droplet3d", "--size", "32", "--frames", "7",
               "--seed-grid", "4", "--out", out, "--json", rep, "--model", str(tmp_path / "none")])
    assert "random-init" in so
    chain = step_chain(7, 2, "fwd")
    frames = [chain[0][0]] + [c[1] for c in chain]
    assert frames == [1, 2, 3, 4, 5]
    traj = np.load(out)
    P = 8 ** 3
    assert traj.shape == (len(frames), P, 3) and traj.dtype == np.float32
    assert traj[0, 1].tolist() == [4, 0, 0] and traj[0, -1].tolist() == [28, 28, 28]  # (x, y, z), x fastest
    doc = json.load(open(rep))
    _check_report(doc, frames, P)
    drift = doc["drift"]["steps"]
    assert [d["step"] for d in drift] == [1, 2, 3, 4] and [d["t"] for d in drift] == frames[1:]
    for d in drift:
        assert 0 < d["n"] <= P and 0 <= d["mean"] <= d["max"] and np.isfinite(d["max"])
    assert np.isfinite(traj).all()


def _droplet_steps(tmp_path):
    """The ground-truth steps of the integer-velocity droplet as a [5,3,32,32,32] stack and as per-frame velocities."""
    from opticalflowscivis_amd.data import synthetic
    T, S = 6, 32
    frames, gt = synthetic.droplet3d_motion(T, S, seed=3, v=(1, -2, 1))
    steps = np.stack([gt(t, t + 1)[0].numpy() for t in range(T - 1)])
    np.save(str(tmp_path / "gt_steps.npy"), steps)
    np.save(str(tmp_path / "vel.npy"), np.concatenate([steps, steps[-1:]]))  # gt(a, a + 1) = vel[a]
    return frames, gt, steps


def test_flow3d_trace_through_given_flows(tmp_path):
    """The same kernel through the same flows twice: drift 0; the dense map equals gt(0, 5) on the sphere."""
    frames, gt, steps = _droplet_steps(tmp_path)
    S = 32
    rep, mp = str(tmp_path / "r.json"), str(tmp_path / "map.npy")
    _run(["-m", "opticalflowscivis_amd.flow3d.trace", "--flows", str(tmp_path / "gt_steps.npy"), "--gt",
          str(tmp_path / "vel.npy"), "--seed-grid", "1", "--map-out", mp, "--json", rep, "--chunk", "2"])
    doc = json.load(open(rep))
    _check_report(doc, [0, 1, 2, 3, 4, 5], S ** 3)
    assert doc["model"] is None
    m = np.load(mp)
    inside = frames[0].numpy() > 0
    assert m.shape == (3, S, S, S) and inside.sum() >= 100
    np.testing.assert_array_equal(m[:, inside], gt(0, 5)[0].numpy()[:, inside])
    # --map-out records nothing per step: the drift of the last step alone
    assert [d["step"] for d in doc["drift"]["steps"]] == [5]
    assert all(d["mean"] == 0.0 and d["max"] == 0.0 and d["n"] > 0 for d in doc["drift"]["steps"])


def test_flow3d_trace_through_a_flow_directory(tmp_path):
    """A directory as --save-flows writes it, chained from --start; recorded, so the drift (0 again) is per step; the
    trajectories are those of the driver run in process on the stack's tail."""
    from opticalflowscivis_amd import ops
    from opticalflowscivis_amd.trace import trace_series
    _, _, steps = _droplet_steps(tmp_path)
    fdir = tmp_path / "flows"
    fdir.mkdir()
    for t in range(5):
        np.save(str(fdir / ("flow_%03d_to_%03d.npy" % (t, t + 1))), steps[t])
        np.save(str(fdir / ("flow_%03d_to_%03d.npy" % (t + 1, t))), -steps[t])
    rep = str(tmp_path / "r.json")
    _run(["-m", "opticalflowscivis_amd.flow3d.trace", "--flows", str(fdir), "--start", "2", "--gt", str(tmp_path / "vel.npy"),
          "--seed-grid", "4", "--method", "rk4", "--substeps", "2", "--out", str(tmp_path / "a.npy"), "--json", rep])
    doc = json.load(open(rep))
    _check_report(doc, [2, 3, 4, 5], 8 ** 3)
    assert [d["step"] for d in doc["drift"]["steps"]] == [1, 2, 3]
    assert all(d["mean"] == 0.0 and d["max"] == 0.0 and d["n"] > 0 for d in doc["drift"]["steps"])
    a = np.load(str(tmp_path / "a.npy"))
    assert a.shape == (4, 8 ** 3, 3)
    tail = torch.from_numpy(steps[2:].copy()).to("cuda")
    want = trace_series(lambda j0, j1: tail[j0:j1], 3, ops.grid_seeds((32, 32, 32), 4, 0, "cuda"), method="rk4", substeps=2)
    np.testing.assert_array_equal(a.view(np.uint32), want["traj"].permute(0, 2, 1).contiguous().cpu().numpy().view(np.uint32))


def test_flow2d_trace_backward(tmp_path):
    from opticalflowscivis_amd.stepflows import step_chain
    out, rep = str(tmp_path / "traj.npy"), str(tmp_path / "r.json")
    _run(["-m", "opticalflowscivis_amd.flow2d.trace", "--dataset", "droplet2d", "--size", "64", "96", "--frames", "6",
          "--seed-grid", "8", "--direction", "bwd", "--method", "rk2", "--substeps", "2", "--out", out, "--json", rep,
          "--model", str(tmp_path / "none")])
    chain = step_chain(6, 2, "bwd")
    frames = [chain[0][0]] + [c[1] for c in chain]
    assert frames == [4, 3, 2, 1]
    P = 8 * 12
    assert np.load(out).shape == (4, P, 2)
    doc = json.load(open(rep))
    _check_report(doc, frames, P)
    assert doc["direction"] == "bwd" and [d["t"] for d in doc["drift"]["steps"]] == [3, 2, 1]


def test_upflow_trace_backward(tmp_path):
    out, rep = str(tmp_path / "traj.npy"), str(tmp_path / "r.json")
    _run(["-m", "opticalflowscivis_amd.upflow.trace", "--dataset", "rectangle2d", "--frames", "4", "--seed-grid", "16",
          "--direction", "bwd", "--out", out, "--json", rep, "--model", str(tmp_path / "none")])
    assert np.load(out).shape == (4, 64, 2)
    doc = json.load(open(rep))
    _check_report(doc, [3, 2, 1, 0], 64)
    assert len(doc["drift"]["steps"]) == 3


def test_chunking_changes_no_bit():
    from opticalflowscivis_amd import ops
    from opticalflowscivis_amd.trace import step_counts, trace_series
    g = torch.Generator().manual_seed(11)
    K, sp = 6, (6, 7, 9)
    flows = (0.8 * torch.randn((K, 3) + sp, generator=g)).to("cuda")
    seeds = ops.grid_seeds(sp, 1, 0, "cuda") + 0.25
    calls = []

    def source(j0, j1):
        calls.append((j0, j1))
        return flows[j0:j1]

    res = {}
    for chunk in (1, 4, 6):
        del calls[:]
        res[chunk] = trace_series(source, K, seeds, chunk=chunk, method="rk4", substeps=2)
        assert calls == [(j, min(K, j + chunk)) for j in range(0, K, chunk)]
    for chunk in (4, 6):
        for k in ("traj", "pos", "status", "steps"):
            assert torch.equal(res[1][k].view(torch.int32) if res[1][k].dtype == torch.float32 else res[1][k],
                               res[chunk][k].view(torch.int32) if res[chunk][k].dtype == torch.float32 else res[chunk][k]), k
    r = res[1]
    assert r["traj"].shape == (K + 1, 3, seeds.shape[1]) and torch.equal(r["traj"][0], seeds) and torch.equal(r["traj"][-1], r["pos"])
    counts = step_counts(r["status"], r["steps"], K)
    assert all(sum(c) == seeds.shape[1] for c in counts) and 0 < counts[-1][0] < seeds.shape[1] and counts[-1][1] > 0
    unrec = trace_series(source, K, seeds, chunk=4, method="rk4", substeps=2, record=False)
    assert unrec["traj"] is None and torch.equal(unrec["pos"], r["pos"]) and torch.equal(unrec["steps"], r["steps"])
