"""-m gpu: the FTLE driver in process on the integer-velocity droplet (overlapping windows against one advect call per
window, the rigid sphere, chunking), and the three `ftle` entry points as fresh child processes, each under its own
timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_FRAMES, S = 6, 32


def _run(args, timeout=300):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return r.stdout.decode()


@pytest.fixture(scope="module")
def droplet():
    """(frames [6,32,32,32], the five ground-truth step flows [5,3,32,32,32]) of the integer-velocity droplet."""
    from opticalflowscivis_amd.data import synthetic
    frames, gt = synthetic.droplet3d_motion(T_FRAMES, S, seed=3, v=(1, -2, 1))
    steps = np.stack([gt(t, t + 1)[0].numpy() for t in range(T_FRAMES - 1)])
    return frames.numpy(), steps


def _core(frame):
    """The nodes of the sphere whose six neighbours are in it too: their whole stencil moves rigidly."""
    m = frame > 0
    core = m.copy()
    for ax in range(3):
        core &= np.roll(m, 1, ax) & np.roll(m, -1, ax)
    core[0], core[-1], core[:, 0], core[:, -1], core[:, :, 0], core[:, :, -1] = (False,) * 6
    return core


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_overlapping_windows_equal_one_advect_call_each(droplet):
    from opticalflowscivis_amd import ops
    from opticalflowscivis_amd.ftle import ftle_series
    frames, steps = droplet
    stack = torch.from_numpy(steps).cuda()
    calls = []

    def source(j0, j1):
        calls.append((j0, j1))
        return stack[j0:j1]

    res = {}
    for chunk in (1, 2, 5):
        del calls[:]
        res[chunk] = ftle_series(source, 5, (S, S, S), window=3, every=1, chunk=chunk)
        assert calls == [(j, min(5, j + chunk)) for j in range(0, 5, chunk)]  # every flow asked for once
    r = res[2]
    assert r["ftle"].shape == (3, S, S, S) and r["cls"].shape == (3, S, S, S) and r["lattice"] == (S, S, S)
    for chunk in (1, 5):  # --chunk does not change a bit
        assert torch.equal(_bits(res[chunk]["ftle"]), _bits(r["ftle"])) and torch.equal(res[chunk]["cls"], r["cls"])
    seeds, lattice, h = ops.lattice_seeds((S, S, S), 1, "cuda")
    for w in range(3):
        pos, status, _ = ops.advect(seeds, stack[w:w + 3])
        want = ops.ftle(pos, status, lattice, h, 3.0)
        assert torch.equal(_bits(r["ftle"][w]), _bits(want["ftle"])) and torch.equal(r["cls"][w], want["cls"])
        row = r["windows"][w]
        assert (row["step"], row["t_from"], row["t_to"], row["frames_spanned"], row["T"]) == (w, w, w + 3, 3, 3.0)
        assert sum(row["counts"].values()) == S ** 3 and row["counts"] == ops.ftle_stats(want["summary"])["counts"]
        assert row["time_advect_s"] > 0 and row["time_ftle_s"] > 0 and row["time_inference_s"] >= 0
        # inside the rigidly moving sphere the map is a translation: exactly 0
        core = _core(frames[w])
        assert core.sum() >= 50
        e, cls = r["ftle"][w].cpu().numpy(), r["cls"][w].cpu().numpy()
        assert (cls[core] == ops.FTLE_OK).all() and (e[core] == 0.0).all()
        assert row["min"] <= 0.0 <= row["max"] and np.isfinite(e[cls == ops.FTLE_OK]).all()
    # windows that do not overlap, a refined lattice, the tensor, dt (Euler: only a particle's own position is sampled)
    r2 = ftle_series(source, 5, (S, S, S), window=2, every=2, refine=2, dt=0.5, with_cg=True)
    L = 2 * S - 1
    assert r2["ftle"].shape == (2, L, L, L) and r2["cg"].shape == (2, 6, L, L, L) and r2["spacing"] == 0.5
    assert [w["step"] for w in r2["windows"]] == [0, 2] and all(w["T"] == 1.0 for w in r2["windows"])
    core2 = np.zeros((L, L, L), bool)
    core2[::2, ::2, ::2] = _core(frames[0])  # the lattice nodes on the grid: their half-step neighbours lie in the core too
    assert (r2["ftle"][0].cpu().numpy()[core2] == 0.0).all()
    assert ftle_series(source, 2, (S, S, S), window=3)["ftle"].shape == (0, S, S, S)  # too short: no window, no flow


def _check_doc(doc, n_windows, nodes):
    assert len(doc["windows"]) == n_windows
    for w in doc["windows"]:
        assert sum(w["counts"].values()) == nodes, w
        assert set(w["counts"]) == {"not_valid", "ok", "ended", "nonfinite", "collapsed"}
        for k in ("frames_spanned", "mean", "std", "min", "max", "time_inference_s", "time_advect_s", "time_ftle_s"):
            assert k in w, k
        assert w["counts"]["ok"] > 0 and w["min"] <= w["max"] and np.isfinite(w["mean"]) and w["std"] >= 0
        assert w["time_advect_s"] > 0 and w["time_ftle_s"] > 0


def _check_fields(out, cls_path, shape, doc):
    e, cls = np.load(out), np.load(cls_path)
    assert e.shape == shape and e.dtype == np.float32 and cls.shape == shape and cls.dtype == np.uint8
    assert np.isfinite(e[cls == 1]).all() and np.isnan(e[cls != 1]).all()
    for w, row in enumerate(doc["windows"]):
        assert row["counts"]["ok"] == int((cls[w] == 1).sum())
    return e, cls


def test_flow3d_ftle_through_given_flows(tmp_path, droplet):
    frames, steps = droplet
    np.save(str(tmp_path / "steps.npy"), steps)
    out, cl, rep = (str(tmp_path / n) for n in ("ftle.npy", "cls.npy", "r.json"))
    _run(["-m", "opticalflowscivis_amd.flow3d.ftle", "--flows", str(tmp_path / "steps.npy"), "--window", "3", "--every",
          "2", "--dt", "0.5", "--chunk", "2", "--out", out, "--classes", cl, "--json", rep])
    doc = json.load(open(rep))
    _check_doc(doc, 2, S ** 3)
    assert doc["model"] is None and doc["frames"] == [0, 1, 2, 3, 4, 5] and doc["lattice"] == [S, S, S]
    assert [(w["t_from"], w["t_to"], w["frames_spanned"], w["T"]) for w in doc["windows"]] == [(0, 3, 3, 1.5), (2, 5, 3, 1.5)]
    e, cls = _check_fields(out, cl, (2, S, S, S), doc)
    for w, t in enumerate((0, 2)):
        core = _core(frames[t])
        assert (cls[w][core] == 1).all() and (e[w][core] == 0.0).all()


def test_flow2d_ftle_with_the_model(tmp_path):
    out, cl, rep = (str(tmp_path / n) for n in ("ftle.npy", "cls.npy", "r.json"))
    so = _run(["-m", "opticalflowscivis_amd.flow2d.ftle", "--dataset", "droplet2d", "--size", "32", "32", "--frames", "6",
               "--window", "2", "--refine", "2", "--direction", "bwd", "--method", "rk4", "--accept-out", "--out", out,
               "--classes", cl, "--json", rep, "--model", str(tmp_path / "none")])
    assert "random-init" in so
    doc = json.load(open(rep))
    _check_doc(doc, 2, 63 * 63)
    assert doc["frames"] == [4, 3, 2, 1] and doc["direction"] == "bwd" and doc["accept_out"] is True
    assert [(w["t_from"], w["t_to"], w["frames_spanned"]) for w in doc["windows"]] == [(4, 2, 2), (3, 1, 2)]
    _check_fields(out, cl, (2, 63, 63), doc)


def test_upflow_ftle(tmp_path):
    out, cl, rep = (str(tmp_path / n) for n in ("ftle.npy", "cls.npy", "r.json"))
    _run(["-m", "opticalflowscivis_amd.upflow.ftle", "--dataset", "rectangle2d", "--frames", "4", "--window", "2",
          "--out", out, "--classes", cl, "--json", rep, "--model", str(tmp_path / "none")])
    doc = json.load(open(rep))
    H, W = doc["shape"]
    _check_doc(doc, 2, H * W)
    assert doc["frames"] == [0, 1, 2, 3] and [w["t_to"] for w in doc["windows"]] == [2, 3]
    _check_fields(out, cl, (2, H, W), doc)
