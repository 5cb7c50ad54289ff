"""-m gpu: the vortex driver in process on an analytic rigid rotation plus translation (the report's numbers against
the closed form, chunking), and the three `vortex` entry points as fresh child processes, each under its own timeout:
their planes and flags against ops.velgrad applied to the step flows they saved."""
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


def _rotation(sp, K):
    """([K, C, *sp] fp32 step flows u = W x (x - c) + t_k with dyadic entries (exact in fp32), |W|^2)."""
    C = len(sp)
    x = np.indices(sp)[::-1].astype(np.float64)
    ctr = np.array([float(s // 2) for s in sp[::-1]]).reshape((C,) + (1,) * C)
    if C == 3:
        w = np.array([0.25, -0.5, 0.75])
        A = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    else:
        w = np.array([0.5])
        A = np.array([[0, -0.5], [0.5, 0]])
    rot = np.einsum("rc,c...->r...", A, x - ctr)
    t = np.array([[0.5 * k, -0.25 * k, 1.0 + k][:C] for k in range(K)]).reshape((K, C) + (1,) * C)
    u = rot[None] + t
    u32 = u.astype(np.float32)
    assert (u32.astype(np.float64) == u).all()
    return u32, float((w * w).sum())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("sp", [(12, 12, 12), (16, 20)], ids=["12x12x12", "16x20"])
def test_rigid_rotation_report_and_chunking(sp, tmp_path):
    from opticalflowscivis_amd import ops
    from opticalflowscivis_amd.vortex import vortex_series
    K, dt = 5, 0.5
    u, w2 = _rotation(sp, K)
    stack = torch.from_numpy(u).cuda()
    calls = []

    def source(j0, j1):
        calls.append((j0, j1))
        return stack[j0:j1]

    frames = [0, 1, 2, 4, 5, 6]  # the third step spans two frames
    res = {}
    for chunk in (2, 5):
        del calls[:]
        res[chunk] = vortex_series(source, K, sp, ops.VG_FIELDS, 1.0, chunk, frames=frames, dt=dt)
        assert calls == [(j, min(K, j + chunk)) for j in range(0, K, chunk)]  # every flow asked for once
    r = res[2]
    C = len(sp)
    assert r["out"].shape == (K, 5 + C * C + (C == 3) * 2) + sp and r["flags"].shape == (K,) + sp
    assert torch.equal(_bits(r["out"]), _bits(res[5]["out"])) and torch.equal(r["flags"], res[5]["flags"])
    for a, b in zip(r["steps"], res[5]["steps"]):  # --chunk does not change a number of the report
        assert a == b
    assert (r["flags"] == 3).all()
    for j, row in enumerate(r["steps"]):
        span = frames[j + 1] - frames[j]
        scale = 1.0 / (span * dt)
        assert (row["step"], row["t_from"], row["t_to"], row["frames_spanned"], row["scale"]) == (j, frames[j], frames[j + 1], span, scale)
        assert row["frac_q_pos"] == 1.0 and row["frac_l2_neg"] == 1.0 and row["frac_both"] == 1.0 and row["n_nonfinite"] == 0
        assert row["rms_div"] == 0.0 and row["div_min"] == 0.0 == row["div_max"]
        want = 2.0 * w2 * scale * scale  # |vort|^2 / 2 with vort = 2 W
        assert abs(row["enstrophy"] - want) <= 1e-6 * want, (row["enstrophy"], want)
        assert abs(row["q_mean"] - w2 * scale * scale) <= 1e-6 * w2 * scale * scale and row["q_std"] <= 1e-6 * want
        assert abs(row["l2_mean"] + w2 * scale * scale) <= 1e-6 * w2 * scale * scale
    assert r["time_kernel_s"] > 0 and r["time_flows_s"] >= 0
    # the same through --flows of the command line (in process: the entry points below run as children)
    from opticalflowscivis_amd import vortex as drv
    np.save(str(tmp_path / "flows.npy"), u)
    out, mask, rep = (str(tmp_path / n) for n in ("vg.npy", "m.npy", "r.json"))
    args = drv.check_args(drv._args(C, "x", "rife").parse_args(
        ["--flows", str(tmp_path / "flows.npy"), "--fields", "div,vort,vmag,q,l2,grad", "--chunk", "2", "--dt", "1.0",
         "--out", out, "--mask", mask, "--json", rep]))
    doc = drv.run(args, C, "rife", None)
    assert doc["model"] is None and doc["frames"] == list(range(K + 1)) and len(doc["steps"]) == K
    assert json.load(open(rep))["steps"][0]["frac_both"] == 1.0
    same = ops.velgrad(stack, ops.VG_FIELDS, 1.0, 1.0)
    assert np.array_equal(np.load(out).view(np.uint32), same["out"].cpu().numpy().view(np.uint32))
    assert np.array_equal(np.load(mask), same["flags"].cpu().numpy())


def _check_entry_point(tmp_path, module, argv, nd, fields, spacing=1.0, dt=1.0):
    """Run one entry point as a child; its files have the documented shapes and equal ops.velgrad on the saved flows."""
    from opticalflowscivis_amd import ops
    out, mask, rep, fl = (str(tmp_path / n) for n in ("vg.npy", "m.npy", "r.json", "flows.npy"))
    so = _run(["-m", module] + argv + ["--out", out, "--mask", mask, "--json", rep, "--save-flows", fl, "--model",
                                       str(tmp_path / "none")])
    doc = json.load(open(rep))
    flows, planes, flags = np.load(fl), np.load(out), np.load(mask)
    K = len(doc["steps"])
    sp = tuple(doc["shape"])
    assert K >= 1 and len(doc["frames"]) == K + 1 and len(sp) == nd
    NP = sum(b - a for a, b in doc["planes"].values())
    assert list(doc["planes"]) == doc["fields"] == [n for n in ops.VG_FIELDS if n in fields.split(",")]
    assert flows.shape == (K, nd) + sp and flows.dtype == np.float32
    assert planes.shape == (K, NP) + sp and planes.dtype == np.float32 and flags.shape == (K,) + sp and flags.dtype == np.uint8
    scales = []
    for j, row in enumerate(doc["steps"]):
        span = abs(doc["frames"][j + 1] - doc["frames"][j])
        assert (row["t_from"], row["t_to"], row["frames_spanned"]) == (doc["frames"][j], doc["frames"][j + 1], span)
        assert row["scale"] == 1.0 / (span * dt) and row["n_finite"] + row["n_nonfinite"] == int(np.prod(sp))
        for k in ("rms_div", "enstrophy", "frac_q_pos", "frac_l2_neg", "frac_both", "div_mean", "q_max"):
            assert k in row, k
        scales.append(row["scale"])
    assert doc["time_kernel_s"] > 0 and doc["time_inference_s"] > 0
    want = ops.velgrad(torch.from_numpy(flows).cuda(), fields, spacing, scales)
    assert np.array_equal(planes.view(np.uint32), want["out"].cpu().numpy().view(np.uint32))
    assert np.array_equal(flags, want["flags"].cpu().numpy())
    stats = ops.velgrad_stats(want["summary"], int(np.prod(sp)))
    for row, st in zip(doc["steps"], stats):
        for k, v in st.items():
            assert row[k] == v or (v != v and row[k] != row[k]), k
    return doc, so


def test_flow3d_vortex_with_the_model(tmp_path):
    doc, so = _check_entry_point(tmp_path, "opticalflowscivis_amd.flow3d.vortex",
                                 ["--dataset", "droplet3d", "--size", "32", "--frames", "5", "--chunk", "2"], 3,
                                 "div,vmag,q,l2")
    assert "random-init" in so and doc["shape"] == [32, 32, 32] and doc["direction"] == "fwd"
    assert all(r["frac_both"] == r["frac_both"] for r in doc["steps"])  # both criteria selected: a number


def test_flow2d_vortex_with_the_model(tmp_path):
    doc, so = _check_entry_point(tmp_path, "opticalflowscivis_amd.flow2d.vortex",
                                 ["--dataset", "droplet2d", "--size", "32", "32", "--frames", "5", "--direction", "bwd",
                                  "--fields", "vort,q,grad", "--spacing", "0.5", "2", "--dt", "0.5"], 2, "vort,q,grad",
                                 spacing=(0.5, 2.0), dt=0.5)
    assert "random-init" in so and doc["direction"] == "bwd" and doc["frames"] == sorted(doc["frames"], reverse=True)
    assert all(r["frac_l2_neg"] != r["frac_l2_neg"] for r in doc["steps"])  # l2 not selected: NaN


def test_upflow_vortex(tmp_path):
    doc, _ = _check_entry_point(tmp_path, "opticalflowscivis_amd.upflow.vortex",
                                ["--dataset", "rectangle2d", "--frames", "4"], 2, "div,vmag,q,l2")
    assert doc["frames"] == [0, 1, 2, 3]
