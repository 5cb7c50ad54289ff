"""CPU: the fp64 restatement of the sequence metrics (tests/metrics_ref.py), the shape rules of the error.py drop-in,
the time-step selection, the argument checks of fs_frame_metrics{2,3}d and their compile-time resources."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticalflowscivis_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_taps_are_get_gaussian_kernel():
    g = ref.gaussian_taps()
    i = np.arange(11)
    want = np.exp(-((i - 5) ** 2) / 4.5)
    np.testing.assert_allclose(g, want / want.sum(), rtol=0, atol=1e-16)
    assert abs(g.sum() - 1) < 1e-15 and g[5] == g.max()


@pytest.mark.parametrize("nd,shape", [(2, (2, 13, 17)), (2, (11, 11)), (3, (12, 11, 14)), (3, (11, 11, 11))])
def test_separable_equals_direct_window(nd, shape):
    a = np.random.default_rng(3).random(shape)
    axes = tuple(range(len(shape) - nd, len(shape)))
    np.testing.assert_allclose(ref.filter_valid(a, axes), ref.filter_valid_direct(a, nd), rtol=0, atol=1e-14)


def test_identity_gives_one_and_inf():
    x = np.random.default_rng(1).random((2, 3, 20, 24))
    p, s = ref.frame_metrics(x, x, 1.0, 2)
    assert np.all(np.isinf(p)) and np.all(p > 0)
    np.testing.assert_allclose(s, 1.0, atol=1e-15)
    v = np.random.default_rng(2).random((1, 1, 12, 13, 14)) * 255
    p, s = ref.frame_metrics(v, v, 255.0, 3)
    assert np.isinf(p[0]) and abs(s[0] - 1) < 1e-15


def test_error_dropin_shape_rules_without_gpu():
    from opticalflowscivis_amd import error
    with pytest.raises(ValueError, match="same dimensions"):
        error.calculate_ssim(np.zeros((20, 20)), np.zeros((20, 21)))
    with pytest.raises(ValueError, match="Wrong input image dimensions"):
        error.calculate_ssim(np.zeros((2, 20, 20, 3)), np.zeros((2, 20, 20, 3)))
    with pytest.raises(ValueError, match="Wrong input image dimensions"):
        error.calculate_ssim(np.zeros(20), np.zeros(20))
    assert error.calculate_ssim(np.zeros((20, 20, 4)), np.zeros((20, 20, 4))) is None  # error.py:67-74 falls through
    with pytest.raises(ValueError, match="same dimensions"):
        error.calculate_psnr(np.zeros((20, 20)), np.zeros((21, 20)))
    # frame layouts: H x W, H x W x C (cv2, C in 1, 3), D x H x W
    assert error._frames(np.zeros((4, 20, 30, 3)))[0].shape == (4, 3, 20, 30)
    assert error._frames(np.zeros((4, 20, 30)))[0].shape == (4, 1, 20, 30)
    assert error._frames(np.zeros((4, 12, 20, 30)))[1] == "3d"


def test_ops_refuse_cpu_tensors():
    import torch
    from opticalflowscivis_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.frame_metrics(torch.rand(2, 1, 16, 16), torch.rand(2, 1, 16, 16))


def test_select_from_psnr():
    from opticalflowscivis_amd.error import select_from_psnr
    psnr = [float("inf"), 30.0, 20.0, float("inf"), 40.0, 25.0, float("inf")]
    idx, thr = select_from_psnr(psnr, 3)
    m = (30 + 20 + 40 + 25) / 4
    assert thr == m - m / 10 and idx == [2, 5]                # error.py:133, 140-145: only i % factor != 0
    assert select_from_psnr(psnr, 3, threshold=35.0) == ([1, 2, 5], 35.0)
    assert select_from_psnr([50.0, 10.0, 50.0], 2) == ([], 9.0)


def test_frame_metrics_argument_errors_without_gpu():
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    assert L.fs_frame_metrics2d(None, None, 1, 1, 16, 16, 1.0, None, None, None, None) == 1       # NULLPTR
    assert L.fs_frame_metrics2d(1, 1, 1, 1, 16, 16, 1.0, 1, None, 1, None) == 1
    assert L.fs_frame_metrics3d(1, None, 1, 1, 16, 16, 16, 1.0, 1, 1, 1, None) == 1
    assert L.fs_frame_metrics2d(1, 1, 1, 1, 10, 16, 1.0, 1, 1, 1, None) == 2                      # SHAPE: H < 11
    assert L.fs_frame_metrics2d(1, 1, 1, 1, 16, 10, 1.0, 1, 1, 1, None) == 2
    assert L.fs_frame_metrics2d(1, 1, 0, 1, 16, 16, 1.0, 1, 1, 1, None) == 2                      # N < 1
    assert L.fs_frame_metrics3d(1, 1, 1, 1, 10, 16, 16, 1.0, 1, 1, 1, None) == 2                  # D < 11
    assert L.fs_frame_metrics2d(1, 1, 1 << 30, 64, 32, 32, 1.0, 1, 1, 1, None) == 2              # grid overflow
    assert L.fs_frame_metrics3d(1, 1, 1 << 20, 1, 2048, 2048, 2048, 1.0, 1, 1, 1, None) == 2
    assert L.fs_frame_metrics2d(1, 1, 1, 1, 16, 16, 0.0, 1, 1, 1, None) == 3                      # ARG: L <= 0
    assert L.fs_frame_metrics3d(1, 1, 1, 1, 16, 16, 16, -1.0, 1, 1, 1, None) == 3
    assert L.fs_frame_metrics2d(1, 1, 1, 1, 16, 16, float("nan"), 1, 1, 1, None) == 3
    # workspace: one fp64 pair per workgroup (16 x 16 output tiles; 3-D: z chunks of >= 16 output slices)
    assert L.fs_frame_metrics2d_ws_bytes(64, 1, 160, 224) == 64 * 10 * 14 * 16
    assert L.fs_frame_metrics2d_ws_bytes(1, 1, 11, 11) == 16
    assert L.fs_frame_metrics3d_ws_bytes(2, 1, 256, 256, 256) == 2 * 256 * 4 * 16
    assert L.fs_frame_metrics3d_ws_bytes(1, 1, 10, 16, 16) == -2


def test_metrics_kernels_do_not_spill():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("needs hipcc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-c", os.path.join(CSRC, "metrics.hip"), "-o", os.devnull, "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "loop not unrolled" not in r.stderr  # the 3-D register ring needs its z loop fully unrolled
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    kernels = {k: v for k, v in usage.items() if "frame_metrics" in k}
    assert len(kernels) == 3, sorted(usage)
    for name, u in kernels.items():
        # (SGPR spills land in VGPR lanes, not in scratch)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (name, u)
