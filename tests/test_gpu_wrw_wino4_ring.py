"""Round 12: the trunk's F(4,3) weight gradient with the source operand transformed and split ONCE per row by the loader
waves into a ring of piece rows (csrc/convwrwwino4.hpp, csrc/convwrwwino4_sched.hpp).  tests/tools/wrw_wino4_ring_check.py
runs the kernel at 64 -> 64 channels on four shapes of exactly 1024 bricks chosen for the ring -- (d) a plane change every
second brick, (e) every row both first and last of its plane, (f) many sample boundaries and padding planes, (g) two
x-bricks per row -- each with random operands and with a gradient that is zero away from the planes' first / last rows and
the volume's first / last planes, in the atomic and the deterministic form against an fp64 reference evaluated tap by tap;
once on the product library and once on the ablation build's fp32-MFMA form (FLOWSCI_WRW_WINO4_NO_S3=1), each in a fresh
process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "tools", "wrw_wino4_ring_check.py")
FS_WRW_KERNEL_WINO43 = 3
BAND = 2e-5  # of max |ref|: the ledger's band (tests/test_gpu_conv_ledger.py)
CASES = [(n, k, d) for n in "defg" for k in ("edge", "rand") for d in "01"]


def _run(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FLOWSCI_")}
    r = subprocess.run([sys.executable, TOOL], env=dict(env, **extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]  # (nothing is launched after a failure)
    cases = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] == "CASE":
            kv = dict(x.split("=", 1) for x in f[3:])
            cases[(f[1], f[2], kv["det"])] = (int(kv["kid"]), float(kv["err"]), kv["rep"] == "1")
    print(r.stdout)
    return cases


@pytest.fixture(scope="module")
def runs(ablation_lib):
    return _run({}), _run({"FLOWSCI_HIP_LIBRARY": ablation_lib, "FLOWSCI_WRW_WINO4_NO_S3": "1"})


def test_every_ring_shape_stays_in_the_ledger_band(runs):
    ring, fp = runs
    assert sorted(ring) == CASES and sorted(fp) == CASES, (sorted(ring), sorted(fp))
    for key, (kid, err, rep) in ring.items():
        assert kid == FS_WRW_KERNEL_WINO43 and fp[key][0] == FS_WRW_KERNEL_WINO43, (key, kid, fp[key])
        assert err < BAND, (key, err)
        assert rep, key  # deterministic form: bitwise equal on a second call


def test_error_against_fp64_is_that_of_the_fp32_kernel(runs):
    """deterministic form, per shape and data within 1.25x the fp32-MFMA kernel's error (the bound of
    tests/test_gpu_wrw_wino4_s3.py); a stale or shifted ring row on the edge data would be an O(1) error"""
    ring, fp = runs
    ratios = {k: (ring[k][1] / fp[k][1], ring[k][1], fp[k][1]) for k in CASES if k[2] == "1"}
    print("ring / fp32 error ratios:", ratios)
    for k, (r, _, _) in ratios.items():
        assert r <= 1.25, (k, ratios[k])
