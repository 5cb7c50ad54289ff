"""Round 11: the trunk's F(4,3) weight gradient on split-bf16 matrix cores (csrc/convwrwwino4.hpp).
tests/tools/wrw_wino4_s3_check.py runs the kernel at 64 -> 64 channels on three shapes -- (a) exactly the 1024 bricks of
the dispatch threshold, (b) odd depth with a run of bricks crossing the batch boundary, (c) two x-bricks per row -- in the
atomic and the deterministic form against an fp64 reference evaluated tap by tap, with G scaled by 2^-40 and with one
+inf in G; once on the product library and once on the ablation build with FLOWSCI_WRW_WINO4_NO_S3=1 (the fp32-MFMA form
of the same kernel, the parent's arithmetic), each in a fresh process.  A third fresh process makes the kernel its first
launch."""
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "tools", "wrw_wino4_s3_check.py")
FS_WRW_KERNEL_WINO43 = 3
BAND = 2e-5  # of max |ref|: the ledger's band (tests/test_gpu_conv_ledger.py)


def _env(extra):
    env0 = {k: v for k, v in os.environ.items() if not k.startswith("FLOWSCI_")}
    return dict(env0, **extra)


def _run(extra):
    r = subprocess.run([sys.executable, TOOL], env=_env(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    cases, scale, nonfinite = {}, {}, None
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] == "CASE":
            kv = dict(x.split("=", 1) for x in f[2:])
            cases[(f[1], kv["det"])] = (int(kv["kid"]), float(kv["err"]), kv["rep"] == "1")
        elif f and f[0] == "SCALE":
            scale[f[1]] = f[2] == "ok=1"
        elif f and f[0] == "NONFINITE":
            nonfinite = (f[1] == "ok=1", float(f[2].split("=", 1)[1]))
    print(r.stdout)
    return cases, scale, nonfinite


@pytest.fixture(scope="module")
def runs(ablation_lib):
    return _run({}), _run({"FLOWSCI_HIP_LIBRARY": ablation_lib, "FLOWSCI_WRW_WINO4_NO_S3": "1"})


def test_both_forms_stay_in_the_ledger_band(runs):
    (s3, _, _), (fp, _, _) = runs
    assert sorted(s3) == [(n, d) for n in "abc" for d in "01"] and s3.keys() == fp.keys(), (sorted(s3), sorted(fp))
    for key, (kid, err, rep) in s3.items():
        assert kid == FS_WRW_KERNEL_WINO43 and fp[key][0] == FS_WRW_KERNEL_WINO43, (key, kid, fp[key])
        assert err < BAND, (key, err)
        assert rep, key  # deterministic form: bitwise equal on a second call
    for key, (kid, err, rep) in fp.items():
        assert err < BAND and rep, (key, err, rep)


def test_error_against_fp64_is_that_of_the_fp32_kernel(runs):
    """deterministic form (the atomic form's error moves about +-30 % with the order of the atomics): per shape within
    1.25x the fp32-MFMA kernel's error on the same data, the geometric mean of the ratios within 1.05"""
    (s3, _, _), (fp, _, _) = runs
    ratios = {n: s3[(n, "1")][1] / fp[(n, "1")][1] for n in "abc"}
    print("s3 / fp32 error ratios:", ratios, {n: (s3[(n, "1")][1], fp[(n, "1")][1]) for n in "abc"})
    for n, r in ratios.items():
        assert r <= 1.25, (n, r, s3[(n, "1")], fp[(n, "1")])
    assert math.exp(sum(math.log(r) for r in ratios.values()) / len(ratios)) <= 1.05, ratios


def test_power_of_two_scaling_is_exact(runs):
    """transforms and splitting commute with a power-of-two scale away from underflow: a piece lost to range shows here"""
    (_, scale, _), _ = runs
    assert scale == {"a": True, "b": True, "c": True}, scale


def test_one_inf_makes_its_row_non_finite_and_no_other(runs):
    """+-inf splits into (inf, NaN, NaN): an entry the fp32 kernel gives as +-inf may come out NaN"""
    (_, _, nf), (_, _, nf_fp) = runs
    assert nf is not None and nf[0] and nf[1] < BAND, nf
    assert nf_fp is not None and nf_fp[0] and nf_fp[1] < BAND, nf_fp


def test_cold_first_launch():
    r = subprocess.run([sys.executable, TOOL, "--cold"], env=_env({}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]  # (nothing is launched after a failure)
    line = [l for l in r.stdout.splitlines() if l.startswith("COLD")]
    assert len(line) == 1, r.stdout[-3000:]
    assert float(line[0].split("=", 1)[1]) < BAND, line
