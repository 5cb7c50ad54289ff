"""CPU (no GPU needed): the step schedule of the trunk's F(4,3) weight-gradient kernel (csrc/convwrwwino4_sched.hpp) and
the kernel's compile-time guards after round 12.

The schedule -- which ring slot a step reads for ky = 0, 1, 2, what the loader waves stage and transform during it, how
many barriers a run has -- is plain constexpr C++ shared by the kernel and tests/tools/wrw_wino4_sched_check.cpp, a
stand-alone host program that plays both roles over every run of the GPU tests' seven shapes and the bench shape (also
with one-brick runs), all three kz.  It is built with the host compiler and -fsanitize=address,undefined and run
directly."""
import os
import shutil
import subprocess

import pytest
from test_build_resources import _check, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticalflowscivis_amd", "csrc")


def test_schedule_model_every_run_reads_the_rows_it_needs(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("needs a host C++ compiler")
    exe = str(tmp_path / "wrw_wino4_sched_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "tools", "wrw_wino4_sched_check.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-3000:] + r.stderr[-3000:]
    assert len([l for l in r.stdout.splitlines() if " spw=" in l]) == 16, r.stdout  # eight geometries, natural and one-brick runs


def test_wrw_wino4_product_kernel_resources():
    usage = _resource_usage("convwrw.hip")
    hits = {k: v for k, v in usage.items() if "conv3d_wrw_wino4_kernel" in k}
    assert len(hits) == 1, sorted(hits)  # the one instantiation <0>
    assert not [k for k in usage if "conv3d_wrw_wino4_mw_kernel" in k], sorted(usage)
    _check(hits, "conv3d_wrw_wino4_kernel", 256)  # no scratch, no VGPR spills
    (u,) = hits.values()
    assert u["LDS Size [bytes/block]"] <= 160 * 1024, u


def test_wrw_wino4_ablation_build_keeps_round_11s_form():
    usage = _resource_usage("convwrw.hip", ["-DFS_ABLATION"])
    _check(usage, "conv3d_wrw_wino4_mw_kernel", 256)  # FLOWSCI_WRW_WINO4_MW=1: both operands split on the matrix waves
    _check(usage, "conv3d_wrw_wino4_kernel", 256)     # <0> and the measurement forms <1>, <2>, <3>, <5>, <6>, <7>
    assert len([k for k in usage if "conv3d_wrw_wino4_kernel" in k]) == 7, sorted(usage)
