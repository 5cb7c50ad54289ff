"""CPU: streamline.hip compiled for gfx950 -- the streamline kernel, in 2-D and 3-D and for each of its three methods,
uses no scratch, spills no register and declares no LDS (a line's position, its stage directions and the corners of a
sample live in registers: every array of the kernel is indexed by unrolled constants)."""
from test_build_resources import _resource_usage


def test_streamline_kernels_use_no_scratch_no_lds_and_spill_nothing():
    usage = _resource_usage("streamline.hip")
    lines = [k for k in usage if "streamline_kernel" in k]
    assert len(lines) == 6, sorted(usage)  # 2-D and 3-D, each Euler, RK2 and RK4
    assert sum("ILi2E" in k for k in lines) == 3 and sum("ILi3E" in k for k in lines) == 3, lines
    for name, u in usage.items():  # (common.hpp's reduction kernel is emitted with every file)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    for name in lines:
        assert usage[name]["LDS Size [bytes/block]"] == 0, (name, usage[name])
    print({k: v["VGPRs"] for k, v in usage.items()})
