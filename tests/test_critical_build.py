"""CPU: critical.hip compiled for gfx950 -- neither pass, in 2-D or 3-D, uses scratch or spills a register (the corners of
a cell live in registers and a simplex picks its own through a switch over constants, not through a runtime index)."""
from test_build_resources import _resource_usage


def test_critical_kernels_use_no_scratch_and_spill_nothing():
    usage = _resource_usage("critical.hip")
    count = [k for k in usage if "critical_count_kernel" in k]
    emit = [k for k in usage if "critical_emit_kernel" in k]
    assert len(count) == 2 and len(emit) == 2, sorted(usage)  # 2-D and 3-D each
    for name, u in usage.items():  # (common.hpp's reduction kernel is emitted with every file)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    for name in count + emit:
        assert usage[name]["LDS Size [bytes/block]"] == 0, (name, usage[name])
    print({k: v["VGPRs"] for k, v in usage.items()})
