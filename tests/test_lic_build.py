"""CPU: lic.hip compiled for gfx950 -- no kernel in the file, the packing pre-pass included, uses scratch or spills a
register (the corner loops are unrolled over constants, the two sides of a line share one loop body and their results are
folded into scalars)."""
from test_build_resources import _resource_usage


def test_lic_kernels_use_no_scratch_and_spill_nothing():
    usage = _resource_usage("lic.hip")
    kernels = {k: v for k, v in usage.items() if "lic_kernel" in k}
    assert len(kernels) == 4, sorted(usage)  # 2-D and 3-D, Euler and RK2
    assert len([k for k in usage if "lic_pack_kernel" in k]) == 2, sorted(usage)
    for name, u in usage.items():  # (common.hpp's reduction kernel is emitted with every file)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    for name, u in kernels.items():
        assert u["LDS Size [bytes/block]"] == 0, (name, u)
    print({k: v["VGPRs"] for k, v in usage.items()})
