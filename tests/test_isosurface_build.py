"""CPU: isosurface.hip compiled for gfx950 -- neither kernel uses scratch or spills a register (the corner arrays of the
emit kernel are indexed by constants only and stay in registers), and neither holds LDS that would keep a second
workgroup off a CU (80 KB each out of 160 KB)."""
from test_build_resources import _resource_usage

KERNELS = ("iso_count_kernel", "iso_emit_kernel")


def test_isosurface_kernels_use_no_scratch_and_little_lds():
    usage = _resource_usage("isosurface.hip")
    for needle in KERNELS:
        hits = {k: v for k, v in usage.items() if needle in k}
        assert len(hits) == 1, "expected one kernel matching %r in %s" % (needle, sorted(usage))
        for name, u in hits.items():
            assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
            assert u["LDS Size [bytes/block]"] <= 80 * 1024, (name, u)
    # the streaming count pass keeps full occupancy
    count = [u for k, u in usage.items() if "iso_count_kernel" in k][0]
    assert count["VGPRs"] <= 64, count
