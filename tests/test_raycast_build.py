"""CPU: raycast.hip compiled for gfx950 -- no kernel of it uses scratch or spills a register, and a workgroup's LDS (the
transfer function and the camera) leaves room for at least two workgroups per CU (80 KB each out of 160 KB)."""
from test_build_resources import _resource_usage

KERNELS = ("raycast_kernel", "brick_range_kernel", "brick_skip_kernel")


def test_raycast_kernels_use_no_scratch_and_little_lds():
    usage = _resource_usage("raycast.hip")
    for needle in KERNELS:
        hits = {k: v for k, v in usage.items() if needle in k}
        assert hits, "no kernel matching %r in %s" % (needle, sorted(usage))
        for name, u in hits.items():
            assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
            assert u["LDS Size [bytes/block]"] <= 80 * 1024, (name, u)
    # both modes of the ray kernel, each with and without the brick map
    assert sum("raycast_kernel" in k for k in usage) == 4
    # one pixel per lane in registers: every ray kernel leaves room for at least four waves per SIMD
    for name, u in usage.items():
        if "raycast_kernel" in name:
            assert u["VGPRs"] <= 128, (name, u)
