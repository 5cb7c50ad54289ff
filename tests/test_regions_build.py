"""CPU: regions.hip compiled for gfx950 -- no kernel of it uses scratch or spills a register, and a workgroup's LDS
leaves room for at least two workgroups per CU (80 KB each out of 160 KB)."""
from test_build_resources import _resource_usage

KERNELS = ("label_tile_kernel", "label_border_kernel", "label_flatten_kernel", "stats_init_kernel", "stats_kernel",
           "stats_final_kernel", "follow_kernel")


def test_region_kernels_use_no_scratch_and_little_lds():
    usage = _resource_usage("regions.hip")
    for needle in KERNELS:
        hits = {k: v for k, v in usage.items() if needle in k}
        assert hits, "no kernel matching %r in %s" % (needle, sorted(usage))
        for name, u in hits.items():
            assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
            assert u["LDS Size [bytes/block]"] <= 80 * 1024, (name, u)
    # both dimensionalities of the templated kernels are there
    for needle in ("label_tile_kernel", "label_border_kernel", "stats_kernel", "follow_kernel"):
        assert sum(needle in k for k in usage) == 2, needle
