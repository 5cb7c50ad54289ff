"""CPU: ridges.hip compiled for gfx950 -- none of its three kernels (the node pass, which carries a 3 x 3 matrix and its
accumulated rotations in fp64, the count pass and the emit pass) uses scratch, spills a register or touches LDS: the
matrices are scalars rotated by name, the eigenvector's column is taken by selects, and a cell's corners are indexed by
constants."""
from test_build_resources import _resource_usage


def test_ridge_kernels_use_no_scratch_and_spill_nothing():
    usage = _resource_usage("ridges.hip")
    for needle in ("ridge_node_kernel", "ridge_count_kernel", "ridge_emit_kernel"):
        assert len([k for k in usage if needle in k]) == 1, (needle, sorted(usage))
    for name, u in usage.items():  # (common.hpp's reduction kernel is emitted with every file)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        if "ridge_" in name:
            assert u["LDS Size [bytes/block]"] == 0, (name, u)
    print({k: v["VGPRs"] for k, v in usage.items()})
