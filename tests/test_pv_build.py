"""CPU: pvlines.hip compiled for gfx950 -- none of its three kernels (the face and tetrahedron kernels of the count pass,
the emit kernel) uses scratch, spills a register or touches LDS: the screening picks corners by constants, load_face by
address arithmetic, and the cubic's knots are chosen by selects."""
from test_build_resources import _resource_usage


def test_pv_kernels_use_no_scratch_and_spill_nothing():
    usage = _resource_usage("pvlines.hip")
    for needle in ("pv_face_kernel", "pv_tet_kernel", "pv_emit_kernel"):
        assert len([k for k in usage if needle in k]) == 1, (needle, sorted(usage))
    for name, u in usage.items():  # (common.hpp's reduction kernel is emitted with every file)
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        if "pv_" in name:
            assert u["LDS Size [bytes/block]"] == 0, (name, u)
    print({k: v["VGPRs"] for k, v in usage.items()})
