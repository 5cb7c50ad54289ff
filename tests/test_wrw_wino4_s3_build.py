"""CPU (no GPU needed): compile-time guards of the trunk's F(4,3) weight-gradient kernel on split-bf16 matrix cores
(csrc/convwrwwino4.hpp).  Its matrix waves hold 144 accumulator registers beside five sets of operand pieces (60) and two
raw operand pairs, at two waves per SIMD (256 registers): a spill is the thing to guard; its two fp32 staging buffers take
140 of the 160 KB of LDS.  In the ablation build the fp32-MFMA form is compiled beside it under its own name."""
from test_build_resources import _check, _resource_usage


def test_wrw_wino4_kernel_has_no_scratch_and_no_spills():
    usage = _resource_usage("convwrw.hip")
    hits = {k: v for k, v in usage.items() if "conv3d_wrw_wino4_kernel" in k}
    assert len(hits) == 1, sorted(hits)  # the product library holds the one instantiation <0>
    assert not [k for k in usage if "conv3d_wrw_wino4_f32_kernel" in k], sorted(usage)
    _check(hits, "conv3d_wrw_wino4_kernel", 256)  # (_check: no scratch, no VGPR spills, at most 160 KB of LDS)
    (u,) = hits.values()
    assert u["LDS Size [bytes/block]"] <= 160 * 1024, u


def test_wrw_wino4_ablation_build_keeps_the_fp32_form():
    usage = _resource_usage("convwrw.hip", ["-DFS_ABLATION"])
    _check(usage, "conv3d_wrw_wino4_kernel", 256)      # <0>, <1> / <2> of FLOWSCI_WINO_DBG, <5> / <6> / <7> of FLOWSCI_WRW_WINO4_S3_AB
    _check(usage, "conv3d_wrw_wino4_f32_kernel", 256)  # FLOWSCI_WRW_WINO4_NO_S3=1
