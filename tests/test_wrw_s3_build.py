"""CPU (no GPU needed): compile-time guards of the split-bf16 weight-gradient kernel (csrc/convwrw_s3.hpp).  Its loader
waves are those of the fp32 loader-wave kernel (LDS-DMA only, no register in flight under an inline-assembly load); the
matrix waves hold 128 accumulator registers beside the operand pieces of two units, so spills are the thing to guard."""
import os
import sys

from test_build_resources import _check, _device_asm, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wrw_s3_kernel_has_no_scratch_and_no_spills():
    usage = _resource_usage("convwrw.hip")
    hits = {k: v for k, v in usage.items() if "conv3d_wrw_s3_kernel" in k}
    assert len(hits) == 3, sorted(hits)  # <6,1,...> (<= 32 gradient channels), <8,2,...> for Wo >= 32 and Wo == 16
    _check(hits, "conv3d_wrw_s3_kernel", 256)


def test_wrw_s3_loaders_keep_no_register_in_flight(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_inflight_regs as chk
    asm = _device_asm("convwrw.hip", tmp_path)
    assert chk.check(asm, "conv3d_wrw_s3_kernel") == 0
