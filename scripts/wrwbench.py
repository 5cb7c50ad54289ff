"""Micro-benchmark of fs_conv3d_wrw on the IFNet-3D layer shapes at 256^3 (GPU box only).  Arguments: substrings of the
row names to run (default: every row).  Each row names the kernel the library dispatches to and the arithmetic it runs:
the product library's F(4,3) and k4 kernels multiply split-bf16 operands; the ablation build (FLOWSCI_HIP_LIBRARY) runs
their fp32-MFMA forms under FLOWSCI_WRW_WINO4_NO_S3=1 / FLOWSCI_WRW_NO_S3=1, and round 11's F(4,3) kernel (both operands
split on the matrix waves) under FLOWSCI_WRW_WINO4_MW=1.  The row "convblock W=128" is the trunk layer at 64 x 64 x 128:
two x-bricks per row."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from opticalflowscivis_amd import ops


def t(fn, n=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


KERNELS = {0: "brick", 1: "dma", 2: "wino F(2,3)", 3: "wino F(4,3)", 4: "k4 s3"}  # FS_WRW_KERNEL_*
AB_LIB = bool(os.environ.get("FLOWSCI_HIP_LIBRARY"))  # (the product library reads no switch)


def arithmetic(kid):
    """INFERRED from the kernel id and the switches this process was started with -- the library is not asked, so a
    misspelt switch prints the wrong label (the ablation library latches its switches at first use)."""
    if kid == 3:
        if AB_LIB and os.environ.get("FLOWSCI_WRW_WINO4_NO_S3"):
            return "fp32 MFMA"
        return "split-bf16 x6, source split on the " + ("matrix waves" if AB_LIB and os.environ.get("FLOWSCI_WRW_WINO4_MW") else "loader waves")
    if kid == 4:
        return "split-bf16 x6"
    return "fp32 MFMA"


def case(name, cg, cs, k, s, out, B=2):
    """out: the output extent, one number for a cube"""
    if len(sys.argv) > 1 and not any(a in name for a in sys.argv[1:]):
        return
    outs = (out,) * 3 if isinstance(out, int) else tuple(out)
    inns = tuple((o - 1) * s + k - 2 for o in outs)
    g = torch.randn((B, cg) + outs, device="cuda")
    src = torch.randn((B, cs) + inns, device="cuda")
    ms = t(lambda: ops.conv3d_wrw(g, src, k, s, 1))
    fl = 2.0 * cg * cs * k ** 3 * B * outs[0] * outs[1] * outs[2]
    kid = ops.conv3d_wrw_kernel_id(g.data_ptr(), src.data_ptr(), B, cg, cs, outs, inns, k, s, 1)
    print("%-28s Cg=%3d Cs=%3d k%d s%d out=%s: %.3f ms  %.1f TFLOP/s  [%s, %s]"
          % (name, cg, cs, k, s, "%3d^3" % out if isinstance(out, int) else "x".join(map(str, outs)), ms, fl / ms / 1e9,
             KERNELS.get(kid, kid), arithmetic(kid)), flush=True)


case("conv0a (11->32)", 32, 11, 4, 2, 128)
case("conv0b (32->64)", 64, 32, 4, 2, 64)
case("convblock (64->64)", 64, 64, 3, 1, 64)
case("convblock W=128 (64->64)", 64, 64, 3, 1, (64, 64, 128))
case("deconv1 (64->32)", 64, 32, 4, 2, 64)
case("deconv2 flow (32->6)", 32, 6, 4, 2, 128)
case("deconv2 mask (32->1)", 32, 1, 4, 2, 128)
case("block0 conv (128->128) @16^3", 128, 128, 3, 1, 16)
