"""The two head launches of the 256^3 step alone (scripts/trbench.py's shapes and timer, without its MIOpen legs): one line
with the error against fp64 (first sample) and min / median / max ms per launch of five timings of 20 launches, for the
flow head (2 x 32 -> 6 at 128^3) and the mask head (32 -> 1).  FLOWSCI_HIP_LIBRARY selects another build for A/B runs.
GPU box only."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from opticalflowscivis_amd import ops, _lib

def t(fn, n=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n

res = []
for cout in (6, 1):
    torch.manual_seed(0)
    x = torch.randn(2, 32, 128, 128, 128, device="cuda")
    w = torch.randn(32, cout, 4, 4, 4, device="cuda") / (32 * 8) ** 0.5
    bias = torch.randn(cout, device="cuda")
    got = ops.conv3d_tr(x, w, bias)
    ref = F.conv_transpose3d(x.double()[:1], w.double(), bias.double(), 2, 1)
    err = float((got[:1].double() - ref).abs().max() / ref.abs().max())
    for _ in range(3):
        t(lambda: ops.conv3d_tr(x, w, bias), 5)
    ts = [t(lambda: ops.conv3d_tr(x, w, bias)) for _ in range(5)]
    res.append("32->%d: err %.2e ms min %.4f med %.4f max %.4f" % (cout, err, min(ts), sorted(ts)[2], max(ts)))
print("HEAD %s | %s" % (os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH), " | ".join(res)), flush=True)
