"""Weight gradients of the k4 s2 layer shapes against an fp64 reference, whole tensors (GPU box only).  Run once with the
product library (split-bf16 kernel, csrc/convwrw_s3.hpp) and once with the ablation build and FLOWSCI_WRW_NO_S3=1 (the
fp32-MFMA kernel of the same bricks); tests/test_gpu_wrw_s3.py compares the two.  Prints one line per case:

    CASE <name> det=<0/1> kid=<FS_WRW_KERNEL_*> err=<max |dW - ref| / max |ref|> rep=<two deterministic runs equal>
    COLD err=<...>            (fresh buffers, caches evicted, one launch)
    NONFINITE <layer> ok=<0/1>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from opticalflowscivis_amd import ops

DEV = torch.device("cuda:0")

# (name, B, Cg, Cs, output grid (D, H, W), multi-source planes or None): every dispatch form of the k4 s2 loader-wave kernels
CASES = [
    ("conv0b 32->64", 2, 64, 32, (8, 12, 32), None),
    ("deconv1 64->32 (G = layer input)", 2, 64, 32, (6, 8, 64), None),
    ("block0 conv0b Wo=16", 2, 64, 32, (6, 8, 16), None),
    ("conv0a 11->32", 2, 32, 11, (10, 8, 32), None),
    ("conv0a 12->32 multi-source", 2, 32, 12, (6, 10, 32), (3, 3, 3, 3)),
    ("conv0a 11->32 multi-source", 2, 32, 11, (6, 6, 32), (1, 1, 3, 3, 3)),
    ("flow head deconv2 32->6", 2, 32, 6, (8, 6, 32), None),
    ("ragged: Cg 48, Cs 20, bricks past the grid", 1, 48, 20, (5, 7, 40), None),
    ("ragged: Cg 24, Cs 7, bricks past the grid", 3, 24, 7, (3, 5, 36), None),
]


def reference(G, S):
    k, s, p = 4, 2, 1
    return torch.nn.grad.conv3d_weight(S.double(), (G.shape[1], S.shape[1], k, k, k), G.double(), stride=s, padding=p)


def run(name, B, Cg, Cs, out, planes, det):
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 17 * det)
    D, H, W = out
    G = torch.randn(B, Cg, D, H, W, generator=gen)
    S = torch.randn(B, Cs, 2 * D, 2 * H, 2 * W, generator=gen)
    ref = reference(G, S)
    Gd = G.to(DEV)
    kid = ops.conv3d_wrw_kernel_id(Gd.data_ptr(), 0x1000, B, Cg, Cs, (D, H, W), (2 * D, 2 * H, 2 * W), 4, 2, 1)
    torch.use_deterministic_algorithms(bool(det))
    try:
        if planes is None:
            dw = ops.conv3d_wrw(Gd, S.to(DEV), 4, 2, 1)
        else:
            pieces, c = [], 0
            for n in planes:
                pieces.append(S[:, c:c + n].contiguous().to(DEV))
                c += n
            dw = ops.conv3d_wrw_ms(Gd, pieces, 4, 2, 1)
            assert dw is not None, name
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(False)
    err = float((dw.cpu().double() - ref).abs().max() / ref.abs().max())
    return kid, err, dw


def cold(name, B, Cg, Cs, out):
    """fresh buffers, caches evicted (a 1 GiB write), one launch"""
    gen = torch.Generator().manual_seed(99)
    D, H, W = out
    G = torch.randn(B, Cg, D, H, W, generator=gen)
    S = torch.randn(B, Cs, 2 * D, 2 * H, 2 * W, generator=gen)
    ref = reference(G, S)
    Gd, Sd = G.to(DEV), S.to(DEV)
    junk = torch.empty(256 * 1024 * 1024, device=DEV)
    junk.fill_(1.0)
    del junk
    torch.cuda.synchronize()
    dw = ops.conv3d_wrw(Gd, Sd, 4, 2, 1)
    torch.cuda.synchronize()
    return float((dw.cpu().double() - ref).abs().max() / ref.abs().max())


def nonfinite(B, Cg, Cs, out):
    """an inf in the source and a NaN in G: every dW entry an fp64 reference makes non-finite must come out non-finite"""
    gen = torch.Generator().manual_seed(5)
    D, H, W = out
    G = torch.randn(B, Cg, D, H, W, generator=gen)
    S = torch.randn(B, Cs, 2 * D, 2 * H, 2 * W, generator=gen)
    S[1, 2, 5, 7, 9] = float("inf")
    S[0, 1, 3, 4, 20] = -float("inf")
    G[0, 3, 2, 2, 5] = float("nan")
    ref = reference(G, S)
    dw = ops.conv3d_wrw(G.to(DEV), S.to(DEV), 4, 2, 1).cpu()
    bad = ~torch.isfinite(ref)
    return int(bad.sum()) > 0 and bool((~torch.isfinite(dw[bad])).all()) and bool(torch.isfinite(dw[~bad]).all())


if __name__ == "__main__":
    for name, B, Cg, Cs, out, planes in CASES:
        for det in (0, 1):
            kid, err, dw = run(name, B, Cg, Cs, out, planes, det)
            if det:  # bitwise reproducible: a second deterministic run
                _, _, dw2 = run(name, B, Cg, Cs, out, planes, det)
                rep = bool(torch.equal(dw, dw2))
            else:
                rep = True
            print("CASE %s det=%d kid=%d err=%.3e rep=%d" % (name.replace(" ", "_"), det, kid, err, int(rep)), flush=True)
    print("COLD err=%.3e" % cold("cold", 2, 64, 32, (16, 16, 32)), flush=True)
    for name, Cg, Cs in (("conv0b", 64, 32), ("conv0a", 32, 11), ("head", 32, 6)):
        print("NONFINITE %s ok=%d" % (name, int(nonfinite(2, Cg, Cs, (6, 8, 32)))), flush=True)
    print("DONE")
