"""The trunk's F(4,3) weight gradient (csrc/convwrwwino4.hpp, 64 -> 64 channels, k3 s1 p1) on the smallest shapes at
which its ring of source-piece rows (csrc/convwrwwino4_sched.hpp) can go wrong, against the fp64 reference of
tests/tools/wrw_wino4_s3_check.py evaluated tap by tap, whole tensors (GPU box only).  Each shape has exactly the 1024
bricks of the dispatch threshold; each runs with random operands ("rand") and with G zeroed except the first and last row
of every plane and the first and last plane ("edge"): the ring's padding rows and plane changes then carry the whole
result.  Run once per library (product; ablation build with FLOWSCI_WRW_WINO4_NO_S3=1 or FLOWSCI_WRW_WINO4_MW=1);
tests/test_gpu_wrw_wino4_ring.py compares.  Prints

    CASE <shape> <data> det=<0/1> kid=<FS_WRW_KERNEL_*> err=<max |dW - ref| / max |ref|> rep=<two deterministic runs equal> hash=<of the deterministic dW>
    DONE

Arguments: shape names (default: all)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from wrw_wino4_s3_check import DEV, err, ops, reference, wrw

# d: a plane change every second brick; e: every gradient row is first and last of its plane (rows y - 1 and y + 1 are
# always padding); f: many sample boundaries, a padding plane (kz = 0 / 2) every fourth plane; g: two x-bricks per row,
# plane changes inside runs
SHAPES = {"d": (1, (512, 4, 64)), "e": (1, (1024, 2, 64)), "f": (8, (4, 64, 64)), "g": (1, (64, 16, 128))}


def data(name, kind):
    B, size = SHAPES[name]
    gen = torch.Generator().manual_seed(1200 + ord(name))
    G = torch.randn((B, 64) + size, generator=gen)
    x = torch.randn((B, 64) + size, generator=gen)
    if kind == "edge":
        keep = torch.zeros(size, dtype=torch.bool)
        keep[0] = keep[-1] = True
        keep[:, 0] = keep[:, -1] = True
        G = G * keep
    return G, x


def main():
    for name in (sys.argv[1:] or list(SHAPES)):
        B, size = SHAPES[name]
        for kind in ("rand", "edge"):
            G, x = data(name, kind)
            ref = reference(G, x)
            Gd, xd = G.to(DEV), x.to(DEV)
            kid = ops.conv3d_wrw_kernel_id(Gd.data_ptr(), xd.data_ptr(), B, 64, 64, size, size, 3, 1, 1)
            print("CASE %s %s det=0 kid=%d err=%.3e rep=1 hash=-" % (name, kind, kid, err(wrw(Gd, xd, 0), ref)), flush=True)
            d1, d2 = wrw(Gd, xd, 1), wrw(Gd, xd, 1)
            h = hashlib.sha1(d1.cpu().numpy().tobytes()).hexdigest()[:16]
            print("CASE %s %s det=1 kid=%d err=%.3e rep=%d hash=%s"
                  % (name, kind, kid, err(d1, ref), int(torch.equal(d1, d2)), h), flush=True)
    print("DONE")


if __name__ == "__main__":
    main()
