"""Ledger of convolution dispatch cases: one row per call of fs_conv3d_fwd* / fs_conv3d_tr* / fs_conv3d_wrw*, with the
compute kernel the library's dispatch ladder (csrc/convfwd.hip conv3d_fwd_impl, csrc/convtr.hip conv3d_tr_slice,
csrc/convwrw.hip conv3d_wrw_impl) must pick for it.  Plain data, read by tests/test_conv_ledger.py (every compiled kernel
has a row, every row agrees with the library's own plan) and tests/test_gpu_conv_ledger.py (the named kernel runs, and
nothing else, and its output matches an fp64 reference inside guard bands).

Row fields:
  op      fwd | fwd_add | fwd_prelu | fwd_dprelu | fwd_ms | tr | tr_add | tr_prelu | wrw | wrw_det | wrw_ms
  B, cin, cout    fwd / tr: input and output channels.  wrw: cin = Cs (source channels), cout = Cg (gradient channels)
  inp, out        fwd / tr: input and output extents (D, H, W).  wrw: inp = the source's, out = the gradient's
  k, stride, pad, wmode
  mis     16-byte misalignment of x (wrw: of g), in floats
  mis2    wrw only: misalignment of src
  kernel  the compute kernel symbol, written as ops._KERNELS writes symbols
  why     the rung of the ladder the row is on

Shapes are as small as their rung allows; the rows on the two sides of a threshold differ in one quantity only."""
from ledger_harness import normalize  # noqa: F401  (a ledger carries the naming of its kernels)

FORMS = ("fwd", "fwd_add", "fwd_prelu", "fwd_dprelu", "fwd_ms", "tr", "tr_add", "tr_prelu", "wrw", "wrw_det", "wrw_ms")

ROWS = []


def _out_fwd(inp, k, s, p):
    return tuple((n + 2 * p - k) // s + 1 for n in inp)


def _fwd(ops, B, cin, cout, inp, k, kernel, why, pad=1, wmode=0, mis=0):
    s = 1 if k == 3 else 2
    for op in ops:
        ROWS.append(dict(op=op, B=B, cin=cin, cout=cout, inp=tuple(inp), out=_out_fwd(inp, k, s, pad), k=k, stride=s,
                         pad=pad, wmode=1 if (op == "fwd_dprelu" and k == 3) else wmode, mis=mis, mis2=0,
                         kernel=kernel, why=why))


def _tr(ops, B, cin, cout, inp, kernel, why, odd=(0, 0, 0), mis=0):
    out = tuple(2 * n + o for n, o in zip(inp, odd))
    for op in ops:
        ROWS.append(dict(op=op, B=B, cin=cin, cout=cout, inp=tuple(inp), out=out, k=4, stride=2, pad=1, wmode=0, mis=mis,
                         mis2=0, kernel=kernel, why=why))


def _wrw(ops, B, cs, cg, out, k, kernel, why, pad=1, mis=0, mis2=0, inp=None):
    s = 1 if k == 3 else 2
    if inp is None:  # the source of the convolution whose gradient grid is `out`
        inp = tuple(n if k == 3 else 2 * n for n in out)
    for op in ops:
        ROWS.append(dict(op=op, B=B, cin=cs, cout=cg, inp=tuple(inp), out=tuple(out), k=k, stride=s, pad=pad, wmode=0,
                         mis=mis, mis2=mis2, kernel=kernel, why=why))


ALL_FWD = ("fwd", "fwd_add", "fwd_prelu")
DP_FWD = ALL_FWD + ("fwd_dprelu",)
ALL_TR = ("tr", "tr_add", "tr_prelu")
BOTH_WRW = ("wrw", "wrw_det")

# ---- forward, k = 3 s 1 -------------------------------------------------------------------------------------------
# the 2-D Winograd trunk kernel: 64-channel output groups, Cin % 4, W % 32, same-size grid, >= 256 bricks (2 z x 2 y x 64 x
# for W % 64 == 0, else 2 z x 4 y x 32 x)
_fwd(DP_FWD, 1, 4, 64, (32, 32, 64), 3, "conv3d_wino2d_ps_kernel<0, 16>", "wino2d, W % 64 == 0, exactly 256 bricks")
_fwd(("fwd",), 1, 4, 40, (32, 64, 32), 3, "conv3d_wino2d_ps_kernel<0, 8>", "wino2d, W = 32, exactly 256 bricks")
_fwd(("fwd_add", "fwd_prelu", "fwd_dprelu"), 1, 4, 64, (32, 64, 32), 3, "conv3d_wino2d_ps_kernel<0, 8>",
     "wino2d, W = 32, exactly 256 bricks")
_fwd(("fwd",), 1, 4, 64, (30, 32, 64), 3, "conv3d_fwd_ws_kernel<3, 1, 4, 2, 1, 1, 4, 32>",
     "240 wino2d bricks < 256: direct loader-wave, 256 <= small, big < 512")
_fwd(("fwd",), 1, 4, 64, (32, 32, 64), 3, "conv3d_fwd_kernel<3, 1, 4, 2, 1, 1, 4, 32>",
     "x misaligned: neither wino2d nor loader-wave; 256 <= small, big < 512", mis=1)
_fwd(("fwd",), 1, 3, 64, (32, 32, 64), 3, "conv3d_fwd_ws_kernel<3, 1, 4, 2, 1, 1, 4, 32>",
     "Cin % 4 != 0: no wino2d; 256 <= small, big < 512")
# big bricks (2 x 8 x 32 / 2 x 16 x 16) x channel groups >= 512
_fwd(DP_FWD, 2, 1, 128, (32, 64, 32), 3, "conv3d_fwd_ws_kernel<3, 1, 4, 2, 4, 2, 8, 32>", "big = 512, wide, loader-wave")
_fwd(ALL_FWD, 2, 1, 128, (32, 64, 32), 3, "conv3d_fwd_kernel<3, 1, 4, 2, 4, 2, 8, 32>", "big = 512, wide, x misaligned",
     mis=1)
_fwd(("fwd",), 2, 1, 128, (32, 64, 34), 3, "conv3d_fwd_kernel<3, 1, 4, 2, 4, 2, 8, 32>", "big = 1024, wide, Wi % 4 != 0")
_fwd(("fwd",), 2, 1, 128, (30, 64, 32), 3, "conv3d_fwd_ws_kernel<3, 1, 4, 2, 1, 1, 4, 32>",
     "big = 480 < 512: 256 <= small, loader-wave")
_fwd(ALL_FWD, 2, 1, 128, (32, 128, 16), 3, "conv3d_fwd_kernel<3, 1, 4, 2, 4, 2, 8, 16>", "big = 512, Wo == 16")
_fwd(("fwd",), 2, 1, 128, (32, 112, 16), 3, "conv3d_fwd_kernel<3, 1, 4, 2, 1, 1, 4, 16>",
     "big = 448 < 512, Wo == 16: 256 <= small")
# small bricks (1 x 4 x 32 / 1 x 8 x 16) x channel groups < 256
_fwd(DP_FWD, 1, 8, 32, (8, 16, 16), 3, "conv3d_fwd_ws_kernel<3, 1, 8, 1, 1, 1, 4, 16>",
     "small < 256, Wo == 16, Cin % 8 == 0, loader-wave")
_fwd(ALL_FWD, 1, 8, 32, (8, 16, 16), 3, "conv3d_fwd_kernel<3, 1, 8, 1, 1, 1, 4, 16>",
     "small < 256, Wo == 16, Cin % 8 == 0, x misaligned", mis=2)
_fwd(ALL_FWD, 1, 12, 32, (8, 16, 16), 3, "conv3d_fwd_kernel<3, 1, 4, 1, 1, 1, 4, 16>", "small < 256, Wo == 16, Cin % 8 != 0")
_fwd(("fwd",), 1, 8, 32, (8, 16, 20), 3, "conv3d_fwd_kernel<3, 1, 4, 1, 1, 1, 4, 32>", "small < 256, Wo = 20 > 16")
_fwd(ALL_FWD, 1, 3, 20, (6, 8, 40), 3, "conv3d_fwd_kernel<3, 1, 4, 1, 1, 1, 4, 32>", "small < 256, wide")
_fwd(("fwd",), 1, 2, 128, (15, 32, 32), 3, "conv3d_fwd_kernel<3, 1, 4, 1, 1, 1, 4, 32>", "small = 240 < 256, wide")
# 256 <= small, big < 512
_fwd(DP_FWD, 1, 2, 128, (16, 32, 32), 3, "conv3d_fwd_ws_kernel<3, 1, 4, 2, 1, 1, 4, 32>", "small = 256, wide, loader-wave")
_fwd(ALL_FWD, 1, 2, 128, (16, 32, 32), 3, "conv3d_fwd_kernel<3, 1, 4, 2, 1, 1, 4, 32>", "small = 256, wide, x misaligned",
     mis=3)
_fwd(("fwd",), 1, 2, 128, (16, 32, 34), 3, "conv3d_fwd_kernel<3, 1, 4, 2, 1, 1, 4, 32>", "small = 512, wide, Wi % 4 != 0")
_fwd(ALL_FWD, 1, 2, 128, (16, 64, 16), 3, "conv3d_fwd_kernel<3, 1, 4, 2, 1, 1, 4, 16>", "small = 256, Wo == 16")
_fwd(("fwd",), 1, 2, 40, (6, 10, 14), 3, "conv3d_fwd_kernel<3, 1, 4, 1, 1, 1, 4, 16>", "pad 2 grid, small < 256", pad=2)

# ---- forward, k = 4 s 2 -------------------------------------------------------------------------------------------
# split-bf16 kernel: pad 1, wmode 0, CoutP 32 / 64, Wi % 4, aligned, >= 256 bricks of 1 x 16 x 32 outputs
_fwd(DP_FWD + ("fwd_ms",), 4, 2, 16, (128, 32, 64), 4, "conv3d_fwd_s3_kernel<1, 8, 4>", "split-bf16, CoutP 32, 256 bricks")
_fwd(ALL_FWD + ("fwd_ms",), 4, 2, 40, (128, 32, 64), 4, "conv3d_fwd_s3_kernel<2, 8, 4>", "split-bf16, CoutP 64, 256 bricks")
_fwd(("fwd",), 3, 2, 16, (170, 32, 64), 4, "conv3d_fwd_kernel<4, 2, 2, 1, 2, 1, 8, 32>",
     "255 split-bf16 bricks < 256, k4tiles 255 < 512, CoutP 32, wide")
# the 32-channel loader-wave kernel: split-bf16 takes every pad-1 wmode-0 call that it could take (its bricks are at
# least half of k4tiles), so only pad != 1 or wmode 1 reach it -- no model layer does
_fwd(DP_FWD + ("fwd_ms",), 4, 1, 8, (64, 64, 64), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 1, 4, 2, 8, 32>",
     "CoutP 32, k4tiles = 680 >= 512, pad 2 (no split-bf16)", pad=2)
_fwd(("fwd", "fwd_add"), 8, 1, 8, (64, 64, 64), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 1, 4, 2, 8, 32>",
     "CoutP 32, k4tiles = 512, wmode 1 (no split-bf16)", wmode=1)
_fwd(("fwd",), 3, 1, 8, (64, 64, 64), 4, "conv3d_fwd_kernel<4, 2, 2, 1, 2, 1, 8, 32>",
     "CoutP 32, k4tiles = 510 < 512, pad 2", pad=2)
_fwd(ALL_FWD, 1, 3, 24, (8, 16, 40), 4, "conv3d_fwd_kernel<4, 2, 2, 1, 2, 1, 8, 32>", "CoutP 32, Wo = 20 > 16")
_fwd(ALL_FWD, 1, 3, 24, (8, 16, 32), 4, "conv3d_fwd_kernel<4, 2, 2, 1, 2, 1, 8, 16>", "CoutP 32, Wo == 16")
# CoutP >= 64 without split-bf16 (CoutP 128, or too few bricks)
_fwd(ALL_FWD, 4, 1, 96, (32, 64, 64), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 2, 2, 1, 8, 32>",
     "CoutP 128, 2 k4tiles x 2 groups = 512, loader-wave")
_fwd(ALL_FWD, 4, 1, 96, (32, 64, 64), 4, "conv3d_fwd_kernel<4, 2, 2, 2, 2, 1, 8, 32>",
     "CoutP 128, big = 256, wide, x misaligned", mis=1)
_fwd(("fwd",), 4, 1, 96, (28, 64, 64), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 2, 1, 1, 4, 32>",
     "CoutP 128, 2 k4tiles x 2 groups = 448 < 512, big = 224 < 256: small, loader-wave")
_fwd(ALL_FWD, 8, 1, 128, (32, 64, 32), 4, "conv3d_fwd_kernel<4, 2, 2, 2, 2, 1, 8, 16>", "CoutP 128, big = 256, Wo == 16")
_fwd(("fwd",), 7, 1, 128, (32, 64, 32), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 2, 1, 1, 4, 16>",
     "CoutP 128, big = 224 < 256, Wo == 16: small = 896, loader-wave")
_fwd(ALL_FWD, 4, 2, 64, (32, 32, 64), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 2, 1, 1, 4, 32>",
     "CoutP 64, 64 split-bf16 bricks, big = 64 < 256, small = 256, wide, loader-wave")
_fwd(ALL_FWD, 4, 2, 64, (32, 32, 64), 4, "conv3d_fwd_kernel<4, 2, 2, 2, 1, 1, 4, 32>",
     "CoutP 64, small = 256, wide, x misaligned", mis=1)
_fwd(ALL_FWD, 4, 2, 64, (32, 64, 32), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 2, 1, 1, 4, 16>",
     "CoutP 64, small = 256, Wo == 16, loader-wave")
_fwd(ALL_FWD, 4, 2, 64, (32, 64, 32), 4, "conv3d_fwd_kernel<4, 2, 2, 2, 1, 1, 4, 16>",
     "CoutP 64, small = 256, Wo == 16, x misaligned", mis=2)
_fwd(("fwd",), 3, 2, 64, (32, 32, 64), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 1, 1, 1, 4, 32>",
     "CoutP 64, small = 192 < 256, wide, loader-wave")
_fwd(ALL_FWD, 1, 3, 50, (8, 16, 64), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 1, 1, 1, 4, 32>", "CoutP 64, small < 256, wide")
_fwd(ALL_FWD, 1, 3, 50, (8, 16, 32), 4, "conv3d_fwd_ws_kernel<4, 2, 2, 1, 1, 1, 4, 16>", "CoutP 64, small < 256, Wo == 16")
_fwd(ALL_FWD, 1, 3, 50, (8, 16, 34), 4, "conv3d_fwd_kernel<4, 2, 2, 1, 1, 1, 4, 32>",
     "CoutP 64, small < 256, Wo = 17 > 16, Wi % 4 != 0")
_fwd(("fwd",), 1, 3, 50, (8, 16, 64), 4, "conv3d_fwd_kernel<4, 2, 2, 1, 1, 1, 4, 32>",
     "CoutP 64, small < 256, wide, x misaligned", mis=2)
_fwd(ALL_FWD, 1, 3, 50, (8, 16, 32), 4, "conv3d_fwd_kernel<4, 2, 2, 1, 1, 1, 4, 16>",
     "CoutP 64, small < 256, Wo == 16, x misaligned", mis=3)

# ---- transposed, k = 4 s 2 p 1 ------------------------------------------------------------------------------------
# all-parities-in-rows kernel: <= 6 channels (row tiles 1 / 3), no PReLU output, Cin <= 64, output exactly 2 x input,
# Wi % 4, aligned, >= 16 bricks of 2 x 2 x 128 (Wi > 64) or 64 positions; Cin > 32: the 64-channel weight table
_tr(("tr", "tr_add"), 1, 8, 2, (6, 6, 128), "convtr_p8_kernel<1, 9, 32>", "p8, Cout <= 2, Wi = 128 > 64, 16 bricks")
_tr(("tr", "tr_add"), 1, 8, 1, (6, 6, 64), "convtr_p8_kernel<1, 5, 32>", "p8, Cout 1, Wi = 64, 16 bricks")
_tr(("tr", "tr_add"), 1, 8, 5, (6, 6, 128), "convtr_p8_kernel<3, 9, 32>", "p8, 3 <= Cout <= 6, Wi > 64")
_tr(("tr", "tr_add"), 1, 32, 6, (6, 6, 64), "convtr_p8_kernel<3, 5, 32>", "p8, Cout 6, Cin = 32, Wi = 64")
_tr(("tr", "tr_add"), 1, 33, 2, (6, 6, 128), "convtr_p8_kernel<1, 9, 64>", "p8, Cin = 33 > 32, Cout 2, Wi > 64")
_tr(("tr", "tr_add"), 1, 64, 1, (6, 6, 64), "convtr_p8_kernel<1, 5, 64>", "p8, Cin = 64, Cout 1, Wi = 64")
_tr(("tr", "tr_add"), 1, 40, 3, (6, 6, 128), "convtr_p8_kernel<3, 9, 64>", "p8, Cin > 32, Cout 3, Wi > 64")
_tr(("tr", "tr_add"), 1, 48, 4, (6, 6, 64), "convtr_p8_kernel<3, 5, 64>", "p8, Cin > 32, Cout 4, Wi = 64")
# the vector-ALU kernels take every other <= 6-channel call
_tr(ALL_TR, 1, 8, 1, (4, 8, 64), "convtr_valu_kernel<1, 2>", "p8 would have 15 bricks < 16")
_tr(("tr",), 1, 65, 2, (6, 6, 64), "convtr_valu_kernel<2, 2>", "Cin = 65 > 64")
_tr(ALL_TR, 2, 5, 2, (3, 5, 7), "convtr_valu_kernel<2, 2>", "odd extents", odd=(1, 1, 1))
_tr(("tr",), 1, 8, 4, (6, 6, 66), "convtr_valu_kernel<4, 2>", "Wi % 4 != 0")
_tr(ALL_TR, 1, 6, 3, (3, 4, 8), "convtr_valu_kernel<4, 2>", "Cout 3, 3 bricks")
_tr(("tr",), 1, 8, 6, (6, 6, 64), "convtr_valu_kernel<6, 2>", "x misaligned", mis=1)
_tr(ALL_TR, 1, 8, 5, (4, 6, 8), "convtr_valu_kernel<6, 2>", "Cout 5, odd output W", odd=(0, 0, 1))
_tr(("tr_prelu",), 1, 8, 6, (6, 6, 64), "convtr_valu_kernel<6, 2>", "PReLU output: never p8")
# 7..16 channels: the 16-row split-bf16 form (output exactly 2 x input, >= 256 bricks of 2 x 3 x 32 input positions),
# else the 16-channel class kernels (loader-wave with >= 128 bricks of 2 x 2 x 32 output classes)
_tr(ALL_TR, 4, 4, 12, (16, 24, 32), "convtr_s3_kernel<true>", "7..16 channels, 256 split-bf16 bricks")
_tr(("tr",), 4, 4, 7, (14, 24, 32), "convtr_mfma16_ws_kernel<2, 2>", "224 split-bf16 bricks < 256, 336 bricks >= 128")
_tr(ALL_TR, 4, 4, 16, (16, 24, 32), "convtr_mfma16_ws_kernel<2, 2>", "output W = 2 Wi + 1: no split-bf16", odd=(0, 0, 1))
_tr(("tr",), 2, 4, 9, (16, 16, 32), "convtr_mfma16_ws_kernel<2, 2>", "exactly 128 bricks")
_tr(("tr",), 2, 4, 9, (16, 14, 32), "convtr_mfma16_kernel<2, 2>", "112 bricks < 128")
_tr(ALL_TR, 1, 4, 10, (4, 6, 16), "convtr_mfma16_kernel<2, 2>", "6 bricks")
_tr(("tr",), 4, 4, 12, (16, 24, 32), "convtr_mfma16_kernel<2, 2>", "x misaligned", mis=2)
# 17..32 channels and 32-channel slices
_tr(ALL_TR, 4, 4, 24, (16, 24, 32), "convtr_s3_kernel<false>", "17..32 channels, 256 split-bf16 bricks")
_tr(("tr", "tr_prelu"), 2, 4, 64, (16, 24, 32), "convtr_s3_kernel<false>", "2 slices x 128 split-bf16 bricks = 256")
_tr(("tr",), 1, 4, 64, (16, 24, 32), "convtr_mfma_ws_kernel<2, 2>", "2 slices x 64 split-bf16 bricks < 256")
_tr(("tr",), 4, 4, 17, (14, 24, 32), "convtr_mfma_ws_kernel<2, 2>", "224 split-bf16 bricks < 256")
_tr(ALL_TR, 4, 4, 32, (16, 24, 32), "convtr_mfma_ws_kernel<2, 2>", "output W = 2 Wi + 1", odd=(0, 0, 1))
_tr(("tr",), 1, 4, 96, (16, 16, 32), "convtr_mfma_ws_kernel<2, 2>", "3 slices x 64 bricks = 192 >= 128")
_tr(("tr",), 1, 4, 64, (16, 16, 32), "convtr_mfma_kernel<2, 2>", "2 slices x 64 bricks = 128, x misaligned", mis=1)
_tr(("tr",), 1, 4, 32, (16, 16, 32), "convtr_mfma_kernel<2, 2>", "64 bricks < 128")
_tr(ALL_TR, 1, 4, 20, (4, 6, 16), "convtr_mfma_kernel<2, 2>", "6 bricks, odd output D", odd=(1, 0, 0))

# ---- weight gradient ------------------------------------------------------------------------------------------------
# loader-wave kernels need pad <= stride, Wo >= 32 or == 16, Wo % 4, Wi % 4, aligned g and src
_wrw(BOTH_WRW, 1, 64, 64, (16, 128, 64), 3, "conv3d_wrw_wino4_kernel<0>",
     "64 -> 64 k3, W % 64, 1024 bricks of 1 x 2 x 64")
_wrw(("wrw",), 1, 64, 64, (15, 128, 64), 3, "conv3d_wrw_dma_kernel<3, 1, 16, 2, 1, 4, 3, 1, 32>",
     "64 -> 64 k3 with 960 Winograd bricks < 1024")
_wrw(BOTH_WRW, 1, 8, 40, (4, 8, 32), 3, "conv3d_wrw_dma_kernel<3, 1, 16, 2, 1, 4, 3, 1, 32>", "k3, Cg > 32, Cs >= 8, Wo >= 32")
_wrw(BOTH_WRW, 1, 8, 40, (4, 8, 16), 3, "conv3d_wrw_dma_kernel<3, 1, 16, 2, 1, 4, 3, 1, 16>", "k3, Cg > 32, Cs >= 8, Wo == 16")
_wrw(("wrw",), 1, 7, 40, (4, 8, 32), 3, "conv3d_wrw_brick_kernel<3, 1, 8, 2, 1, 4>", "k3, Cs = 7 < 8, Cg > 32")
_wrw(("wrw",), 1, 8, 32, (4, 8, 32), 3, "conv3d_wrw_brick_kernel<3, 1, 8, 1, 1, 4>", "k3, Cg = 32")
_wrw(BOTH_WRW, 1, 8, 40, (4, 8, 20), 3, "conv3d_wrw_brick_kernel<3, 1, 8, 2, 1, 4>", "k3, Wo = 20: neither 16 nor >= 32")
_wrw(BOTH_WRW, 1, 5, 24, (4, 6, 12), 3, "conv3d_wrw_brick_kernel<3, 1, 8, 1, 1, 4>", "k3, Cg <= 32")
_wrw(("wrw",), 1, 8, 40, (4, 8, 32), 3, "conv3d_wrw_brick_kernel<3, 1, 8, 2, 1, 4>", "k3, g misaligned", mis=1)
_wrw(("wrw",), 1, 8, 40, (4, 8, 32), 3, "conv3d_wrw_brick_kernel<3, 1, 8, 2, 1, 4>", "k3, src misaligned", mis2=2)
_wrw(("wrw",), 1, 8, 40, (4, 8, 32), 3, "conv3d_wrw_brick_kernel<3, 1, 8, 2, 1, 4>", "k3, pad 2 > stride", pad=2,
     inp=(2, 6, 30))
# k = 4 s 2: split-bf16 for >= 3 (Cg <= 32) / >= 4 (Cg > 32) source channels
_wrw(BOTH_WRW, 1, 4, 40, (4, 8, 16), 4, "conv3d_wrw_s3_kernel<8, 2, 1, 2, 4, 0, 16>", "k4, Cg > 32, Cs = 4, Wo == 16")
_wrw(BOTH_WRW, 1, 4, 40, (4, 8, 32), 4, "conv3d_wrw_s3_kernel<8, 2, 1, 2, 4, 0, 32>", "k4, Cg > 32, Cs = 4, Wo >= 32")
_wrw(BOTH_WRW, 1, 3, 32, (4, 6, 32), 4, "conv3d_wrw_s3_kernel<6, 1, 2, 2, 3, 0, 32>", "k4, Cg = 32, Cs = 3, Wo >= 32")
_wrw(("wrw_ms",), 1, 5, 24, (4, 6, 32), 4, "conv3d_wrw_s3_kernel<6, 1, 2, 2, 3, 0, 32>", "k4 multi-source planes")
_wrw(("wrw",), 1, 3, 32, (4, 6, 16), 4, "conv3d_wrw_brick_kernel<4, 2, 4, 1, 1, 2>",
     "k4, Cg <= 32, Wo == 16: no loader-wave form; cost2 = cost4 = 2")
_wrw(BOTH_WRW, 1, 2, 32, (4, 6, 32), 4, "conv3d_wrw_dma_kernel<4, 2, 2, 1, 2, 2, 1, 0, 32>", "k4, Cg <= 32, Cs = 2 < 3")
_wrw(("wrw",), 1, 1, 8, (4, 6, 64), 4, "conv3d_wrw_dma_kernel<4, 2, 2, 1, 2, 2, 1, 0, 32>", "k4, Cs = 1, Wo = 64")
_wrw(("wrw",), 1, 3, 40, (4, 8, 32), 4, "conv3d_wrw_brick_kernel<4, 2, 4, 2, 1, 2>",
     "k4, Cg > 32, Cs = 3 < 4: brick; cost2 = cost4 = 2")
_wrw(BOTH_WRW, 1, 2, 40, (4, 8, 32), 4, "conv3d_wrw_brick_kernel<4, 2, 2, 2, 1, 2>", "k4, Cg > 32, Cs = 2: cost2 1 < cost4 2")
_wrw(BOTH_WRW, 1, 5, 24, (4, 6, 20), 4, "conv3d_wrw_brick_kernel<4, 2, 2, 1, 1, 2>", "k4, Wo = 20, Cs = 5: cost2 3 < cost4 4")
_wrw(BOTH_WRW, 1, 4, 24, (4, 6, 20), 4, "conv3d_wrw_brick_kernel<4, 2, 4, 1, 1, 2>", "k4, Wo = 20, Cs = 4: cost2 = cost4")
_wrw(BOTH_WRW, 1, 7, 40, (3, 5, 12), 4, "conv3d_wrw_brick_kernel<4, 2, 4, 2, 1, 2>", "k4, Cg > 32, Cs = 7: cost2 = cost4 = 4")
_wrw(("wrw",), 1, 4, 40, (4, 8, 32), 4, "conv3d_wrw_brick_kernel<4, 2, 4, 2, 1, 2>", "k4, src misaligned", mis2=1)
_wrw(("wrw",), 1, 3, 32, (4, 6, 32), 4, "conv3d_wrw_brick_kernel<4, 2, 4, 1, 1, 2>", "k4, g misaligned", mis=3)
_wrw(("wrw",), 1, 3, 32, (4, 6, 32), 4, "conv3d_wrw_brick_kernel<4, 2, 4, 1, 1, 2>", "k4, Wi % 4 != 0 (src W 66)",
     inp=(8, 12, 66))

# Compute kernels of the product build that no call of the product library can reach.
UNREACHABLE_IN_PRODUCT = {
    "convtr_p8_kernel<6, 5, 32>": "7..12 channels reach the all-parities kernel only with FLOWSCI_TR_P8_ALL, an ablation "
                                  "switch (FS_AB_ENV is constant false in the product build)",
    "conv3d_wrw_dma_kernel<4, 2, 8, 2, 1, 2, 4, 0, 16>": "the split-bf16 pick under the same condition comes first; only the "
                                                         "ablation build's FLOWSCI_WRW_NO_S3 reaches it",
    "conv3d_wrw_dma_kernel<4, 2, 8, 2, 1, 2, 4, 0, 32>": "the split-bf16 pick under the same condition comes first; only the "
                                                         "ablation build's FLOWSCI_WRW_NO_S3 reaches it",
    "conv3d_wrw_dma_kernel<4, 2, 6, 1, 2, 2, 3, 0, 32>": "the split-bf16 pick under the same condition comes first (plain and "
                                                         "multi-source); only the ablation build's FLOWSCI_WRW_NO_S3 reaches it",
}

# Kernels the three files compile that are not convolution compute kernels (weight re-layout, reductions, the finish
# passes of the fused PReLU-backward and deterministic weight-gradient epilogues).
HELPERS = {"fs::reduce_final_kernel", "wprep_one_kernel", "wprep_batch_kernel", "dprelu_finish1_kernel",
           "dprelu_finish2_kernel", "wrw_reduce_kernel"}

# the library's plan per kernel family: FS_WPREP_* slab kind (fwd / tr, None: no re-layout job) or FS_WRW_KERNEL_* id
PLAN_OF = {
    "conv3d_wino2d_ps_kernel": 6, "conv3d_fwd_s3_kernel": 7, "conv3d_fwd_kernel": 0, "conv3d_fwd_ws_kernel": 0,
    "convtr_p8_kernel": 3, "convtr_valu_kernel": None, "convtr_s3_kernel<true>": 9, "convtr_s3_kernel<false>": 8,
    "convtr_mfma16_kernel": 2, "convtr_mfma16_ws_kernel": 2, "convtr_mfma_kernel": 1, "convtr_mfma_ws_kernel": 1,
    "conv3d_wrw_brick_kernel": 0, "conv3d_wrw_dma_kernel": 1, "conv3d_wrw_wino4_kernel": 3, "conv3d_wrw_s3_kernel": 4,
}


def plan_of(kernel):
    return PLAN_OF[kernel] if kernel in PLAN_OF else PLAN_OF[kernel.split("<")[0]]


def row_id(r):
    return "%s-%s-B%d-%dx%d-%s-%s-p%d-w%d-m%d%d" % (r["op"], r["kernel"].split("<")[0], r["B"], r["cin"], r["cout"],
                                                   "x".join(map(str, r["inp"])), "x".join(map(str, r["out"])), r["pad"],
                                                   r["wmode"], r["mis"], r["mis2"])
