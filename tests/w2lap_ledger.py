"""Ledger of the 2-D warp, occlusion and Laplacian-pyramid kernels' dispatch cases: one row per call of one C-ABI entry
point of csrc/warp2d.hip (fs_warp2d_fwd / _bwd, fs_warp2d_pair_fwd / _bwd, fs_occ_check2d), csrc/laplacian.hip
(fs_laploss2d_fwd / _bwd) and csrc/laplacian3d.hip (fs_laploss3d_fwd / _bwd), with the compute kernel(s) the dispatch code
(slices_for, grid_for, launch_fwd, launch_bwd; the per-level loops of the pyramids) must launch for it.  Plain data, read
by tests/test_w2lap_ledger.py (every compiled kernel has a row, a restatement of the dispatch predicts each row's kernels,
the inputs keep their margins and the fp32 oracle inside the band) and tests/test_gpu_w2lap_ledger.py (the named kernels
run and nothing else, every output matches an fp64 reference or an exact expectation at every element inside NaN-patterned
guard bands).  tests/w2lap_ledger_inputs.py builds each row's inputs and references.

Row fields:
  op       w_fwd w_bwd (fs_warp2d_*), wp_fwd wp_bwd (fs_warp2d_pair_*), occ (fs_occ_check2d), l2_fwd l2_bwd
           (fs_laploss2d_*), l3_fwd l3_bwd (fs_laploss3d_*)
  B, C     warps and occ (C = 2 there); the pyramids' N is B, C stays 1
  ext      warps / occ: extent (H, W) of the flow == of the output; pyramids: (H, W) or (D, H, W) of the input
  inp      warps: extent of the sampled image when it differs from the flow's (RIFE only), else None
  mode     warps: FS_WARP2D_* (0 RIFE, 1 PWC, 2 PHOTO, 3 DILATED); occ: FS_OCC_* (0 ALL, 1 OBJ, 2 OUT)
  mask     with_mask; start: a `start` tensor is passed (DILATED)
  gin, gflow   which gradients the backward is asked for; alias: grad_img0 IS grad_img1 (pair)
  flow     the kind the flow is built from (w2lap_ledger_inputs.FLOW_KINDS); "dyadic" on every masked row, "integer"
           on the exact occlusion row
  levels, target (pyramids: a target is passed), gl (grad_loss), data ("randn", "cb": a unit checkerboard, which the
           binomial filter annihilates exactly, plus 0.1 x noise: |lap| stays near 1 on rows too long for a seed search;
           "same": input == target), margin (the |lap| margin the forward row's seed search promises: 1e-5, and 1e-3 on the
           "cb" rows, whose |lap| is near 1 and whose spike makes the fp32 error of lap as large as 4e-6), spike (100 is
           added to the last element: the far side of a cap)
  nc       (NC, CG) the plane-owner launch must use, where the row is about them
  mis      {operand name: misalignment in floats, 0..3}
  kernel   the expected compute kernel symbols, in launch order (one each, however often a pyramid launches it)
  why      the rung

Shapes are as small as the rung allows; the rows on the two sides of a threshold differ in one quantity.

What reading the dispatch code decided (the rows pin each of these):
  * every kernel of the three sources makes 4-byte accesses only, so no operand's alignment is inspected and the rows
    "every operand misaligned" run the same kernel to the same result.
  * launch_bwd with grad_in and a plane that fits launches TWO kernels when grad_flow is asked for (the gather kernel
    <.., false, SL> and the plane owner) and the plane owner alone otherwise; the atomic kernel <.., true, SL> is left to
    planes above 48 KB and to a pair whose grad_img0 == grad_img1.  For RIFE the plane is the sampled image's (in_hw),
    not the flow's.
  * the plane owner adds into grad_in with plain read-modify-writes and the atomic kernel with float atomics: grad_in is
    held to the gradient band, not to equal bits; grad_flow is deterministic and every backward row runs twice for it.
  * with_mask parity is claimed on "dyadic" inputs only (W - 1 and H - 1 powers of two, flows odd multiples of 1/8: the
    coordinate and weight chain is exact in fp32, so the mask decision is the same in any arithmetic and every pixel is
    compared).  On generic flows the mask of a fully interior sample is decided by fp32 rounding; parity stays
    undefined there and is not claimed.
  * the sampled images of extents above 65 are smooth ("wave"): the fp32 coordinate chain of the normalising modes is
    off by about W x 2^-23 px, which times the slope of white noise would leave the output band at such widths in the
    project's own fp32 oracle as well.

Not walked: the 3-D pyramid's grid cap (65536 blocks: more than 16.7 M voxels for the fine kernels, 134 M for the coarse
ones) and its levels 7 and 8 (129 and 257 voxels per axis: 2.1 M and 17 M voxels), and the 2-D coarse kernels' grid cap
(lap_down_kernel / lap_up_adj_kernel: a coarse count above 4 194 304 needs 3 x 4 194 305 fine floats; the fp64 reference
of those 12.6 M elements alone takes 2 s forward and 3.5 s backward on the CPU, before the fp32 oracle) -- too large for a
test of a few seconds."""
from ledger_harness import normalize  # noqa: F401  (the names these sources' kernels go by need nothing more)

ROWS = []
RIFE, PWC, PHOTO, DILATED = 0, 1, 2, 3
OCC_ALL, OCC_OBJ, OCC_OUT = 0, 1, 2
FORMS = ((RIFE, 0), (PWC, 0), (PWC, 1), (PHOTO, 0), (DILATED, 0))  # the five (MODE, MASK) instantiations
MODE_NAMES = {RIFE: "RIFE", PWC: "PWC", PHOTO: "PHOTO", DILATED: "DILATED"}
WARP_OPS = ("w_fwd", "w_bwd", "wp_fwd", "wp_bwd")
PAIR_OPS = ("wp_fwd", "wp_bwd")
BWD_OPS = ("w_bwd", "wp_bwd")
LAP_OPS = ("l2_fwd", "l2_bwd", "l3_fwd", "l3_bwd")
OPS = WARP_OPS + ("occ",) + LAP_OPS
PREFIXES = ("warp2d_", "occ_check2d_", "lap_", "lap3_")  # the witness filter

_b = lambda v: "true" if v else "false"


def FWD(mode, mask, sl):
    return "warp2d_fwd_kernel<%d, %s, %d>" % (mode, _b(mask), sl)


def BWD(mode, mask, gin, sl):
    return "warp2d_bwd_kernel<%d, %s, %s, %d>" % (mode, _b(mask), _b(gin), sl)


def PLANE(mode, mask):
    return "warp2d_gin_plane_kernel<%d, %s>" % (mode, _b(mask))


OCC = "occ_check2d_kernel"
L2_FWD = ("lap_down_kernel", "lap_level_kernel")
L2_BWD = ("lap_up_adj_kernel", "lap_down_adj_kernel")
L3_FWD = ("lap3_down_kernel", "lap3_level_kernel")
L3_BWD = ("lap3_up_adj_kernel", "lap3_down_adj_kernel")


def _row(op, kernel, why, ext, B=1, C=1, mode=PWC, mask=0, inp=None, start=False, gin=False, gflow=True, alias=False,
         flow="smooth", levels=0, target=True, gl=1.0, data="randn", margin=1e-5, spike=False, nc=None, mis=None):
    ROWS.append(dict(op=op, kernel=kernel if isinstance(kernel, tuple) else (kernel,), why=why, ext=tuple(ext), B=B, C=C,
                     mode=mode, mask=mask, inp=tuple(inp) if inp else None, start=start, gin=gin, gflow=gflow, alias=alias,
                     flow="dyadic" if mask else flow, levels=levels, target=target, gl=gl, data=data, margin=margin,
                     spike=spike, nc=nc, mis=dict(mis or {})))


# ---- warp2d.hip: slices_for, walked once with unmasked PWC ------------------------------------------------------------
_row("w_fwd", FWD(PWC, 0, 1), "slices: C = 3 < 4 at small n -> 1", (5, 9), B=2, C=3)
_row("w_fwd", FWD(PWC, 0, 4), "slices: C = 4 at small n -> 4", (5, 9), B=2, C=4, flow="noise")
_row("w_fwd", FWD(PWC, 0, 4), "slices: C = 15 < 16 at n < 32768 -> 4", (5, 9), B=2, C=15, flow="shift")
_row("w_fwd", FWD(PWC, 0, 16), "slices: C = 16 at n < 32768 -> 16", (5, 9), B=2, C=16, flow="shift")
_row("w_fwd", FWD(PWC, 0, 16), "slices: n = 32767 (217 x 151) with C = 16 -> 16", (217, 151), C=16)
_row("w_fwd", FWD(PWC, 0, 4), "slices: n = 32768 (128 x 256) with C = 16 -> 4", (128, 256), C=16)
_row("w_fwd", FWD(PWC, 0, 4), "slices: n = 131071 (1 x 131071) with C = 4 -> 4", (1, 131071), C=4)
_row("w_fwd", FWD(PWC, 0, 1), "slices: n = 131072 (256 x 512) with C = 4 -> 1", (256, 512), C=4)
# ---- every remaining forward instantiation ----------------------------------------------------------------------------
for _mode, _mask in FORMS:
    for _sl, _c in ((1, 3), (4, 5), (16, 17)):
        if (_mode, _mask) == (PWC, 0):
            continue
        _row("w_fwd", FWD(_mode, _mask, _sl), "forward %s%s with %d slices (C = %d)%s" % (
            MODE_NAMES[_mode], " masked" if _mask else "", _sl, _c,
            ", start given together with slices" if _mode == DILATED and _sl > 1 else ""),
             (2, 2) if (_mode, _sl) == (RIFE, 1) else (9, 17), B=2, C=_c, mode=_mode, mask=_mask,
             start=_mode == DILATED and _sl > 1, flow=("smooth", "noise", "shift")[_sl % 3])
# ---- backward form ----------------------------------------------------------------------------------------------------
_row("w_bwd", PLANE(PWC, 0), "backward form: grad_in only -> the plane kernel alone; B*C = 6 < 512: nc = 1", (5, 9), B=2, C=3,
     gin=True, gflow=False, nc=(1, 3))
_row("w_bwd", BWD(PWC, 0, 0, 1), "backward form: grad_flow only", (5, 9), B=2, C=3)
_row("w_bwd", (BWD(PWC, 0, 0, 1), PLANE(PWC, 0)), "backward form: both, the plane fits -> gather kernel + plane kernel",
     (5, 9), B=2, C=3, gin=True, flow="noise")
_row("w_bwd", (BWD(PWC, 0, 0, 4), PLANE(PWC, 0)), "48 KB switch: Hi*Wi = 12288 (96 x 128) fits", (96, 128), C=4, gin=True)
_row("w_bwd", BWD(PWC, 0, 1, 4), "48 KB switch: 96 x 129 does not fit -> both from the atomic kernel", (96, 129), C=4,
     gin=True)
_row("w_bwd", BWD(PWC, 0, 1, 4), "backward form: grad_in only, the plane does not fit -> atomic kernel with a null "
     "grad_flow", (96, 129), C=4, gin=True, gflow=False)
# all 15 <.., false, SL> with their plane kernel (a C that nc = 2 does not divide: B*C >= 1024), all 15 <.., true, SL>
for _mode, _mask in FORMS:
    for _sl, _c in ((1, 3), (4, 5), (16, 17)):
        _k = MODE_NAMES[_mode] + (" masked" if _mask else "")
        if _sl == 16:
            _row("w_bwd", (BWD(_mode, _mask, 0, 16), PLANE(_mode, _mask)), "plane kernel %s: B*C = 1088, fill = 2 -> nc = 2 "
                 "does not divide C = 17 (CG = 9, the last group has 1 channel); 16 slices" % _k, (3, 5), B=64, C=17,
                 mode=_mode, mask=_mask, gin=True, nc=(2, 9), start=_mode == DILATED, flow="noise")
        else:
            _row("w_bwd", (BWD(_mode, _mask, 0, _sl), PLANE(_mode, _mask)), "backward %s, gather kernel with %d slices + "
                 "plane kernel" % (_k, _sl), (9, 17), B=2, C=_c, mode=_mode, mask=_mask, gin=True,
                 flow=("shift", "smooth")[_sl % 2])
        _row("w_bwd", BWD(_mode, _mask, 1, _sl), "atomic grad_in %s with %d slices (plane above 48 KB%s)" % (
            _k, _sl, ", start given together with slices" if _mode == DILATED and _sl > 1 else ""),
             (65, 257) if _mask else (96, 129), C=_c, mode=_mode, mask=_mask, gin=True, start=_mode == DILATED and _sl > 1)
# ---- RIFE: the sampled image's extent decides the switch ----------------------------------------------------------------
_row("w_bwd", BWD(RIFE, 0, 1, 1), "RIFE in_hw: the flow's plane fits (96 x 128), the image's does not (96 x 129) -> atomic",
     (96, 128), C=2, mode=RIFE, inp=(96, 129), gin=True)
_row("w_bwd", (BWD(RIFE, 0, 0, 1), PLANE(RIFE, 0)), "RIFE in_hw: the flow's plane does not fit (96 x 129), the image's "
     "does (96 x 128) -> plane kernel", (96, 129), C=2, mode=RIFE, inp=(96, 128), gin=True)
_row("w_fwd", FWD(RIFE, 0, 1), "RIFE in_hw: forward, image larger than the flow", (7, 10), B=2, C=3, mode=RIFE, inp=(9, 13))
# ---- nc / fill / CG -------------------------------------------------------------------------------------------------------
_row("w_bwd", PLANE(PWC, 0), "nc: B*C = 1024 (B = 512, C = 2), plane <= 24 KB -> fill = 2, nc = 2, CG = 1", (3, 8), B=512,
     C=2, gin=True, gflow=False, nc=(2, 1))
_row("w_bwd", PLANE(PWC, 0), "nc: B*C = 1022 (B = 511, C = 2) -> fill = 1, nc = 1, CG = 2", (3, 8), B=511, C=2, gin=True,
     gflow=False, nc=(1, 2))
_row("w_bwd", (BWD(PWC, 0, 0, 16), PLANE(PWC, 0)), "nc: the C3 level shape 32 x 196 x 3 x 8 -> nc = 12, CG = 17, the last "
     "group has 4 channels", (3, 8), B=32, C=196, gin=True, nc=(12, 17))
_row("w_bwd", PLANE(PWC, 0), "nc: B = 1024, C = 1 -> fill = 2 is cut to C = 1", (3, 8), B=1024, C=1, gin=True, gflow=False,
     nc=(1, 1))
# ---- pair launches ----------------------------------------------------------------------------------------------------
_row("wp_fwd", FWD(RIFE, 0, 1), "pair forward RIFE (blockIdx.y, the 4-channel flow in place)", (5, 9), B=2, C=3, mode=RIFE)
_row("wp_fwd", FWD(PHOTO, 0, 4), "pair forward PHOTO: flowC = 4 indexing in another mode", (5, 9), B=2, C=4, mode=PHOTO,
     flow="noise")
_row("wp_bwd", (BWD(RIFE, 0, 0, 1), PLANE(RIFE, 0)), "pair backward RIFE, distinct grad_img tensors -> plane kernel", (5, 9),
     B=2, C=3, mode=RIFE, gin=True)
_row("wp_bwd", BWD(RIFE, 0, 1, 1), "pair backward RIFE, grad_img0 == grad_img1 (aliased) -> atomic kernel; the one buffer "
     "holds the sum of both gradients", (5, 9), B=2, C=3, mode=RIFE, gin=True, alias=True)
_row("wp_bwd", BWD(RIFE, 0, 0, 1), "pair backward RIFE, grad_flow4 only", (5, 9), B=2, C=3, mode=RIFE, flow="noise")
_row("wp_bwd", (BWD(PHOTO, 0, 0, 4), PLANE(PHOTO, 0)), "pair backward PHOTO: flowC = 4 indexing in another mode", (5, 9),
     B=2, C=4, mode=PHOTO, gin=True, flow="noise")
# ---- grid cap (16384 blocks of 256 pixels) ----------------------------------------------------------------------------------
_row("w_fwd", FWD(PWC, 0, 1), "grid cap: n = 4194304 (2048 x 2048), one trip", (2048, 2048))
_row("w_fwd", FWD(PWC, 0, 1), "grid cap: n = 4194305 (1985 x 2113), second trip of the grid-stride loop", (1985, 2113))
_row("w_bwd", BWD(PWC, 0, 0, 1), "grid cap backward: n = 4194304, one trip", (2048, 2048))
_row("w_bwd", BWD(PWC, 0, 0, 1), "grid cap backward: n = 4194305, second trip", (1985, 2113))
# (DILATED with a constant dyadic shift: its coordinates are then exact sums; any fp32 coordinate chain is off by ~2e-4 px
# at this width otherwise, which times an O(1) grad_out is the whole gradient band of grad_in in the fp32 oracle as well)
_row("w_bwd", BWD(DILATED, 0, 1, 1), "grid cap backward: n = 4194305 with grad_in through the atomic kernel (DILATED)",
     (1985, 2113), mode=DILATED, gin=True, flow="shift")
# ---- DILATED ----------------------------------------------------------------------------------------------------------------
_row("w_fwd", FWD(DILATED, 0, 1), "DILATED: start NULL, samples clamped on all four sides", (9, 17), B=2, C=3, mode=DILATED,
     flow="wide")
_row("w_fwd", FWD(DILATED, 0, 1), "DILATED: start given, samples clamped on all four sides", (9, 17), B=2, C=3, mode=DILATED,
     start=True, flow="wide")
_row("w_bwd", (BWD(DILATED, 0, 0, 1), PLANE(DILATED, 0)), "DILATED backward: start given, clamped on all four sides", (9, 17),
     B=2, C=3, mode=DILATED, start=True, gin=True, flow="wide")
# ---- tiny extents -------------------------------------------------------------------------------------------------------------
for _mode in (PWC, PHOTO, DILATED):
    for _ext in ((1, 1), (1, 7), (6, 1)):
        _row("w_fwd", FWD(_mode, 0, 1), "tiny: %s at %d x %d" % (MODE_NAMES[_mode], *_ext), _ext, B=2, C=2, mode=_mode,
             flow="small")
        _row("w_bwd", (BWD(_mode, 0, 0, 1), PLANE(_mode, 0)), "tiny backward: %s at %d x %d" % (MODE_NAMES[_mode], *_ext),
             _ext, B=2, C=2, mode=_mode, gin=True, flow="small")
_row("w_bwd", (BWD(RIFE, 0, 0, 1), PLANE(RIFE, 0)), "tiny backward: RIFE at 2 x 2", (2, 2), B=2, C=2, mode=RIFE, gin=True,
     flow="small")
# ---- every operand misaligned ---------------------------------------------------------------------------------------------
_row("w_fwd", FWD(DILATED, 0, 4), "fs_warp2d_fwd, every operand misaligned (4-byte accesses only: same kernel)", (9, 17),
     B=2, C=4, mode=DILATED, start=True, mis={"in0": 1, "flow": 2, "start": 3, "out0": 1})
_row("w_bwd", (BWD(DILATED, 0, 0, 4), PLANE(DILATED, 0)), "fs_warp2d_bwd, every operand misaligned", (9, 17), B=2, C=4,
     mode=DILATED, start=True, gin=True, mis={"in0": 3, "flow": 1, "start": 2, "gout0": 1, "gin0": 2, "gflow": 3})
_row("wp_fwd", FWD(RIFE, 0, 1), "fs_warp2d_pair_fwd, every operand misaligned", (5, 9), B=2, C=3, mode=RIFE,
     mis={"in0": 1, "in1": 2, "flow": 3, "out0": 2, "out1": 1})
_row("wp_bwd", (BWD(RIFE, 0, 0, 1), PLANE(RIFE, 0)), "fs_warp2d_pair_bwd, every operand misaligned", (5, 9), B=2, C=3,
     mode=RIFE, gin=True, mis={"in0": 2, "in1": 1, "flow": 1, "gout0": 3, "gout1": 2, "gin0": 1, "gin1": 3, "gflow": 2})

# ---- occ_check2d ------------------------------------------------------------------------------------------------------------
for _m, _n in ((OCC_ALL, "ALL"), (OCC_OBJ, "OBJ"), (OCC_OUT, "OUT")):
    _row("occ", OCC, "occ mode %s at B = 2 on a ragged shape" % _n, (13, 19), B=2, C=2, mode=_m, flow="occ")
_row("occ", OCC, "occ: H = 1 (dH = max(H - 1, 1)), mode ALL: every sample leaves the row, OBJ would be 1 everywhere", (1, 23), B=2, C=2, mode=OCC_ALL, flow="occ")
_row("occ", OCC, "occ: W = 1 (dW = max(W - 1, 1)), mode ALL", (21, 1), B=2, C=2, mode=OCC_ALL, flow="occ")
_row("occ", OCC, "occ grid cap: n = 4194304, one trip", (2048, 2048), C=2, mode=OCC_OBJ, flow="occ")
_row("occ", OCC, "occ grid cap: n = 4194305, second trip", (1985, 2113), C=2, mode=OCC_OBJ, flow="occ")
_row("occ", OCC, "fs_occ_check2d, every operand misaligned", (13, 19), B=2, C=2, mode=OCC_OBJ, flow="occ",
     mis={"flow_f": 1, "flow_b": 2, "occ_f": 3, "occ_b": 1})
_row("occ", OCC, "occ exact: integer flows that land exactly on 0 and on n - 1 stay 1 (strict comparisons)", (6, 11), B=2,
     C=2, mode=OCC_OUT, flow="integer")

# ---- Laplacian pyramids -------------------------------------------------------------------------------------------------------
for _ext, _n in (((3, 3), 1), ((3, 3), 3), ((3, 9), 1), ((3, 9), 3), ((4, 7), 2), ((5, 8), 2), ((6, 5), 2), ((8, 3), 2),
                 ((9, 4), 2), ((7, 6), 2)):
    _row("l2_fwd", L2_FWD, "2-D extents %d x %d, levels = 1, N = %d" % (*_ext, _n), _ext, B=_n, levels=1,
         target=(_ext[0] + _n) % 2 == 0)
    _row("l2_bwd", L2_BWD, "2-D backward extents %d x %d, levels = 1, N = %d" % (*_ext, _n), _ext, B=_n, levels=1,
         gl=(1.0, -2.5)[_n % 2])
for _lv in (1, 2, 3, 4):
    _row("l2_fwd", L2_FWD, "2-D levels: 17 x 33 at levels = %d (17, 9, 5, 3)" % _lv, (17, 33), B=2, levels=_lv,
         target=_lv % 2 == 0)
    _row("l2_bwd", L2_BWD, "2-D backward levels: 17 x 33 at levels = %d" % _lv, (17, 33), B=2, levels=_lv,
         gl=(1.0, -2.5)[_lv % 2])
_row("l2_fwd", L2_FWD, "2-D levels: 257 x 257 at levels = 8 (kMaxLevels)", (257, 257), levels=8)
_row("l2_bwd", L2_BWD, "2-D backward levels: 257 x 257 at levels = 8 (kMaxLevels)", (257, 257), levels=8, gl=-2.5)
_row("l2_fwd", L2_FWD, "2-D target NULL", (7, 6), B=3, levels=1, target=False)
_row("l2_fwd", L2_FWD, "2-D target given", (7, 6), B=3, levels=1, target=True)
_row("l2_fwd", L2_FWD, "2-D partial-sum cap: N*H*W = 131072 (256 x 512): 512 blocks, one trip", (256, 512), levels=1,
     data="cb", margin=1e-3)
_row("l2_fwd", L2_FWD, "2-D partial-sum cap: N*H*W = 131073 (3 x 43691): second trip of lap_level_kernel", (3, 43691),
     levels=1, data="cb", margin=1e-3, spike=True)
_row("l2_fwd", L2_FWD, "2-D grid cap, fine kernels: N*H*W = 4194304 (2048 x 2048)", (2048, 2048), levels=1, data="cb", margin=1e-3)
_row("l2_fwd", L2_FWD, "2-D grid cap, fine kernels: N*H*W = 4194306 (3 x 1398102), second trip", (3, 1398102), levels=1,
     data="cb", margin=1e-3, spike=True)
_row("l2_bwd", L2_BWD, "2-D backward grid cap, fine kernels: N*H*W = 4194304 (2048 x 2048)", (2048, 2048), levels=1)
_row("l2_bwd", L2_BWD, "2-D backward grid cap, fine kernels: N*H*W = 4194306 (3 x 1398102), second trip", (3, 1398102),
     levels=1)
_row("l2_fwd", L2_FWD, "2-D exact: input == target gives loss 0 and sgn 0", (9, 12), B=2, levels=2, data="same")
_row("l2_fwd", L2_FWD, "fs_laploss2d_fwd, every operand misaligned", (9, 12), B=2, levels=2,
     mis={"input": 1, "target": 2, "sgn": 3, "ws": 1, "loss": 2})
_row("l2_bwd", L2_BWD, "fs_laploss2d_bwd, every operand misaligned", (9, 12), B=2, levels=2, gl=-2.5,
     mis={"sgn": 1, "gl": 3, "ws": 2, "gdiff": 1})

for _ext, _n in (((3, 3, 3), 1), ((3, 3, 3), 3), ((3, 9, 4), 1), ((4, 4, 7), 2), ((6, 5, 8), 1), ((8, 6, 3), 1),
                 ((9, 3, 5), 1), ((7, 8, 6), 1)):
    _why = "one axis odd, the others even" if _ext in ((4, 4, 7), (6, 5, 8), (8, 6, 3), (7, 8, 6)) else "edge extents"
    _row("l3_fwd", L3_FWD, "3-D extents %d x %d x %d (%s), levels = 1, N = %d" % (*_ext, _why, _n), _ext, B=_n, levels=1,
         target=(_ext[2] + _n) % 2 == 0)
    _row("l3_bwd", L3_BWD, "3-D backward extents %d x %d x %d (%s), levels = 1, N = %d" % (*_ext, _why, _n), _ext, B=_n,
         levels=1, gl=(1.0, -2.5)[_n % 2])
for _lv in (1, 2):
    _row("l3_fwd", L3_FWD, "3-D levels: 33 x 17 x 9 at levels = %d" % _lv, (33, 17, 9), levels=_lv, target=_lv == 2)
    _row("l3_bwd", L3_BWD, "3-D backward levels: 33 x 17 x 9 at levels = %d" % _lv, (33, 17, 9), levels=_lv,
         gl=(1.0, -2.5)[_lv % 2])
_row("l3_fwd", L3_FWD, "3-D levels: 65^3 at levels = 6", (65, 65, 65), levels=6)
_row("l3_bwd", L3_BWD, "3-D backward levels: 65^3 at levels = 6", (65, 65, 65), levels=6, gl=-2.5)
_row("l3_fwd", L3_FWD, "3-D target NULL", (7, 8, 6), B=2, levels=1, target=False)
_row("l3_fwd", L3_FWD, "3-D target given", (7, 8, 6), B=2, levels=1, target=True)
_row("l3_fwd", L3_FWD, "3-D partial-sum cap: N*D*H*W = 262144 (64^3): 1024 blocks, one trip", (64, 64, 64), levels=1,
     data="cb", margin=1e-3)
_row("l3_fwd", L3_FWD, "3-D partial-sum cap: N*D*H*W = 262145 (65 x 37 x 109): second trip of lap3_level_kernel",
     (65, 37, 109), levels=1, data="cb", margin=1e-3, spike=True)
_row("l3_fwd", L3_FWD, "3-D exact: input == target gives loss 0 and sgn 0", (5, 6, 7), B=2, levels=1, data="same")
_row("l3_fwd", L3_FWD, "fs_laploss3d_fwd, every operand misaligned", (5, 6, 7), B=2, levels=1,
     mis={"input": 3, "target": 1, "sgn": 2, "ws": 3, "loss": 1})
_row("l3_bwd", L3_BWD, "fs_laploss3d_bwd, every operand misaligned", (5, 6, 7), B=2, levels=1, gl=-2.5,
     mis={"sgn": 2, "gl": 1, "ws": 3, "gdiff": 2})

UNREACHABLE = {}  # every one of the 51 + 4 + 4 kernels is reached by a row at a test-sized tensor

HELPERS = {"fs::reduce_final_kernel"}  # common.hpp's reduction finish, compiled into every source that includes it


def kernels_of(r):
    return r["kernel"]


def row_id(r):
    short = lambda n: n.replace("warp2d_", "").replace("_kernel", "").replace(" ", "").replace("false", "f").replace(
        "true", "t")
    bits = [r["op"], "+".join(short(n) for n in r["kernel"]) if r["op"] in WARP_OPS else "",
            "B%dC%d" % (r["B"], r["C"]) if r["op"] in WARP_OPS else "B%d" % r["B"], "x".join(map(str, r["ext"]))]
    if r["inp"]:
        bits.append("i" + "x".join(map(str, r["inp"])))
    if r["op"] == "occ":
        bits.append("m%d" % r["mode"])
    if r["op"] in LAP_OPS:
        bits.append("L%d" % r["levels"])
        bits.append(r["data"] + ("" if r["target"] or r["op"].endswith("bwd") else "-nt") + ("-spike" if r["spike"] else "")
                    + ("-gl%g" % r["gl"] if r["op"].endswith("bwd") else ""))
    else:
        bits.append("".join(ch for ch, on in (("s", r["start"]), ("g", r["gin"]), ("n", not r["gflow"]), ("a", r["alias"]))
                            if on) + "-" + r["flow"])
    if r["mis"]:
        bits.append("m" + "".join("%s%d" % kv for kv in sorted(r["mis"].items())))
    return "-".join(b for b in bits if b)
