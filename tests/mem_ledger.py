"""Ledger of the memory-bound kernels' dispatch cases: one row per call of one C-ABI entry point of csrc/warp3d.hip (with
warp3d_rc.hpp) and csrc/interp.hip, with the compute kernel(s) the dispatch code (launch_fwd / launch_bwd,
fs_interp3d_bwd_scaled, fs_upsample3d_scale_add, downsample3d_impl, fs_resize2d_*) must pick for it.  Plain data, read by
tests/test_mem_ledger.py (every compiled kernel has a row, fs_warp3d_kernel_id agrees, the inputs keep the fp32 oracle
inside the band) and tests/test_gpu_mem_ledger.py (the named kernel runs and nothing else, every output matches an fp64
reference inside NaN-patterned guard bands).  tests/mem_ledger_inputs.py builds each row's inputs and reference.

Row fields:
  op       w_fwd w_bwd (fs_warp3d_*), wp_fwd wp_bwd wp_acc wp_acc3 (fs_warp3d_pair_*), uw_fwd uw_bwd uw_bwd3
           (fs_upsample_warp3d_pair_*), up_add (fs_upsample3d_scale_add), down down_ms (fs_downsample3d_fwd[_ms]),
           ibwd ibwd_s (fs_interp3d_bwd[_scaled]), r2_fwd r2_bwd (fs_resize2d_*)
  B, C
  ext      warps: extent (D, H, W) of the flow == of the output; the fused up-sampling forms (uw_*): extent (Ds, Hs, Ws)
           of delta, the flow's is factor x that.  resizes: extent of the forward's INPUT (2-D: (H, W))
  inp      warps: extent of the sampled volumes when it differs from the flow's (else None)
  factor, scale, upsample, with_ws, prev (up_add / uw_fwd: a running tensor is added)
  nadd     number of addends; add_strided[i]: addend i is channels 5..10 of an 11-channel tensor; gout_strided: the two
           upstream gradients are channels 2 and 3 of an 11-channel tensor; alias: add0 IS grad_flow6
  with_grad_in, with_grad_flow
  flow     the kinds the row's flow is built from (mem_ledger_inputs.FLOW_KINDS), one per pair member
  mis      {operand name: misalignment in floats, 0..3}
  stride_mis  the operand whose batch stride is not a multiple of 4 (add0 add1 add2 gout0 gout1 / src1), or None
  kernel   the expected compute kernel symbol; a tuple for the two-launch entry points
  plan     the FS_W3_KERNEL_* id fs_warp3d_kernel_id must give, None where the query cannot see the deciding operand
  why      the rung

Shapes are as small as the rung allows; the rows on the two sides of a threshold differ in one quantity.

What reading the dispatch code against its operands decided (the rows pin each of these):
  * launch_fwd does not inspect `in`, the fused form not `delta`, fs_upsample3d_scale_add not `small`, launch_bwd not
    grad_in: all four are only ever read or written with 4-byte accesses (8-byte pair loads at 4-byte alignment, scalar
    staging loops, float atomics), so the vector forms stay correct -- rows "... misaligned, not inspected".
  * downsample3d_impl's `(Hin * Win) % 4` cannot fail once `Win % 4 == 0` holds, so it has no far side.

Out of scope here (the next ledgers): census3d.hip, flowsmooth3d.hip and the metrics sources (metrics.hip, flowmetrics.hip,
series.hip).  losses.hip, wssim.hip, epilogue.hip and prelu.hip have theirs: tests/loss_ledger.py; corr2d.hip and corr3d.hip
(both over corr_q.hpp) theirs: tests/corr_ledger.py; warp2d.hip, laplacian.hip and laplacian3d.hip theirs:
tests/w2lap_ledger.py."""
from ledger_harness import normalize as _normalize

ROWS = []

RC_F = "warp3d_rc_kernel<false, 2, 6, 0>"
RC_B = "warp3d_rc_kernel<true, 4, 5, 0>"
RING_V = "warp3d_fwd_ring_kernel<true, 2, 4, 0>"
RING_S = "warp3d_fwd_ring_kernel<false, 0, 3, 0>"
UPS_V = "warp3d_fwd_kernel<512, true, true>"
UPS_S = "warp3d_fwd_kernel<512, false, true>"
BWD_V = "warp3d_bwd_kernel<256, true, false>"
BWD_VG = "warp3d_bwd_kernel<256, true, true>"
BWD_S = "warp3d_bwd_kernel<256, false, false>"
BWD_SG = "warp3d_bwd_kernel<256, false, true>"
ADJ_FUSED = "up_adjoint_fused_kernel<2, 4, 8>"
ADJ_SEP8 = "interp_axis_adjoint_kernel<8>"
UP_TILE2, UP_TILE4 = "upsample3d_scale_add_tile_kernel<2>", "upsample3d_scale_add_tile_kernel<4>"
UP_V4, UP_S = "upsample3d_scale_add_v4_kernel", "upsample3d_scale_add_kernel"
DOWN2, DOWN4 = "downsample3d_v4_kernel<2>", "downsample3d_v4_kernel<4>"
DADJ_V4, DADJ_S = "interp3d_down_adjoint_exact_v4<unsigned int>", "interp3d_down_adjoint_exact"

GATHER, RC = 0, 1  # FS_W3_KERNEL_*
WARP_OPS = ("w_fwd", "w_bwd", "wp_fwd", "wp_bwd", "wp_acc", "wp_acc3", "uw_fwd", "uw_bwd", "uw_bwd3")
RESIZE_OPS = ("up_add", "down", "down_ms", "ibwd", "ibwd_s", "r2_fwd", "r2_bwd")
PAIR_OPS = ("wp_fwd", "wp_bwd", "wp_acc", "wp_acc3", "uw_fwd", "uw_bwd", "uw_bwd3")
BWD_OPS = ("w_bwd", "wp_bwd", "wp_acc", "wp_acc3", "uw_bwd", "uw_bwd3")


def normalize(name):
    """ledger_harness.normalize, and no `rc::` (ops._KERNELS writes the row-cache kernels without their namespace)."""
    return _normalize(name).replace("rc::", "")


def _row(op, kernel, why, ext, plan=None, B=1, C=1, inp=None, factor=0, scale=1.0, upsample=0, with_ws=False, prev=False,
         nadd=0, add_strided=(False, False, False), gout_strided=False, alias=False, with_grad_in=False,
         with_grad_flow=True, flow=("smooth", "shift"), mis=None, stride_mis=None):
    ROWS.append(dict(op=op, B=B, C=C, ext=tuple(ext), inp=tuple(inp) if inp else None, factor=factor, scale=scale,
                     upsample=upsample, with_ws=with_ws, prev=prev, nadd=nadd, add_strided=tuple(add_strided),
                     gout_strided=gout_strided, alias=alias, with_grad_in=with_grad_in, with_grad_flow=with_grad_flow,
                     flow=tuple(flow), mis=dict(mis or {}), stride_mis=stride_mis, kernel=kernel, plan=plan, why=why))


E_RC = (37, 4, 72)   # the smallest volume that holds the row-cache window (NP = 37 planes, NX = 72 columns)
E_SM = (5, 8, 8)     # a small vector-friendly volume without the window
E_BIG = (40, 70, 76)  # strictly contains the window; Hi = 70 rows against R = 6 (forward) / 5 (backward) cached rows

# ---- forward warps: row cache against the ring kernel ---------------------------------------------------------------
_row("w_fwd", RC_F, "row cache: C = 1, W_in = 72, D_in = 37, aligned; pick_dc shrinks to 8", E_RC, RC, flow=("smooth",))
_row("w_fwd", RC_F, "row cache, smallest volume, white noise (the window is the whole volume: every voxel hits)", E_RC, RC,
     flow=("noise",))
_row("wp_fwd", RC_F, "row cache pair, smallest volume: jump and shift (all Hi = 4 rows stay resident)", E_RC, RC, B=2,
     flow=("jump", "shift"))
# a volume that strictly contains the window (x 72 of 76 columns, z 37 of 40 planes) with Hi = 70 rows >> R = 6 / 5 ring
# slots.  One slice of the flow's D = 40 is (Hi - 1) / (Di - 1) = 1.77 input rows, pick_dc gives 8-slice workgroups
# (5 x 2 x 3 tiles), so a smooth flow walks ~14 rows per workgroup.  Read against warp3d_rc.hpp's advance():
for _op, _k, _kw in (("w_fwd", RC_F, {}), ("w_bwd", RC_B, {}),
                     ("wp_acc3", RC_B, dict(nadd=3, add_strided=(False, True, False), gout_strided=True))):
    _pair = _op == "wp_acc3"
    for _kinds, _why in (
            (("smooth", "bigshift"), "smooth: rows advance 1.77 per slice, the ring slot wraps (s >= R) within 4 slices"
                                     "; shift 9.25 / -6.5 / 11.75: window origin 10 columns and 6 planes off the tile"),
            (("noise", "jump"), "white noise: y0 spreads over ~11 rows > R and x over > NX columns, voxels outside the "
                                "resident window take the global-gather fallback; jump of 7 = 12.4 rows at D / 2 inside "
                                "the chunk 16..23: the predicted rows miss (whole slice on the fallback), then lo_req > chi: "
                                "the discontinuity branch restarts the row ring"),
            (("ramp", "noise"), "ramp 2.5 per slice = 6.2 rows per slice > R: discontinuity every slice until the "
                                "coordinate clamps at Hi - 1 near d = 11, then a stationary window on the last rows")):
        for _kind in (_kinds,) if _pair else tuple((k,) for k in _kinds):
            if any(r["op"] == _op and r["ext"] == E_BIG and r["flow"] == _kind for r in ROWS):
                continue  # (white noise sits in two of the pairs)
            _row(_op, _k, "row cache on a volume that strictly holds the window (%s), %s" % (
                "acc3" if _pair else _op[2:], _why), E_BIG, RC, flow=_kind, **_kw)
_row("w_fwd", RING_V, "row cache: C = 2 -> ring", E_RC, GATHER, C=2, flow=("smooth",))
_row("w_fwd", RING_V, "row cache: W_in = 68 < 72 -> ring", (37, 4, 68), GATHER, flow=("smooth",))
_row("w_fwd", RING_V, "row cache: D_in = 36 < 37 -> ring", (36, 4, 72), GATHER, flow=("smooth",))
_row("w_fwd", RING_V, "row cache: W_in % 4 != 0 (W_in = 74, flow W = 72) -> ring", E_RC, GATHER, inp=(37, 4, 74),
     flow=("smooth",))
_row("w_fwd", RING_V, "row cache: in0 misaligned -> ring (rc::applicable inspects it)", E_RC, GATHER, flow=("smooth",),
     mis={"in0": 1})
_row("wp_fwd", RING_V, "row cache: in1 misaligned -> ring", E_RC, GATHER, mis={"in1": 2})
_row("wp_fwd", RC_F, "pick_dc stays at 64: 512 x 1 x 1 x 1 tiles x 2 members = 1024 workgroups", (64, 2, 4), RC, B=512,
     inp=(37, 2, 72), flow=("smooth", "noise"))
_row("wp_fwd", RC_F, "pick_dc: 511 tiles x 2 = 1022 < 1024 workgroups -> 32", (64, 2, 4), RC, B=511, inp=(37, 2, 72),
     flow=("smooth", "noise"))
_row("w_fwd", RC_F, "row cache: D = 6 smaller than the chosen dc = 8", (6, 4, 72), RC, inp=E_RC, flow=("smooth",))
_row("w_fwd", RING_S, "vec_ok: flow W = 70, W % 4 != 0 on a volume that holds the window -> scalar ring", (37, 4, 70),
     GATHER, inp=E_RC, flow=("smooth",))
_row("w_fwd", RING_S, "vec_ok fwd: flow misaligned on the window volume -> scalar ring", E_RC, GATHER, flow=("smooth",),
     mis={"flow": 1})
_row("w_fwd", RING_S, "vec_ok fwd: out0 misaligned on the window volume -> scalar ring; the query cannot see out", E_RC,
     None, flow=("smooth",), mis={"out0": 3})
_row("wp_fwd", RING_S, "vec_ok fwd: out1 misaligned -> scalar ring", E_SM, GATHER, mis={"out1": 1})
_row("wp_fwd", RING_V, "vec_ok fwd: in0 misaligned, not inspected (pair gathers are 4-byte aligned) -> vector ring", E_SM,
     GATHER, mis={"in0": 2})
# ---- ring forward geometry ------------------------------------------------------------------------------------------
_row("w_fwd", RING_V, "ring: D = 2 below the 4 ring stages", (2, 8, 8), GATHER, flow=("noise",))
_row("w_fwd", RING_V, "ring: D = 3 below the 4 ring stages", (3, 8, 8), GATHER, flow=("smooth",))
_row("w_fwd", RING_S, "scalar ring: D = 2 below the 3 ring stages", (2, 8, 6), GATHER, flow=("noise",))
_row("wp_fwd", RING_V, "ring: D = 17 not a multiple of 16 (second chunk of one slice)", (17, 8, 8), GATHER, C=2)
_row("w_fwd", RING_S, "scalar ring: D = 17 not a multiple of 16", (17, 8, 6), GATHER, flow=("jump",))
_row("w_fwd", RING_V, "ring: H = 64, W = 32 at a tile", (3, 64, 32), GATHER, flow=("smooth",))
_row("w_fwd", RING_V, "ring: H = 63 below a tile (W = 32)", (3, 63, 32), GATHER, flow=("smooth",))
_row("w_fwd", RING_V, "ring: H = 65 one above a tile (W = 32)", (3, 65, 32), GATHER, flow=("smooth",))
_row("w_fwd", RING_V, "ring: W = 28 below a tile (H = 64)", (3, 64, 28), GATHER, flow=("smooth",))
_row("w_fwd", RING_V, "ring: W = 36 one above a tile (H = 64)", (3, 64, 36), GATHER, flow=("smooth",))
_row("w_fwd", RING_S, "scalar ring: H = 65, W = 33 one above a tile", (3, 65, 33), GATHER, flow=("shift",))
_row("wp_fwd", RING_V, "ring: images larger than the flow", E_SM, GATHER, B=2, C=3, inp=(8, 9, 12))

# ---- backward warps -------------------------------------------------------------------------------------------------
_row("w_bwd", RC_B, "row cache backward: without grad_in", E_RC, RC, flow=("smooth",))
_row("w_bwd", RC_B, "row cache backward, smallest volume, white noise (every voxel hits the window)", E_RC, RC,
     flow=("noise",))
_row("w_bwd", BWD_VG, "row cache backward: with grad_in -> gather kernel", E_RC, GATHER, with_grad_in=True,
     flow=("smooth",))
_row("w_bwd", BWD_VG, "row cache backward: grad_flow null with grad_in set -> gather kernel", E_RC, GATHER,
     with_grad_in=True, with_grad_flow=False, flow=("smooth",))
_row("w_bwd", BWD_V, "row cache backward: C = 2 -> gather kernel", E_RC, GATHER, C=2, flow=("smooth",))
_row("w_bwd", BWD_V, "row cache backward: W_in = 68 < 72", (37, 4, 68), GATHER, flow=("smooth",))
_row("w_bwd", BWD_V, "row cache backward: D_in = 36 < 37", (36, 4, 72), GATHER, flow=("smooth",))
_row("w_bwd", BWD_V, "row cache backward: W_in % 4 != 0 (W_in = 74)", E_RC, GATHER, inp=(37, 4, 74), flow=("smooth",))
_row("w_bwd", BWD_V, "row cache backward: in0 misaligned -> gather kernel", E_RC, GATHER, flow=("smooth",), mis={"in0": 1})
_row("w_bwd", RC_B, "row cache backward: D = 6 smaller than the chosen dc", (6, 4, 72), RC, inp=E_RC, flow=("jump",))
_row("wp_bwd", RC_B, "row cache pair backward", E_RC, RC, B=2, flow=("jump", "ramp"))
_row("wp_bwd", RC_B, "pick_dc stays at 64, pair backward", (64, 2, 4), RC, B=512, inp=(37, 2, 72), flow=("smooth", "noise"))
_row("wp_bwd", BWD_VG, "pair backward with grad_img0 / grad_img1", E_SM, GATHER, B=2, C=2, with_grad_in=True)
_row("wp_bwd", BWD_S, "pair backward: W % 4 != 0", (5, 8, 6), GATHER, C=2)
_row("wp_bwd", BWD_SG, "pair backward: W % 4 != 0 with grad_in; H = 65 one above a tile", (3, 65, 33), GATHER,
     with_grad_in=True)
_row("wp_acc", RC_B, "acc: one dense addend, row cache", E_RC, RC, nadd=1)
_row("wp_acc", RC_B, "acc: add0 aliases grad_flow6, row cache", E_RC, RC, nadd=1, alias=True)
_row("wp_acc", BWD_V, "acc: null addend, gather kernel", E_SM, GATHER, C=2)
_row("wp_acc", BWD_VG, "acc: aliased addend with grad_in", E_SM, GATHER, nadd=1, alias=True, with_grad_in=True)
_row("wp_acc3", RC_B, "acc3: 0 addends, grad_out dense", E_RC, RC)
_row("wp_acc3", RC_B, "acc3: 1 strided addend", E_RC, RC, B=2, nadd=1, add_strided=(True, False, False))
_row("wp_acc3", RC_B, "acc3: 2 addends dense + strided, grad_out channels 2 and 3 of a wider tensor", E_RC, RC, B=2, nadd=2,
     add_strided=(False, True, False), gout_strided=True)
_row("wp_acc3", RC_B, "acc3: 3 addends, add0 aliases grad_flow6, strided grad_out", E_RC, RC, B=2, nadd=3,
     add_strided=(False, True, True), gout_strided=True, alias=True)
_row("wp_acc3", BWD_V, "acc3: 3 strided addends, gather kernel", E_SM, GATHER, B=2, nadd=3, add_strided=(True, True, True),
     gout_strided=True)
_row("wp_acc3", BWD_VG, "acc3: 3 addends with grad_in", E_SM, GATHER, B=2, C=1, nadd=3, add_strided=(False, True, False),
     with_grad_in=True)
# launch_bwd's vec_ok: each inspected operand misaligned on its own (window volume: the query still says row cache)
for _name in ("flow", "gflow", "gout0", "gout1", "add0", "add1", "add2"):
    _row("wp_acc3", BWD_S, "vec_ok bwd: %s misaligned -> scalar gather kernel%s" % (
        _name, "" if _name == "flow" else "; the query cannot see it"), E_RC, GATHER if _name == "flow" else None, B=2, nadd=3,
         mis={_name: 1 + len(_name) % 3})
_row("wp_bwd", BWD_V, "vec_ok bwd: in0 misaligned, not inspected (4-byte pair gathers) -> vector kernel", E_SM, GATHER,
     mis={"in0": 3})
_row("wp_bwd", BWD_VG, "vec_ok bwd: grad_in misaligned, not inspected (float atomics) -> vector kernel", E_SM, GATHER,
     with_grad_in=True, mis={"gin0": 1, "gin1": 2})
# the five stride conditions
for _name in ("add0", "add1", "add2", "gout0", "gout1"):
    _row("wp_acc3", BWD_S, "strides: batch stride of %s %% 4 != 0 -> scalar gather kernel; the query cannot see it" % _name,
         E_RC, None, B=2, nadd=3, add_strided=(True, True, True), gout_strided=True, stride_mis=_name)

# ---- fused up-sampling + warp ---------------------------------------------------------------------------------------
_row("uw_fwd", UPS_V, "upsample-warp x2 without prev_flow", (3, 4, 4), B=2, factor=2, scale=2.0)
_row("uw_fwd", UPS_V, "upsample-warp x2 with prev_flow, images larger than the flow", (3, 4, 4), C=2, inp=(7, 9, 12),
     factor=2, scale=2.0, prev=True)
_row("uw_fwd", UPS_V, "upsample-warp x4 with prev_flow", (2, 2, 2), factor=4, scale=4.0, prev=True)
_row("uw_fwd", UPS_V, "upsample-warp x4 without prev_flow, D = 20 > 16 slices per workgroup, H = 68 above a tile", (5, 17, 9),
     factor=4, scale=4.0)
_row("uw_fwd", UPS_V, "upsample-warp x2, D = 10 > 8 slices per workgroup, W = 36 above a tile", (5, 4, 18), factor=2,
     scale=2.0, prev=True)
_row("uw_fwd", UPS_S, "upsample-warp: W = 6, W % 4 != 0", (3, 4, 3), factor=2, scale=2.0, prev=True)
for _name in ("prev", "fout", "out0", "out1"):
    _row("uw_fwd", UPS_S, "vec_ok upsample-warp: %s misaligned -> scalar form" % _name, (3, 4, 4), factor=2, scale=2.0,
         prev=True, mis={_name: 1 + len(_name) % 3})
_row("uw_fwd", UPS_V, "vec_ok upsample-warp: delta misaligned, not inspected (scalar staging loop) -> vector form",
     (3, 4, 4), factor=2, scale=2.0, prev=True, mis={"delta": 1})
_row("uw_fwd", UPS_V, "vec_ok upsample-warp: in0 misaligned, not inspected -> vector form", (3, 4, 4), factor=2, scale=2.0,
     mis={"in0": 2})
_row("uw_bwd", (BWD_V, ADJ_FUSED), "upsample-warp backward x2: gather kernel + fused adjoint", (3, 4, 4), B=2, factor=2,
     scale=2.0, nadd=1)
_row("uw_bwd", (BWD_V, ADJ_FUSED), "upsample-warp backward x2: aliased addend", (3, 4, 4), factor=2, scale=2.0, nadd=1,
     alias=True)
_row("uw_bwd", (BWD_V, ADJ_SEP8), "upsample-warp backward x4: gather kernel + separable adjoint (workspace used)",
     (2, 2, 2), factor=4, scale=4.0)
_row("uw_bwd", (RC_B, ADJ_SEP8), "upsample-warp backward x4 on a window volume: row cache + separable adjoint", (10, 1, 18),
     factor=4, scale=4.0, nadd=1)
_row("uw_bwd3", (RC_B, ADJ_FUSED), "upsample-warp backward3 x2 on a window volume: 3 addends, strided grad_out",
     (19, 2, 36), B=2, factor=2, scale=2.0, nadd=3, add_strided=(True, False, True), gout_strided=True)
_row("uw_bwd3", (BWD_S, ADJ_FUSED), "upsample-warp backward3 x2: W % 4 != 0", (3, 4, 3), factor=2, scale=2.0, nadd=2)
_row("uw_bwd3", (BWD_V, ADJ_SEP8), "upsample-warp backward3 x4: add0 aliases grad_flow_total", (2, 2, 2), B=2, factor=4,
     scale=4.0, nadd=2, alias=True)

# ---- fs_upsample3d_scale_add: tile against v4 against scalar ------------------------------------------------------------
_row("up_add", UP_TILE2, "upsample tile x2: Do = 8, Ho = 8, Wo = 64", (4, 4, 32), B=2, C=3, factor=2, scale=2.0, prev=True)
_row("up_add", UP_TILE2, "upsample tile x2 without prev, two tiles per axis", (8, 8, 64), factor=2, scale=1.0)
_row("up_add", UP_TILE4, "upsample tile x4: Do = 8, Ho = 8, Wo = 64", (2, 2, 16), C=6, factor=4, scale=4.0, prev=True)
_row("up_add", UP_V4, "upsample: Wo = 60, Wo % 64 != 0 -> v4", (4, 4, 30), B=2, C=3, factor=2, scale=2.0, prev=True)
_row("up_add", UP_V4, "upsample: Do = 12, Do % 8 != 0 -> v4", (6, 4, 32), B=2, C=3, factor=2, scale=2.0, prev=True)
_row("up_add", UP_V4, "upsample: Ho = 12, Ho % 8 != 0 -> v4", (4, 6, 32), B=2, C=3, factor=2, scale=2.0, prev=True)
_row("up_add", UP_V4, "upsample x4: Ho = 12 -> v4", (2, 3, 16), C=2, factor=4, scale=4.0)
_row("up_add", UP_S, "upsample: out misaligned -> scalar", (4, 4, 32), B=2, C=3, factor=2, scale=2.0, prev=True,
     mis={"out": 1})
_row("up_add", UP_S, "upsample: prev misaligned -> scalar", (4, 4, 32), B=2, C=3, factor=2, scale=2.0, prev=True,
     mis={"prev": 2})
_row("up_add", UP_S, "upsample: Wo = 62, Wo % 4 != 0 -> scalar", (4, 4, 31), B=2, C=3, factor=2, scale=2.0, prev=True)
_row("up_add", UP_TILE2, "upsample: small misaligned, not inspected (scalar staging loop) -> tile", (4, 4, 32), B=2, C=3,
     factor=2, scale=2.0, prev=True, mis={"small": 3})
_row("up_add", UP_V4, "upsample v4: small misaligned, not inspected (scalar corner loads)", (4, 4, 30), C=2, factor=2,
     scale=2.0, mis={"small": 1})

# ---- fs_downsample3d_fwd[_ms]: v4 against the two fall-backs ----------------------------------------------------------
_row("down", DOWN2, "downsample v4 /2: Win % 4 == 0, (Hin * Win) % 4 == 0, Wo % 4 == 0", (4, 6, 16), B=2, C=3, factor=2,
     scale=0.5)
_row("down", DOWN2, "downsample v4 /2: floor extents in D and H", (5, 7, 16), C=2, factor=2, scale=0.5)
_row("down", DOWN4, "downsample v4 /4", (8, 4, 16), B=2, C=2, factor=4, scale=0.25)
_row("down", DOWN4, "downsample v4 /4: floor extents in D and H", (9, 6, 16), factor=4, scale=1.0)
_row("down", UP_V4, "downsample: in misaligned -> generic v4 fall-back", (4, 6, 16), B=2, C=3, factor=2, scale=0.5,
     mis={"in": 1})
_row("down", UP_V4, "downsample: Win = 9, Win % 4 != 0 with Wo = 4 -> generic v4 fall-back", (4, 6, 9), C=2, factor=2,
     scale=0.5)
_row("down", UP_S, "downsample: Wo = 6, Wo % 4 != 0 -> scalar fall-back", (4, 6, 12), B=2, C=3, factor=2, scale=0.5)
_row("down", UP_S, "downsample: out misaligned -> scalar fall-back", (4, 6, 16), B=2, C=3, factor=2, scale=0.5,
     mis={"out": 2})
_row("down_ms", DOWN2, "downsample multi-source /2: planes with a spare channel", (4, 6, 16), B=2, C=3, factor=2, scale=0.5)
_row("down_ms", DOWN4, "downsample multi-source /4", (8, 4, 16), B=2, C=5, factor=4, scale=0.25)
_row("down_ms", UP_V4, "downsample multi-source stride with % 4 != 0 -> generic v4 with a null `in`", (4, 6, 16), B=2, C=3,
     factor=2, scale=0.5, stride_mis="src1")
_row("down_ms", UP_V4, "downsample multi-source: src1 misaligned -> generic v4 with a null `in`", (4, 6, 16), B=2, C=3,
     factor=2, scale=0.5, mis={"src1": 1})
_row("down_ms", UP_S, "downsample multi-source: Wo % 4 != 0 -> scalar with a null `in`", (4, 6, 12), B=2, C=3, factor=2,
     scale=0.5)

# ---- adjoint ladder (ext = the forward's input = grad_in) ----------------------------------------------------------------
_row("ibwd", DADJ_V4, "adjoint ladder: down exact v4<unsigned>", (4, 6, 16), B=2, C=3, factor=2)
_row("ibwd_s", DADJ_V4, "adjoint ladder: down exact v4<unsigned> /4 with scale = 1/4", (8, 4, 16), C=2, factor=4, scale=0.25)
_row("ibwd", DADJ_S, "adjoint ladder: down exact scalar (Win = 6, Win % 4 != 0)", (4, 6, 6), B=2, C=3, factor=2)
_row("ibwd", DADJ_S, "adjoint ladder: down exact scalar (grad_in misaligned)", (4, 6, 16), B=2, C=3, factor=2,
     mis={"gin": 1})
_row("ibwd", DADJ_V4, "adjoint ladder: down exact v4, grad_out misaligned, not inspected (scalar loads)", (4, 6, 16), C=2,
     factor=2, mis={"gout": 1})
_row("ibwd", "interp3d_adjoint_kernel<3>", "adjoint ladder: down floor extents /2 -> adjoint<3>", (5, 7, 9), B=2, C=2,
     factor=2)
_row("ibwd", "interp3d_adjoint_kernel<3>", "adjoint ladder: down floor extents /4 -> adjoint<3>", (9, 6, 17), C=2, factor=4)
_row("ibwd_s", ADJ_FUSED, "adjoint ladder: up x2 with workspace -> fused, scale = 2", (3, 5, 7), B=2, C=3, factor=2,
     scale=2.0, upsample=1, with_ws=True)
_row("ibwd", ADJ_FUSED, "adjoint ladder: up x2 with workspace -> fused, more than one tile per axis", (5, 9, 33), C=2,
     factor=2, upsample=1, with_ws=True)
_row("ibwd_s", ADJ_SEP8, "adjoint ladder: up x4 with workspace -> separable x4, scale = 4", (3, 2, 5), B=2, C=3, factor=4,
     scale=4.0, upsample=1, with_ws=True)
_row("ibwd", "interp3d_adjoint_kernel<4>", "adjoint ladder: up x2 without workspace -> adjoint<4>", (3, 5, 7), B=2, C=3,
     factor=2, upsample=1)
_row("ibwd", "interp3d_adjoint_kernel<8>", "adjoint ladder: up x4 without workspace -> adjoint<8>", (3, 2, 5), B=2, C=3,
     factor=4, upsample=1)

# ---- 2-D bilinear pair (ext = (Hin, Win)) ------------------------------------------------------------------------------
_row("r2_fwd", "resize2d_kernel", "resize2d forward up x2", (5, 7), B=2, C=3, factor=2, upsample=1, scale=2.0)
_row("r2_fwd", "resize2d_kernel", "resize2d forward up x4", (3, 5), C=2, factor=4, upsample=1, scale=4.0)
_row("r2_fwd", "resize2d_kernel", "resize2d forward down /2, floor extents", (9, 13), B=2, C=3, factor=2, scale=0.5)
_row("r2_fwd", "resize2d_kernel", "resize2d forward down /4", (8, 16), C=2, factor=4, scale=0.25)
_row("r2_bwd", "resize2d_adjoint_kernel<3>", "resize2d backward down /2, floor extents", (9, 13), B=2, C=3, factor=2,
     scale=0.5)
_row("r2_bwd", "resize2d_adjoint_kernel<3>", "resize2d backward down /4", (8, 16), C=2, factor=4, scale=0.25)
_row("r2_bwd", "resize2d_adjoint_kernel<4>", "resize2d backward up x2", (5, 7), B=2, C=3, factor=2, upsample=1, scale=2.0)
_row("r2_bwd", "resize2d_adjoint_kernel<8>", "resize2d backward up x4", (3, 5), C=2, factor=4, upsample=1, scale=4.0)

# Compute kernels of the product build that no call of the product library can reach at a test-sized tensor.
UNREACHABLE_IN_PRODUCT = {
    "interp3d_down_adjoint_exact_v4<long long>": "needs more than 2^32 - 2^28 float4 groups of grad_in (a 60 GB tensor)",
    "interp_axis_adjoint_kernel<4>": "the fused x2 adjoint comes first; the separable x2 form needs 2^31 fused tiles or "
                                     "the ablation build's FLOWSCI_INTERP_SEPARABLE (FS_AB_ENV is constant false in the "
                                     "product build)",
}
# (warp3d_fwd_kernel has no non-up-sampling form: its branches were deleted from the source, nothing to list)

HELPERS = {"fs::reduce_final_kernel"}  # common.hpp's reduction finish, compiled into every source that includes it


def kernels_of(r):
    return r["kernel"] if isinstance(r["kernel"], tuple) else (r["kernel"],)


def row_id(r):
    k = "+".join(n.split("<")[0].replace("_kernel", "") + "".join(c for c in n[n.find("<"):] if c.isalnum())[:14]
                 if "<" in n else n.replace("_kernel", "") for n in kernels_of(r))
    bits = [r["op"], k, "B%dC%d" % (r["B"], r["C"]), "x".join(map(str, r["ext"]))]
    if r["inp"]:
        bits.append("i" + "x".join(map(str, r["inp"])))
    if r["factor"]:
        bits.append("%s%d" % ("u" if r["upsample"] or r["op"] in ("up_add", "uw_fwd", "uw_bwd", "uw_bwd3") else "d",
                              r["factor"]))
    flags = "".join(ch for ch, on in (("p", r["prev"]), ("w", r["with_ws"]), ("g", r["with_grad_in"]),
                                      ("n", not r["with_grad_flow"]), ("a", r["alias"]), ("s", r["gout_strided"])) if on)
    if r["nadd"]:
        flags += "A%d%s" % (r["nadd"], "".join("s" if s else "d" for s in r["add_strided"][:r["nadd"]]))
    if r["op"] in WARP_OPS:
        flags += "-" + ".".join(r["flow"])
    bits.append(flags)
    if r["mis"]:
        bits.append("m" + "".join("%s%d" % kv for kv in sorted(r["mis"].items())))
    if r["stride_mis"]:
        bits.append("st-" + r["stride_mis"])
    return "-".join(b for b in bits if b)
