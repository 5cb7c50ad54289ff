"""Ledger of the loss, epilogue and PReLU kernels: one row per raw call of one C-ABI entry point of csrc/losses.hip
(fs_robust_sum[_bwd], fs_census_dist_{fwd,bwd}), csrc/wssim.hip (fs_wssim_{fwd,bwd}), csrc/epilogue.hip (fs_merge_*,
fs_distill_*, fs_distill3_*) and csrc/prelu.hip (fs_prelu_bwd), with the compute kernel(s) the call must launch.  Plain
data, read by tests/test_loss_ledger.py (every compiled kernel has a row, the inputs keep the fp32 oracle inside the band and
every discontinuity decision equal in fp32 and fp64) and tests/test_gpu_loss_ledger.py (the named kernel runs and no other,
every output matches an fp64 reference inside NaN-patterned guard bands).  tests/loss_ledger_inputs.py builds each row's
inputs, reference and exact expectations.

None of these entry points dispatches on shape or alignment (one kernel each, fs_prelu_bwd two; fs_robust_sum* one per
penalty): what the rows walk are the rungs INSIDE the kernels -- the second trip of the grid-stride loops, the register /
re-read branches of the distillation backward, the chunk ladder and the vector / scalar blocks of the PReLU backward,
tile edges of the census and SSIM kernels, every nullable operand -- with a row on each side of every threshold.

Row fields:
  op       rs_fwd rs_bwd (fs_robust_sum[_bwd]), cen_fwd cen_bwd (fs_census_dist_*), ws_fwd ws_bwd (fs_wssim_*), mg_fwd mg_bwd
           (fs_merge_*), ds_fwd ds_bwd (fs_distill_*), d3_fwd d3_bwd (fs_distill3_*), prelu (fs_prelu_bwd)
  kernel   tuple of the compute kernel symbols the call must launch (fs_prelu_bwd: two)
  B, C, S  batch, channels, spatial size per channel (rs with a border, cen, ws: S = H * W); F: flow channels (distill)
  mode, q, eps, border, with_y, wkind   fs_robust_sum*: penalty, exponent, Charbonnier eps, border, y given, the weight
           (None: NULL; "01": a 0 / 1 mask, sums[1] is then exact; "float": uniform weights)
  use_occ, ykind   fs_wssim_*: the flag; y is independent noise ("noise") or x plus a perturbation ("near")
  grads    the nullable outputs that are asked for (rs_bwd / ws_bwd: gx gy; cen_bwd: g1 g2; mg_bwd: gw0 gw1 gm)
  sig, gsig  fs_merge_fwd: sigmoid_out given; fs_merge_bwd: grad_sigmoid given
  coef0    distill backward: coef == 0 and non-finite student flows (the gradient is exactly 0)
  nw, bias fs_prelu_bwd: num_weights, grad_bias given
  mis      {operand name: misalignment in floats, 0..3}
  why      the rung

Shapes are as small as the rung allows; the rows on the two sides of a threshold differ in one quantity."""

ROWS = []
HELPERS = {"fs::reduce_final_kernel"}  # common.hpp's reduction finish, compiled into every source that includes it
UNREACHABLE = {}  # every kernel of the four sources is reached by a row

FS_REDUCE_BLOCKS, FS_PRELU_MAX_CHUNKS = 1024, 64
FWD_CAP = FS_REDUCE_BLOCKS * 256   # 262 144: one more element starts the second trip of the forward reductions
BWD_CAP = 16384 * 256              # 4 194 304: the same for robust_sum_bwd, merge_{fwd,bwd}, distill*_bwd
ABS_ROBUST, CHARBONNIER, L1_EPS, L1 = 0, 1, 2, 3  # FS_PEN_*
PEN = ("abs_robust", "charbonnier", "l1_eps", "l1")

OPS = ("rs_fwd", "rs_bwd", "cen_fwd", "cen_bwd", "ws_fwd", "ws_bwd", "mg_fwd", "mg_bwd", "ds_fwd", "ds_bwd", "d3_fwd",
       "d3_bwd", "prelu")
DEFAULTS = dict(B=1, C=1, S=0, H=0, W=0, F=0, mode=0, q=0.4, eps=1e-6, border=0, with_y=True, wkind=None, use_occ=0,
                ykind="noise", grads=(), sig=False, gsig=False, coef0=False, nw=0, bias=False, mis={})
_ID_ORDER = ("B", "C", "S", "H", "W", "F", "mode", "q", "eps", "border", "with_y", "wkind", "use_occ", "ykind", "grads", "sig",
             "gsig", "coef0", "nw", "bias")


def make(op, kernel, why, **kw):
    assert op in OPS and set(kw) <= set(DEFAULTS), (op, kw)
    r = dict(DEFAULTS, **kw)
    r.update(op=op, kernel=kernel if isinstance(kernel, tuple) else (kernel,), why=why, mis=dict(kw.get("mis", {})),
             grads=tuple(kw.get("grads", ())))
    if r["H"] and not r["S"]:
        r["S"] = r["H"] * r["W"]
    return r


def _row(op, kernel, why, **kw):
    ROWS.append(make(op, kernel, why, **kw))


def kernels_of(r):
    return r["kernel"]


def row_id(r):
    bits = [r["op"]]
    for k in _ID_ORDER:
        v = r[k]
        if v == DEFAULTS[k]:
            continue
        if isinstance(v, bool):
            bits.append(k if v else "no" + k)
        elif isinstance(v, tuple):
            bits.append("+".join(v))
        elif isinstance(v, str):
            bits.append(v)
        else:
            bits.append("%s%d" % (k, v) if isinstance(v, int) else "%s%g" % (k, v))
    if r["mis"]:
        bits.append("m" + "".join("%s%d" % kv for kv in sorted(r["mis"].items())))
    return "-".join(bits)


# ---- fs_robust_sum / fs_robust_sum_bwd ----------------------------------------------------------------------------------
RS_F = lambda mode: "robust_sum_kernel<%d>" % mode
RS_B = lambda mode: "robust_sum_bwd_kernel<%d>" % mode
_BC = ((1, 1), (2, 3), (3, 2), (1, 3), (3, 1), (2, 2), (2, 1), (1, 2))

_i = 0
for _mode in (ABS_ROBUST, CHARBONNIER, L1_EPS, L1):
    for _with_y in (False, True):
        for _wkind in (None, "01" if _mode in (ABS_ROBUST, CHARBONNIER) or _with_y else "float"):
            _B, _C = _BC[_i % len(_BC)]
            _kw = dict(B=_B, C=_C, S=(257, 1031, 77, 515)[_i % 4], mode=_mode, with_y=_with_y, wkind=_wkind,
                       q=(0.4, 1.0)[_i % 2], eps=(1e-6, 1e-8)[(_i // 2) % 2])
            _what = "%s, y %s, w %s, q = %g, eps = %g, S odd" % (PEN[_mode], "given" if _with_y else "NULL",
                                                                 _wkind or "NULL", _kw["q"], _kw["eps"])
            _row("rs_fwd", RS_F(_mode), "penalty fwd: " + _what, **_kw)
            _row("rs_bwd", RS_B(_mode), "penalty bwd: " + _what, grads=(("gx", "gy") if _with_y else ("gx",)), **_kw)
            _i += 1
# both exponents and both eps for the two penalties that read them (the loop above alternates them)
for _mode in (ABS_ROBUST, CHARBONNIER):
    for _q, _eps in ((0.4, 1e-8), (1.0, 1e-6), (1.0, 1e-8), (0.4, 1e-6)):
        _kw = dict(B=2, C=2, S=129, mode=_mode, q=_q, eps=_eps, wkind="float")
        _row("rs_fwd", RS_F(_mode), "penalty fwd: %s with q = %g and eps = %g, uniform weights" % (PEN[_mode], _q, _eps), **_kw)
        _row("rs_bwd", RS_B(_mode), "penalty bwd: %s with q = %g and eps = %g, uniform weights" % (PEN[_mode], _q, _eps),
             grads=("gx", "gy"), **_kw)
for _H, _W, _why in ((7, 9, "border = 3 on 7x9: one inner row"),
                     (6, 9, "border = 3 on 6x9: H <= 2 * border, all weights zero, sums == (0, 0), gradient exactly 0"),
                     (20, 31, "border = 3 on 20x31")):
    for _mode, _wkind in ((ABS_ROBUST, "01"), (CHARBONNIER, "float")):
        _kw = dict(B=2, C=3, H=_H, W=_W, border=3, mode=_mode, wkind=_wkind)
        _row("rs_fwd", RS_F(_mode), "%s, fwd, B = 2, C = 3, w %s" % (_why, _wkind), **_kw)
        _row("rs_bwd", RS_B(_mode), "%s, bwd, B = 2, C = 3, w %s" % (_why, _wkind), grads=("gx", "gy"), **_kw)
_row("rs_fwd", RS_F(CHARBONNIER), "border = 0 on 7x9: H and W given but not used", B=2, C=3, H=7, W=9, mode=CHARBONNIER,
     wkind="01")
for _mode in (ABS_ROBUST, L1):
    _row("rs_fwd", RS_F(_mode), "robust_sum fwd: n = 262144, every thread of the 1024 blocks takes one element", S=FWD_CAP,
         mode=_mode, wkind="01")
    _row("rs_fwd", RS_F(_mode), "robust_sum fwd: n = 262145, second trip of the grid-stride loop", S=FWD_CAP + 1, mode=_mode,
         wkind="01")
_row("rs_fwd", RS_F(CHARBONNIER), "robust_sum fwd: n = 262145 = 1 x 5 x 52429, second trip with C > 1 (weight index)", C=5,
     S=52429, mode=CHARBONNIER, wkind="01")
_row("rs_bwd", RS_B(ABS_ROBUST), "robust_sum bwd: n = 4194304 at the 16384-block cap, both gradients", S=BWD_CAP,
     grads=("gx", "gy"), wkind="01")
for _mode, _grads in ((ABS_ROBUST, ("gx", "gy")), (CHARBONNIER, ("gx",)), (L1_EPS, ("gy",))):
    _row("rs_bwd", RS_B(_mode), "robust_sum bwd: n = 4194305, second trip, %s" % " and ".join(_grads), S=BWD_CAP + 1,
         mode=_mode, grads=_grads, wkind="01" if _mode == ABS_ROBUST else None)
for _mode in (ABS_ROBUST, CHARBONNIER, L1_EPS, L1):
    _kw = dict(B=2, C=2, S=131, mode=_mode, wkind="01")
    _row("rs_fwd", RS_F(_mode), "robust_sum fwd %s: every operand misaligned (scalar kernel, same result)" % PEN[_mode],
         mis=dict(x=1, y=2, w=3, sums=1, ws=3), **_kw)
    _row("rs_bwd", RS_B(_mode), "robust_sum bwd %s: every operand misaligned (scalar kernel, same result)" % PEN[_mode],
         grads=("gx", "gy"), mis=dict(x=3, y=1, w=2, coef=1, gx=2, gy=3), **_kw)

# ---- fs_census_dist_{fwd,bwd}: the 16x16 tile with its 3-pixel halo ------------------------------------------------------
CEN_F, CEN_B = "census_dist_kernel<3>", "census_dist_bwd_kernel<3>"
_CEN = ((1, 1, "1x1: smaller than the 7x7 patch, every neighbour is padding"),
        (3, 5, "3x5: smaller than the 7x7 patch"),
        (7, 7, "7x7: one patch"),
        (15, 16, "15x16: H one below the 16-pixel tile, W at it"),
        (16, 17, "16x17: H at the tile, W one above (a second tile column of one pixel)"),
        (17, 33, "17x33: H one above the tile, three tile columns"))
for _n, (_H, _W, _why) in enumerate(_CEN):
    for _B in (1, 3):
        _row("cen_fwd", CEN_F, "census fwd %s, B = %d" % (_why, _B), B=_B, H=_H, W=_W)
    for _k, _grads in enumerate((("g1",), ("g2",), ("g1", "g2"))):
        _B = (1, 3)[(_n + _k) % 2]
        _row("cen_bwd", CEN_B, "census bwd %s, B = %d, %s" % (_why, _B, " and ".join(_grads)), B=_B, H=_H, W=_W, grads=_grads)
_row("cen_fwd", CEN_F, "census fwd: every operand misaligned (4-byte accesses only)", B=2, H=17, W=18,
     mis=dict(img1=1, img2=2, dist=3))
_row("cen_bwd", CEN_B, "census bwd: every operand misaligned (4-byte accesses only)", B=2, H=17, W=18, grads=("g1", "g2"),
     mis=dict(img1=3, img2=1, gdist=2, g1=1, g2=2))

# ---- fs_wssim_{fwd,bwd}: 3x3 windows, the 16x16 tile of the backward -----------------------------------------------------
WS_F, WS_B = "wssim_fwd_kernel", "wssim_bwd_kernel"
_WS = ((3, 3, "3x3: one window"),
       (3, 20, "3x20: one row of windows, two tile columns"),
       (16, 16, "16x16: at the 16-pixel tile of the backward"),
       (17, 18, "17x18: one above the tile in H, W - 2 = 16 windows"),
       (18, 19, "18x19: H - 2 = 16 windows, W one above"),
       (19, 37, "19x37: three tile columns"))
for _n, (_H, _W, _why) in enumerate(_WS):
    for _k, (_B, _C) in enumerate(((1, 1), (2, 3))):
        _occ, _yk = (_n + _k) % 2, ("noise", "near")[(_n // 2 + _k) % 2]
        _row("ws_fwd", WS_F, "wssim fwd %s, B x C = %dx%d, use_occ = %d, y %s" % (_why, _B, _C, _occ, _yk), B=_B, C=_C, H=_H,
             W=_W, use_occ=_occ, ykind=_yk)
        _row("ws_fwd", WS_F, "wssim fwd %s, B x C = %dx%d, use_occ = %d, y %s" % (_why, _B, _C, 1 - _occ, _yk), B=_B, C=_C,
             H=_H, W=_W, use_occ=1 - _occ, ykind=_yk)
        for _j, _grads in enumerate((("gx",), ("gy",), ("gx", "gy"))):
            _o = (_occ + _j) % 2
            _row("ws_bwd", WS_B, "wssim bwd %s, B x C = %dx%d, use_occ = %d, y %s, %s" % (
                _why, _B, _C, _o, _yk, " and ".join(_grads)), B=_B, C=_C, H=_H, W=_W, use_occ=_o, ykind=_yk, grads=_grads)
_row("ws_bwd", WS_B, "wssim bwd 19x37, B x C = 2x3, use_occ = 1, both gradients (the other flag of that row)", B=2, C=3, H=19,
     W=37, use_occ=1, ykind="near", grads=("gx", "gy"))
_row("ws_fwd", WS_F, "wssim fwd: 262144 windows (3 x 262146), every thread of the 1024 blocks takes one", H=3, W=FWD_CAP + 2,
     use_occ=1)
_row("ws_fwd", WS_F, "wssim fwd: 262145 windows (3 x 262147), second trip of the grid-stride loop", H=3, W=FWD_CAP + 3,
     use_occ=1)
_row("ws_fwd", WS_F, "wssim fwd: 261942 windows (1 x 3 x 295 x 300), just under the cap", C=3, H=295, W=300, use_occ=1,
     ykind="near")
_row("ws_fwd", WS_F, "wssim fwd: 266412 windows (1 x 3 x 300 x 300), second trip with C > 1", C=3, H=300, W=300, use_occ=1,
     ykind="near")
_row("ws_fwd", WS_F, "wssim fwd: every operand misaligned (4-byte accesses only)", B=2, C=3, H=17, W=18, use_occ=1,
     mis=dict(x=1, y=2, w=3, sums=2, ws=1))
_row("ws_bwd", WS_B, "wssim bwd: every operand misaligned (4-byte accesses only)", B=2, C=3, H=17, W=18, use_occ=1,
     grads=("gx", "gy"), mis=dict(x=2, y=3, w=1, coef=3, gx=1, gy=2))

# ---- fs_merge_{fwd,bwd} ---------------------------------------------------------------------------------------------------
MG_F, MG_B = "merge_fwd_kernel", "merge_bwd_kernel"
for _C in (1, 3):
    for _sig in (False, True):
        _row("mg_fwd", MG_F, "merge fwd: C = %d, sigmoid_out %s; logits 0, +-20, +-88, +-100" % (
            _C, "given" if _sig else "NULL"), B=2, C=_C, S=1031, sig=_sig)
_n = 0
for _grads in (("gw0",), ("gw1",), ("gm",), ("gw0", "gw1"), ("gw0", "gm"), ("gw1", "gm"), ("gw0", "gw1", "gm")):
    for _gsig in (False, True):
        _C = (1, 3)[(_n // 2 + _gsig) % 2]
        _row("mg_bwd", MG_B, "merge bwd: %s asked for, grad_sigmoid %s, C = %d; logits 0, +-20, +-88, +-100" % (
            " ".join(_grads), "given" if _gsig else "NULL", _C), B=2, C=_C, S=1031, grads=_grads, gsig=_gsig)
        _n += 1
_row("mg_fwd", MG_F, "merge fwd: n = 4194304 at the 16384-block cap", S=BWD_CAP, sig=True)
_row("mg_fwd", MG_F, "merge fwd: n = 4194305, second trip of the grid-stride loop", S=BWD_CAP + 1, sig=True)
_row("mg_fwd", MG_F, "merge fwd: n = 4194305 = 1 x 5 x 838861, second trip with C > 1 (sigmoid_out written once per voxel)",
     C=5, S=838861, sig=True)
_row("mg_bwd", MG_B, "merge bwd: B * S = 4194304 at the 16384-block cap, C = 1", S=BWD_CAP, grads=("gw0", "gw1", "gm"),
     gsig=True)
_row("mg_bwd", MG_B, "merge bwd: B * S = 4194305, second trip, C = 1", S=BWD_CAP + 1, grads=("gw0", "gw1", "gm"), gsig=True)
_row("mg_fwd", MG_F, "merge fwd: every operand misaligned (scalar kernel)", B=2, C=3, S=131, sig=True,
     mis=dict(w0=1, w1=2, m=3, merged=1, sig=2))
_row("mg_bwd", MG_B, "merge bwd: every operand misaligned (scalar kernel)", B=2, C=3, S=131, grads=("gw0", "gw1", "gm"),
     gsig=True, mis=dict(w0=3, w1=1, m=2, gmerged=1, gsig=3, gw0=2, gw1=3, gm=1))

# ---- fs_distill_{fwd,bwd}, fs_distill3_{fwd,bwd} --------------------------------------------------------------------------
# (every row holds a block of voxels where the student flow equals the teacher's: root == 0; distill3 one block per
# student, at three different places, and three different students)
DS_F, DS_B, D3_F, D3_B = "distill_fwd_kernel", "distill_bwd_kernel", "distill3_fwd_kernel", "distill3_bwd_kernel"
for _F in (1, 4, 6, 7, 8):
    for _C in (1, 3):
        _rung = ("F = %d <= MAXF = 6: the differences stay in registers" if _F <= 6 else
                 "F = %d > MAXF = 6: the second pass reads the flows again") % _F
        _row("ds_fwd", DS_F, "distill fwd: F = %d, C = %d, root == 0 block" % (_F, _C), B=2, C=_C, F=_F, S=1031)
        _row("ds_bwd", DS_B, "distill bwd: %s, C = %d, root == 0 block" % (_rung, _C), B=2, C=_C, F=_F, S=1031)
        _row("d3_fwd", D3_F, "distill3 fwd: F = %d, C = %d, three students, root == 0 blocks" % (_F, _C), B=2, C=_C, F=_F,
             S=1031)
        _row("d3_bwd", D3_B, "distill3 bwd: %s, C = %d, three students, root == 0 blocks" % (_rung, _C), B=2, C=_C, F=_F,
             S=1031)
for _F in (4, 7):
    _row("ds_bwd", DS_B, "distill bwd: coef == 0 with non-finite student flows, F = %d: gradient exactly 0" % _F, B=2, C=3,
         F=_F, S=515, coef0=True)
    _row("d3_bwd", D3_B, "distill3 bwd: coef == 0 with non-finite student flows, F = %d: gradient exactly 0" % _F, B=2, C=3,
         F=_F, S=515, coef0=True)
for _op, _k in (("ds_fwd", DS_F), ("d3_fwd", D3_F)):
    _row(_op, _k, "%s: B * S = 262144, every thread of the 1024 blocks takes one voxel" % _k, C=1, F=2, S=FWD_CAP)
    _row(_op, _k, "%s: B * S = 262145, second trip of the grid-stride loop" % _k, C=1, F=2, S=FWD_CAP + 1)
for _op, _k in (("ds_bwd", DS_B), ("d3_bwd", D3_B)):
    _row(_op, _k, "%s: B * S = 4194304 at the 16384-block cap, F = 2, C = 1" % _k, C=1, F=2, S=BWD_CAP)
    _row(_op, _k, "%s: B * S = 4194305, second trip, F = 2, C = 1" % _k, C=1, F=2, S=BWD_CAP + 1)
_row("ds_fwd", DS_F, "distill fwd: every operand misaligned (scalar kernel)", B=2, C=3, F=4, S=131,
     mis=dict(mi0=1, mt=2, gt=3, fi0=1, ft=2, sums=3, ws=1))
_row("ds_bwd", DS_B, "distill bwd: every operand misaligned (scalar kernel)", B=2, C=3, F=7, S=131,
     mis=dict(mi0=3, mt=1, gt=2, fi0=3, ft=1, coef=2, gf0=3))
_row("d3_fwd", D3_F, "distill3 fwd: every operand misaligned (scalar kernel)", B=2, C=3, F=4, S=131,
     mis=dict(mi0=1, mi1=2, mi2=3, mt=1, gt=2, fi0=3, fi1=1, fi2=2, ft=3, sums=1, ws=2))
_row("d3_bwd", D3_B, "distill3 bwd: every operand misaligned (scalar kernel)", B=2, C=3, F=7, S=131,
     mis=dict(mi0=3, mi1=1, mi2=2, mt=3, gt=1, fi0=2, fi1=3, fi2=1, ft=2, coef=3, gf0=1, gf1=2, gf2=3))

# ---- fs_prelu_bwd: chunk ladder, vector / scalar blocks, the two workspace halves ---------------------------------------------
PRELU = ("prelu_bwd_kernel", "prelu_ga_kernel")
for _S, _why in ((8192, "S = 8192: 1 chunk"),
                 (8193, "S = 8193: 2 chunks of 4100, the last chunk's length 4093 is not a multiple of 4"),
                 (40961, "S = 40961: 6 chunks, beyond 4"),
                 (524288, "S = 524288: 64 chunks of 8192, at the FS_PRELU_MAX_CHUNKS cap"),
                 (524292, "S = 524292: beyond the cap, 64 chunks of 8196")):
    _row("prelu", PRELU, "prelu chunk ladder, %s; grad_bias given (second workspace half)" % _why, B=1, C=2, S=_S, nw=2,
         bias=True)
_row("prelu", PRELU, "prelu chunk ladder, S = 8193 with B * C = 4: chunked rows at all four residues mod 4", B=2, C=2, S=8193,
     nw=2, bias=True)
_row("prelu", PRELU, "prelu: grad_bias NULL at 2 chunks (first workspace half only)", B=2, C=2, S=8193, nw=2)
_row("prelu", PRELU, "prelu: S = 1001 odd with B * C = 6: row bases take all four residues mod 4, vector and scalar blocks in "
     "one launch; grad_bias given", B=2, C=3, S=1001, nw=3, bias=True)
_row("prelu", PRELU, "prelu: S = 1001 odd with B * C = 6, grad_bias NULL", B=2, C=3, S=1001, nw=3)
_row("prelu", PRELU, "prelu: S = 3 smaller than one quad, tails only", B=2, C=2, S=3, nw=2, bias=True)
for _name in ("x", "g", "gx"):
    _row("prelu", PRELU, "prelu: %s misaligned -> scalar path in every block" % _name, B=2, C=2, S=1028, nw=2, bias=True,
         mis={_name: 1 + len(_name)})
_row("prelu", PRELU, "prelu: aligned S = 1028, vector path in every block (the near side of the misaligned rows)", B=2, C=2,
     S=1028, nw=2, bias=True)
_row("prelu", PRELU, "prelu: weight, ws, grad_weight and grad_bias misaligned, not inspected -> vector path", B=2, C=2, S=1028,
     nw=2, bias=True, mis=dict(a=1, ws=3, gw=2, gb=1))
_row("prelu", PRELU, "prelu: num_weights = C = 5, grad_bias given", B=2, C=5, S=260, nw=5, bias=True)
_row("prelu", PRELU, "prelu: num_weights = C = 5, grad_bias NULL", B=2, C=5, S=260, nw=5)
_row("prelu", PRELU, "prelu: num_weights = 1 with C = 5 (shared slope, one sum over every row), grad_bias given", B=2, C=5,
     S=260, nw=1, bias=True)
_row("prelu", PRELU, "prelu: num_weights = 1 with C = 5, grad_bias NULL", B=2, C=5, S=260, nw=1)
_row("prelu", PRELU, "prelu: num_weights = 1 with C = 1, grad_bias given", B=3, C=1, S=260, nw=1, bias=True)
_row("prelu", PRELU, "prelu: num_weights = 1 with C = 1, grad_bias NULL", B=3, C=1, S=260, nw=1)
