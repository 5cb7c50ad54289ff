"""Ledger of the correlation and plane-moment kernels: one row per raw call of one C-ABI entry point of csrc/corr2d.hip
(fs_corr2d_{fwd,bwd}, fs_corr2d_norm_{fwd,bwd}, fs_corr2d_pair_{fwd,bwd}, fs_plane_moments[4], fs_plane_norm_bwd[4]) and
csrc/corr3d.hip (fs_corr3d_{fwd,bwd}), both over csrc/corr_q.hpp, with the kernel the dispatch code (launch_fwd /
launch_bwd / launch_small_fwd of corr2d.hip, launch of corr3d.hip) must pick for it.  Plain data, read by
tests/test_corr_ledger.py (every compiled kernel of either source has a row, threshold pairs differ in one field, the
fp32 oracle stays inside every band, the bands notice an omitted channel / slice / displacement row / stride trip) and
tests/test_gpu_corr_ledger.py (the named kernel runs and no other, every output matches an fp64 reference inside
NaN-patterned guard bands).  tests/corr_ledger_inputs.py builds each row's inputs, references, exact expectations and bands.

The two sources compile kernels with the same normalised names (corr_fwd_q_kernel<MD, 1>, corr_bwd_q_kernel<MD>) in
different anonymous namespaces: a kernel is keyed by (src, kernel).

Row fields:
  op       c2_fwd c2_bwd (fs_corr2d_*), n_fwd n_bwd (fs_corr2d_norm_*), p_fwd p_bwd (fs_corr2d_pair_*), mom mom4
           (fs_plane_moments[4]), nb nb4 (fs_plane_norm_bwd[4]), c3_fwd c3_bwd (fs_corr3d_*), chain (fs_plane_moments4 ->
           fs_corr2d_pair_fwd -> fs_corr2d_pair_bwd -> fs_plane_norm_bwd4, four calls, four kernels)
  src      the source file whose kernel must run
  kernel   tuple of the kernel symbols the call must launch (one; chain: four)
  B C D H W md   the correlation's shape (D: 3-D only);  planes, S: the moment kernels' shape
  grads    the nullable outputs asked for (bwd: g1 g2; p_bwd: g1a g2a g1b g2b; nb4: gfa gfb gfc gfd); the others are NULL
  stats    p_fwd / p_bwd: the (mean, rstd) tables are given (normalisation folded in)
  alias    pair form as the model uses it: f1b IS f2a and f2b IS f1a (the same device pointers);  mom4: one tensor four times
  drop     nb4: a skipped tensor's f and grad_n are NULL too
  kind     rand;  const: constant planes (their normalised map is exactly 0);  offset: planes with mean / std = 100;  int:
           small integers in every operand, so every sum is exact in any order and the output must be fl(sum / C) bitwise
  poison   None or (operand, "elem" | "sample" | "edge"): one NaN at a chosen element / the whole last sample NaN / one NaN
           of grad_out at displacement (0, +md) in the last column of a middle row
  pair     (tag, field): the two rows with this tag sit on the two sides of a threshold and differ in `field` alone
  mis      {operand name: misalignment in floats, 0..3}
  why      the rung

What reading the dispatch code gave (corr2d.hip): direct kernels up to H * W = kSmallFwd = 128 (plain forward), kSmallFwdNorm
= 32 (forward with moments; the pair form reads set 0's table pointer), kSmallBwd = 32 (both backward forms); channel
slices of launch_small_fwd: cs doubles while cs < 8, items * cs < 131072 and C / (2 cs) >= 12, so C = 23 | 24, 47 | 48,
95 | 96 are the rungs and, at md = 4 on 8x16 with C = 96 (10368 items per sample), B = 3 | 4, 6 | 7, 12 | 13 the item caps.
corr3d.hip has no direct kernels: every shape runs the tiled pair with D planes per sample and 2 md + 1 displacement planes."""

ROWS = []
HELPERS = {"fs::reduce_final_kernel"}  # common.hpp's reduction finish, compiled into every source that includes it
UNREACHABLE = {}  # every kernel of both sources is reached by a row

SRC2, SRC3 = "corr2d.hip", "corr3d.hip"
SOURCES = (SRC2, SRC3)
K_SMALL_FWD, K_SMALL_FWD_NORM, K_SMALL_BWD, ITEM_CAP, SLICE_MIN_CHANNELS = 128, 32, 32, 131072, 12


def SF(md, cs):
    return "corr2d_small_fwd_kernel<%d, %d>" % (md, cs)


def SB(md):
    return "corr2d_small_bwd_kernel<%d>" % md


def TF(md):
    return "corr_fwd_q_kernel<%d, 1>" % md


def TB(md):
    return "corr_bwd_q_kernel<%d>" % md


MOM, NB = "plane_moments_kernel", "plane_norm_bwd_kernel"

OPS = {"c2_fwd": "fs_corr2d_fwd", "c2_bwd": "fs_corr2d_bwd", "n_fwd": "fs_corr2d_norm_fwd", "n_bwd": "fs_corr2d_norm_bwd",
       "p_fwd": "fs_corr2d_pair_fwd", "p_bwd": "fs_corr2d_pair_bwd", "mom": "fs_plane_moments", "mom4": "fs_plane_moments4",
       "nb": "fs_plane_norm_bwd", "nb4": "fs_plane_norm_bwd4", "c3_fwd": "fs_corr3d_fwd", "c3_bwd": "fs_corr3d_bwd",
       "chain": "fs_plane_moments4 + fs_corr2d_pair_fwd + fs_corr2d_pair_bwd + fs_plane_norm_bwd4"}
GRADS_OF = {"c2_bwd": ("g1", "g2"), "n_bwd": ("g1", "g2"), "c3_bwd": ("g1", "g2"), "p_bwd": ("g1a", "g2a", "g1b", "g2b"),
            "nb4": ("gfa", "gfb", "gfc", "gfd")}
DEFAULTS = dict(B=1, C=1, D=1, H=1, W=1, md=4, planes=0, S=0, grads=(), stats=False, alias=False, drop=False, kind="rand",
                poison=None, pair=None, mis={})
_ID_ORDER = ("md", "B", "C", "D", "H", "W", "planes", "S", "grads", "stats", "alias", "drop", "kind", "poison")


def make(op, kernel, why, **kw):
    assert op in OPS and set(kw) <= set(DEFAULTS), (op, kw)
    r = dict(DEFAULTS, **kw)
    if op in GRADS_OF and "grads" not in kw:
        r["grads"] = GRADS_OF[op]
    r.update(op=op, src=SRC3 if op.startswith("c3_") else SRC2, kernel=kernel if isinstance(kernel, tuple) else (kernel,),
             why=why, mis=dict(kw.get("mis", {})), grads=tuple(r["grads"]))
    return r


def _row(op, kernel, why, **kw):
    ROWS.append(make(op, kernel, why, **kw))


def kernels_of(r):
    return r["kernel"]


def row_id(r):
    bits = [r["op"]]
    for k in _ID_ORDER:
        v = r[k]
        if k == "md" and r["op"] in ("mom", "mom4", "nb", "nb4"):
            continue
        if k == "grads":
            if v != GRADS_OF.get(r["op"], ()):
                bits.append("+".join(v))
        elif k == "md":
            bits.append("md%d" % v)
        elif v == DEFAULTS[k]:
            continue
        elif isinstance(v, bool):
            bits.append(k)
        elif isinstance(v, tuple):
            bits.append("nan_" + "_".join(v))
        elif isinstance(v, str):
            bits.append(v)
        else:
            bits.append("%s%d" % (k, v))
    if r["mis"]:
        bits.append("m" + "".join("%s%d" % kv for kv in sorted(r["mis"].items())))
    return "-".join(bits)


# ---- direct against tiled: kSmallFwd, kSmallFwdNorm, kSmallBwd ------------------------------------------------------------
for _op, _lim, _near, _far in (("c2_fwd", 128, SF(4, 1), TF(4)), ("n_fwd", 32, SF(4, 1), TF(4)),
                               ("c2_bwd", 32, SB(4), TB(4)), ("n_bwd", 32, SB(4), TB(4))):
    _row(_op, _near, "direct | tiled: H * W = %d, the last direct size (1 x %d)" % (_lim, _lim), B=2, C=5, W=_lim,
         pair=(_op + " threshold", "W"))
    _row(_op, _far, "direct | tiled: H * W = %d, the first tiled size (1 x %d)" % (_lim + 1, _lim + 1), B=2, C=5, W=_lim + 1,
         pair=(_op + " threshold", "W"))
_row("c2_fwd", SF(4, 1), "direct | tiled: 8 x 16 = 128 pixels, direct", B=2, C=5, H=8, W=16)
_row("c2_fwd", TF(4), "direct | tiled: 3 x 43 = 129 pixels, tiled", B=2, C=5, H=3, W=43)
for _op, _near, _far in (("n_fwd", SF(4, 1), TF(4)), ("c2_bwd", SB(4), TB(4)), ("n_bwd", SB(4), TB(4))):
    _row(_op, _near, "direct | tiled: 4 x 8 = 32 pixels, direct", B=2, C=5, H=4, W=8)
    _row(_op, _far, "direct | tiled: 3 x 11 = 33 pixels, tiled", B=2, C=5, H=3, W=11)
# the pair form reads the threshold from set 0's table pointer
for _stats in (True, False):
    _t = "with" if _stats else "without"
    for _lim in (32, 128):
        _small = _lim <= (K_SMALL_FWD_NORM if _stats else K_SMALL_FWD)
        _row("p_fwd", SF(4, 1) if _small else TF(4), "pair fwd %s stats at 1 x %d: %s" % (
            _t, _lim, "direct" if _small else "tiled on both sides of %d" % _lim), B=2, C=5, W=_lim, stats=_stats,
             pair=("p_fwd %s stats at %d" % (_t, _lim), "W"))
        _small = _lim + 1 <= (K_SMALL_FWD_NORM if _stats else K_SMALL_FWD)
        _row("p_fwd", SF(4, 1) if _small else TF(4), "pair fwd %s stats at 1 x %d: %s" % (
            _t, _lim + 1, "direct on both sides of %d" % _lim if _small else "tiled"), B=2, C=5, W=_lim + 1, stats=_stats,
             pair=("p_fwd %s stats at %d" % (_t, _lim), "W"))
    _row("p_bwd", SB(4), "pair bwd %s stats at 1 x 32: direct" % _t, B=2, C=5, W=32, stats=_stats,
         pair=("p_bwd %s stats" % _t, "W"))
    _row("p_bwd", TB(4), "pair bwd %s stats at 1 x 33: tiled" % _t, B=2, C=5, W=33, stats=_stats,
         pair=("p_bwd %s stats" % _t, "W"))

# ---- the channel-slice ladder of launch_small_fwd --------------------------------------------------------------------------
for _C, _cs in ((23, 1), (24, 2), (47, 2), (48, 4), (95, 4), (96, 8)):
    _lo = _C if _C % 2 else _C - 1
    _row("c2_fwd", SF(4, _cs), "slice ladder: C = %d -> %d slice(s) (C / (2 cs) >= 12), 8 x 16, md = 4" % (_C, _cs), C=_C, H=8,
         W=16, pair=("ladder C %d|%d" % (_lo, _lo + 1), "C"))
for _B, _cs in ((3, 8), (4, 4), (6, 4), (7, 2), (12, 2), (13, 1)):
    _lo = _B if _B in (3, 6, 12) else _B - 1
    _row("c2_fwd", SF(4, _cs), "slice ladder, item cap items * cs < 131072: C = 96, 8 x 16, md = 4, B = %d (%d items) -> %d "
         "slice(s)" % (_B, _B * 81 * 128, _cs), B=_B, C=96, H=8, W=16, pair=("ladder cap B %d|%d" % (_lo, _lo + 1), "B"))
for _md in (1, 2, 3):
    for _C, _cs in ((23, 1), (24, 2), (48, 4), (96, 8)):
        _row("c2_fwd", SF(_md, _cs), "slice ladder at md = %d: C = %d -> corr2d_small_fwd_kernel<%d, %d>" % (_md, _C, _md, _cs),
             B=2, C=_C, H=8, W=16, md=_md)
_row("c2_fwd", SF(4, 8), "slice ladder: C = 97 not divisible by its 8 slices (13 channels each, the last slice 6)", C=97, H=8,
     W=16)
_row("c2_fwd", SF(4, 2), "slice ladder: C = 25 not divisible by its 2 slices (13 and 12 channels)", C=25, H=8, W=16)
_row("c2_fwd", SF(1, 8), "slice ladder: 135 items, not a multiple of the 8 items per wave: the last wave is partly dead", C=96,
     H=3, W=5, md=1)
_row("c2_fwd", SF(2, 4), "slice ladder: 375 items of 16 per wave (7 live in the last), B = 1, C = 50", C=50, H=3, W=5, md=2)
_row("n_fwd", SF(4, 8), "direct fwd with moments: C = 96 in 8 slices, 4 x 8", B=2, C=96, H=4, W=8)
_row("n_fwd", SF(3, 2), "direct fwd with moments: C = 25 in 2 slices (13 and 12), 4 x 8, tables misaligned (4-byte aligned "
     "float2 loads)", B=2, C=25, H=4, W=8, md=3, mis=dict(st1=1, st2=3))
_row("n_fwd", SF(2, 4), "direct fwd with moments: C = 49 in 4 slices, 3 x 5", B=2, C=49, H=3, W=5, md=2)
_row("n_fwd", SF(1, 1), "direct fwd with moments: C = 7, one slice, 3 x 5", B=3, C=7, H=3, W=5, md=1)

# ---- tiled forward ----------------------------------------------------------------------------------------------------------
_CH = {1: "one partial chunk of 8", 7: "one partial chunk", 8: "exactly one chunk", 9: "one chunk plus one channel",
       16: "two chunks", 17: "two chunks plus one channel"}
for _C, _what in _CH.items():
    for _md in (1, 2, 3, 4):
        _row("c2_fwd", TF(_md), "tiled fwd: C = %d, %s; md = %d (tile 0 of sample 0: fix_head shifts by %d%s), 5 x 27" % (
            _C, _what, _md, _md, "" if _md < 4 else ", the vector is wholly masked"), B=2, C=_C, H=5, W=27, md=_md)
_row("c2_fwd", TF(4), "tiled fwd: C = 24, mean4 divides by C", B=2, C=24, H=5, W=27, pair=("mean4 C 24|32", "C"))
_row("c2_fwd", TF(4), "tiled fwd: C = 32, mean4 multiplies by 1 / C", B=2, C=32, H=5, W=27, pair=("mean4 C 24|32", "C"))
_HW = ((9, 31, "W = 31, one pixel short of the tile"), (9, 32, "W = 32, exactly one tile column"),
       (9, 33, "W = 33, a second tile column of one pixel; 2 x 2 tiles x B = 2: exactly 8 workgroups"),
       (9, 37, "W = 37"), (9, 65, "W = 65, three tile columns"), (1, 33, "H = 1"), (8, 33, "H = 8, exactly one tile row"),
       (17, 33, "H = 17, three tile rows"), (43, 3, "W = 3: one 16-byte vector spans more than one row"),
       (129, 1, "W = 1 with H = 129: a vector spans four rows"),
       (17, 65, "17 x 65: 9 tiles x B = 2 = 18 workgroups = 8 * 2 + 2, the identity tail of xcd_tile"))
for _n, (_H, _W, _what) in enumerate(_HW):
    _row("n_fwd", TF(4), "tiled fwd with moments, md = 4: %s" % _what, B=2, C=3, H=_H, W=_W)
    if _H * _W > K_SMALL_FWD:
        _row("c2_fwd", TF(1 + _n % 3), "tiled fwd, md = %d: %s" % (1 + _n % 3, _what), B=2, C=3, H=_H, W=_W, md=1 + _n % 3)
_row("c2_fwd", TF(4), "tiled fwd: 9 x 33 with B = 1: 4 workgroups, fewer than 8 (xcd_tile is the identity)", C=3, H=9, W=33)
_row("c2_fwd", TF(4), "tiled fwd: 9 x 33 with B = 5: 20 workgroups = 8 * 2 + 4", B=5, C=3, H=9, W=33)
for _md in (1, 2, 3, 4):
    _row("c2_fwd", TF(_md), "tiled fwd md = %d: every operand misaligned (f1 %d, f2 %d, out %d floats)" % (
        _md, _md % 4, (_md + 1) % 4, (_md + 2) % 4), B=2, C=9, H=9, W=33, md=_md,
         mis=dict(f1=_md % 4, f2=(_md + 1) % 4, out=(_md + 2) % 4))
_row("n_fwd", TF(2), "tiled fwd with moments: C = 9, every operand misaligned, tables 4-byte aligned", B=2, C=9, H=5, W=9, md=2,
     mis=dict(f1=1, f2=2, st1=1, st2=3, out=3))
_row("n_fwd", TF(3), "tiled fwd with moments: C = 17, tables at misalignment 1", B=2, C=17, H=5, W=9, md=3, mis=dict(st1=1, st2=1))

# integer operands: the sums are exact, so the output is fl(sum / C) bitwise -- the division of mean4, not a product with 1 / C
_row("c2_fwd", TF(4), "exact: integer operands, C = 24: mean4 must divide (sum * fl(1 / 24) is another float)", B=2, C=24, H=5,
     W=27, kind="int")
_row("c2_fwd", TF(4), "exact: integer operands, C = 32: mean4's reciprocal is exact", B=2, C=32, H=5, W=27, kind="int")
_row("c2_fwd", SF(4, 2), "exact: integer operands, direct, C = 24 in 2 slices", B=2, C=24, H=4, W=8, kind="int")
_row("c2_bwd", TB(4), "exact: integer operands, tiled bwd, C = 3: mean4 must divide", B=2, C=3, H=5, W=9, kind="int")
_row("c2_bwd", SB(4), "exact: integer operands, direct bwd, C = 3", B=2, C=3, H=4, W=8, kind="int")
_row("c3_fwd", TF(2), "exact: integer operands, 3-D fwd, C = 3", B=2, C=3, D=3, H=5, W=7, md=2, kind="int")
_row("c3_bwd", TB(2), "exact: integer operands, 3-D bwd, C = 3", B=2, C=3, D=3, H=5, W=7, md=2, kind="int")

# ---- tiled backward ---------------------------------------------------------------------------------------------------------
_CB = {1: "half a channel pair", 2: "one pair", 3: "a pair and a half", 31: "one short of the 32-channel group",
       32: "exactly one group", 33: "one channel past the group", 65: "two groups and one channel"}
for _n, (_C, _what) in enumerate(_CB.items()):
    _row("c2_bwd", TB(1 + _n % 4), "tiled bwd: C = %d, %s; md = %d, 5 x 9, both gradients" % (_C, _what, 1 + _n % 4), B=2, C=_C,
         H=5, W=9, md=1 + _n % 4)
for _C in (33, 65):
    for _grads in (("g1",), ("g2",), ("g1", "g2")):
        _row("c2_bwd", TB(4), "tiled bwd: C = %d, md = 4, %s asked for" % (_C, " and ".join(_grads)), B=2, C=_C, H=5, W=9,
             grads=_grads)
_row("c2_bwd", TB(4), "tiled bwd: 11 x 3, narrower than md = 4: the transposed direction is clipped left and right", B=2, C=3,
     H=11, W=3)
_row("c2_bwd", TB(4), "tiled bwd: 3 x 11, lower than md = 4: the transposed direction is clipped above and below", B=2, C=3, H=3,
     W=11)
_row("c2_bwd", SB(4), "direct bwd: 3 x 3, narrower and lower than md = 4: clipped on all four sides", B=2, C=3, H=3, W=3)
_row("c2_fwd", SF(4, 1), "direct fwd: 3 x 3, narrower and lower than md = 4", B=2, C=3, H=3, W=3)
for _n, (_H, _W) in enumerate(((9, 31), (9, 33), (17, 65), (43, 3), (33, 1), (8, 32))):
    _row("c2_bwd", TB(4 - _n % 3), "tiled bwd: %d x %d, md = %d, C = 3" % (_H, _W, 4 - _n % 3), B=2, C=3, H=_H, W=_W, md=4 - _n % 3)
for _md in (1, 2, 3):
    _row("c2_bwd", SB(_md), "direct bwd: md = %d, 4 x 8, C = 5" % _md, B=2, C=5, H=4, W=8, md=_md)
_row("c2_bwd", SB(4), "direct bwd: only g2 asked for, 4 x 8", B=2, C=5, H=4, W=8, grads=("g2",))
_row("c2_bwd", SB(4), "direct bwd: only g1 asked for, 4 x 8", B=2, C=5, H=4, W=8, grads=("g1",))
_row("c2_bwd", TB(3), "tiled bwd md = 3: every operand misaligned", B=2, C=3, H=9, W=33, md=3,
     mis=dict(f1=1, f2=2, gout=3, g1=1, g2=2))
_row("c2_bwd", SB(2), "direct bwd md = 2: every operand misaligned", B=2, C=5, H=4, W=8, md=2,
     mis=dict(f1=3, f2=1, gout=2, g1=3, g2=1))
for _C, _grads in ((1, ("g1", "g2")), (33, ("g1",)), (33, ("g2",)), (33, ("g1", "g2"))):
    _row("n_bwd", TB(4), "tiled bwd with moments: C = %d, 9 x 33, %s asked for, tables at misalignment 1" % (
        _C, " and ".join(_grads)), B=2, C=_C, H=9, W=33, grads=_grads, mis=dict(st1=1, st2=1))
_row("n_bwd", TB(2), "tiled bwd with moments, md = 2: every operand misaligned", B=2, C=3, H=5, W=9, md=2,
     mis=dict(f1=2, f2=3, st1=3, st2=1, gout=1, g1=2, g2=3))
_row("n_bwd", SB(3), "direct bwd with moments, md = 3, 3 x 5, tables misaligned", B=2, C=7, H=3, W=5, md=3, mis=dict(st1=1, st2=3))

# ---- the pair form -----------------------------------------------------------------------------------------------------------
for _H, _W, _kb, _fam in ((5, 9, TB(4), "tiled"), (4, 8, SB(4), "direct")):
    for _stats in (False, True):
        _t = "with" if _stats else "without"
        _kff = SF(4, 1) if _H * _W <= (K_SMALL_FWD_NORM if _stats else K_SMALL_FWD) else TF(4)
        for _alias in (False, True):
            _a = "aliased as the model calls it (f1b = f2a, f2b = f1a)" if _alias else "distinct sets"
            _row("p_fwd", _kff, "pair fwd (%s) %s stats, %d x %d, %s" % ("tiled" if _kff == TF(4) else "direct", _t, _H, _W, _a),
                 B=2, C=5, H=_H, W=_W, stats=_stats, alias=_alias)
            _row("p_bwd", _kb, "pair bwd (%s) %s stats, %d x %d, %s, all four gradients" % (_fam, _t, _H, _W, _a), B=2, C=5, H=_H,
                 W=_W, stats=_stats, alias=_alias)
_P4 = ("g1a", "g2a", "g1b", "g2b")
for _n, _g in enumerate(_P4):
    for _k, _grads in enumerate(((_g,), tuple(x for x in _P4 if x != _g))):
        _tiled = (_n + _k) % 2 == 0
        _row("p_bwd", TB(4) if _tiled else SB(4), "pair bwd (%s): %s asked for, the rest NULL" % (
            "tiled, C = 33" if _tiled else "direct", " ".join(_grads)), B=2, C=33 if _tiled else 5, H=5 if _tiled else 4,
             W=9 if _tiled else 8, stats=bool(_n % 2), grads=_grads)
_row("p_fwd", TF(2), "pair fwd with stats, md = 2: every operand misaligned", B=2, C=9, H=5, W=9, md=2, stats=True,
     mis=dict(f1a=1, f2a=2, f1b=3, f2b=1, stats=1, outa=2, outb=3))
_row("p_bwd", TB(2), "pair bwd with stats, md = 2: every operand misaligned", B=2, C=3, H=5, W=9, md=2, stats=True,
     mis=dict(f1a=3, f2a=1, f1b=2, f2b=3, stats=3, gouta=1, goutb=2, g1a=3, g2a=1, g1b=2, g2b=1))

# ---- 3-D ------------------------------------------------------------------------------------------------------------------------
_D3 = {1: (1, 2, 3, 4), 2: (1, 2, 3, 5, 6), 4: (1, 2, 4, 5, 9, 10)}  # D = 1, 2, md, md + 1, 2 md + 1, 2 md + 2
_n = 0
for _md, _Ds in _D3.items():
    for _D in _Ds:
        _what = ("D = %d %s md = %d" % (_D, "<" if _D < _md else ("==" if _D == _md else ">"), _md)) + (
            ", D = 2 md + 1" if _D == 2 * _md + 1 else (", D = 2 md + 2: only now one slice sees every displacement plane"
                                                        if _D == 2 * _md + 2 else ""))
        _big = _md == 4 and _D == 10
        _H, _W, _B = (8, 33, 1) if _big else (5, 7, 1 + _n % 2)
        _row("c3_fwd", TF(_md), "3-D fwd: %s; planes with z + dz outside are written as 0; %d x %d" % (_what, _H, _W), B=_B, C=3,
             D=_D, H=_H, W=_W, md=_md)
        _grads = (("g1", "g2"), ("g1",), ("g2",))[_n % 3]
        _row("c3_bwd", TB(_md), "3-D bwd: %s; %s; %s asked for; %d x %d" % (
            _what, "the first and last displacement planes are skipped at every slice" if _D <= _md else
            ("skipped at the outer slices" if _D <= 2 * _md + 1 else "skipped at all but the middle slices"),
            " and ".join(_grads), 5, 7), B=_B, C=3, D=_D, H=5, W=7, md=_md, grads=_grads)
        _n += 1
_row("c3_bwd", TB(4), "3-D bwd: md = 4, D = 10 on 8 x 33, both gradients", C=2, D=10, H=8, W=33)
_row("c3_bwd", TB(2), "3-D bwd: C = 33, one channel past the group, D = 3, md = 2", B=2, C=33, D=3, H=5, W=7, md=2)
_row("c3_fwd", TF(2), "3-D fwd: C = 9, one chunk plus one channel, D = 3, md = 2", B=2, C=9, D=3, H=5, W=7, md=2)
_row("c3_fwd", TF(1), "3-D fwd md = 1: every operand misaligned", B=2, C=3, D=3, H=5, W=7, md=1, mis=dict(f1=1, f2=3, out=2))
_row("c3_bwd", TB(1), "3-D bwd md = 1: every operand misaligned", B=2, C=3, D=3, H=5, W=7, md=1,
     mis=dict(f1=2, f2=1, gout=3, g1=1, g2=3))
_row("c3_fwd", TF(3), "3-D fwd md = 3 (the fourth instantiation), D = 4", C=3, D=4, H=5, W=7, md=3)
_row("c3_bwd", TB(3), "3-D bwd md = 3 (the fourth instantiation), D = 4", C=3, D=4, H=5, W=7, md=3)

# ---- constant planes: the normalised map is exactly 0 ------------------------------------------------------------------------
_row("n_fwd", TF(4), "constant planes, tiled: C = 1, both maps constant: every output is exactly 0", B=2, H=5, W=9, kind="const")
_row("n_fwd", SF(4, 1), "constant planes, direct: C = 1, both maps constant: every output is exactly 0", B=2, H=4, W=8,
     kind="const")
_row("n_fwd", TF(4), "constant planes, tiled: C = 3, the last channel of both maps constant (it adds exactly 0)", B=2, C=3, H=5,
     W=9, kind="const")
_row("n_bwd", TB(4), "constant planes, tiled: C = 3, the gradient w.r.t. the channel facing a constant plane is exactly 0",
     B=2, C=3, H=5, W=9, kind="const")
_row("n_bwd", SB(4), "constant planes, direct: C = 3, the gradient w.r.t. the channel facing a constant plane is exactly 0",
     B=2, C=3, H=4, W=8, kind="const")

# ---- plane moments and their adjoint ------------------------------------------------------------------------------------------
_SS = {2: "the smallest plane", 3: "S = 3", 24: "UPFlow's coarsest plane", 255: "one short of the 256-thread stride",
       256: "exactly one trip of the stride loop", 257: "one element in the second trip", 512: "two full trips",
       513: "one element in the third trip", 4294: "UPFlow's finest plane, 17 trips"}
for _n, (_S, _what) in enumerate(_SS.items()):
    for _planes in (1, 3):
        _row("mom", MOM, "moments: S = %d, %s; planes = %d" % (_S, _what, _planes), planes=_planes, S=_S)
        _row("nb", NB, "moment adjoint: S = %d, %s; planes = %d" % (_S, _what, _planes), planes=_planes, S=_S)
for _S in (257, 4294):
    _row("mom", MOM, "moments: mean / std = 100 at S = %d (a one-pass fp32 variance would leave the band)" % _S, planes=3, S=_S,
         kind="offset")
    _row("nb", NB, "moment adjoint: mean / std = 100 at S = %d" % _S, planes=3, S=_S, kind="offset")
_row("mom", MOM, "moments: constant planes (mean exact, rstd = 1e8)", planes=3, S=257, kind="const")
_row("nb", NB, "moment adjoint: constant planes (n == 0, rstd = 1e8)", planes=3, S=257, kind="const")
_row("mom", MOM, "moments: f and stats misaligned", planes=3, S=257, mis=dict(f=1, stats=3))
_row("nb", NB, "moment adjoint: every operand misaligned", planes=3, S=257, mis=dict(f=3, stats=1, gn=2, gf=1))
for _S in (24, 257):
    _row("mom4", MOM, "moments4: four distinct tensors, S = %d, the [4][planes][2] layout" % _S, planes=3, S=_S)
    _row("mom4", MOM, "moments4: one tensor given four times, S = %d: four equal tables" % _S, planes=3, S=_S, alias=True)
_row("mom4", MOM, "moments4: every operand misaligned", planes=3, S=257, mis=dict(fa=1, fb=2, fc=3, fd=1, stats=1))
_G4 = GRADS_OF["nb4"]
_row("nb4", NB, "moment adjoint x 4: all four tensors", planes=3, S=257)
for _n, _g in enumerate(_G4):
    _row("nb4", NB, "moment adjoint x 4: %s NULL (its f and grad_n %s)" % (_g, "NULL too" if _n % 2 else "given"), planes=3, S=257,
         grads=tuple(x for x in _G4 if x != _g), drop=bool(_n % 2))
    _row("nb4", NB, "moment adjoint x 4: only %s given (f and grad_n of the skipped tensors %s)" % (
        _g, "given" if _n % 2 else "NULL too"), planes=3, S=24, grads=(_g,), drop=not _n % 2)
_row("nb4", NB, "moment adjoint x 4: every operand misaligned", planes=3, S=257,
     mis=dict(fa=1, fb=2, fc=3, fd=1, stats=3, gna=2, gnb=3, gnc=1, gnd=2, gfa=3, gfb=1, gfc=2, gfd=3))

# ---- chains: moments4 -> pair_fwd -> pair_bwd -> norm_bwd4 against autograd through the oracle ---------------------------------
_row("chain", (MOM, TF(4), TB(4), NB), "chain, tiled: 5 x 9, C = 5, distinct sets", B=2, C=5, H=5, W=9, stats=True)
_row("chain", (MOM, SF(4, 1), SB(4), NB), "chain, direct: 4 x 8, C = 5, distinct sets", B=2, C=5, H=4, W=8, stats=True)
_row("chain", (MOM, TF(4), TB(4), NB), "chain, tiled: 9 x 33, C = 33, aliased as the model calls it", B=2, C=33, H=9, W=33,
     stats=True, alias=True)
_row("chain", (MOM, SF(2, 2), SB(2), NB), "chain, direct: 3 x 8, C = 25 in 2 slices, md = 2, aliased", B=2, C=25, H=3, W=8, md=2,
     stats=True, alias=True)

# ---- poison: one NaN / a NaN sample next to a finite one; the non-finite set must be the reference's -------------------------
_row("c2_fwd", SF(4, 2), "poison, direct fwd: the last sample of f2 is NaN, C = 25 in 2 slices", B=2, C=25, H=4, W=8,
     poison=("f2", "sample"))
_row("c2_fwd", SF(4, 1), "poison, direct fwd: one NaN in f2", B=2, C=5, H=4, W=8, poison=("f2", "elem"))
_row("c2_bwd", SB(4), "poison, direct bwd: one NaN in grad_out (centre displacement)", B=2, C=5, H=4, W=8,
     poison=("gout", "elem"))
_row("c2_bwd", SB(4), "poison, direct bwd: the last sample of f2 is NaN", B=2, C=5, H=4, W=8, poison=("f2", "sample"))
_row("c2_fwd", TF(4), "poison, tiled fwd: the last sample of f2 is NaN, C = 9: the masked channel lanes of sample 0's second "
     "chunk read it", B=2, C=9, H=5, W=27, poison=("f2", "sample"))
_row("c2_fwd", TF(4), "poison, tiled fwd: the last sample of f1 is NaN, C = 9", B=2, C=9, H=5, W=27, poison=("f1", "sample"))
_row("c2_fwd", TF(2), "poison, tiled fwd: one NaN in f2, md = 2", B=2, C=9, H=9, W=33, md=2, poison=("f2", "elem"))
_row("c2_bwd", TB(4), "poison, tiled bwd, first direction: the last sample of f2 is NaN, C = 33: the masked channel lanes of "
     "sample 0's second group read it", B=2, C=33, H=5, W=9, poison=("f2", "sample"))
_row("c2_bwd", TB(4), "poison, tiled bwd, second direction: the last sample of f1 is NaN, C = 33", B=2, C=33, H=5, W=9,
     poison=("f1", "sample"))
_row("c2_bwd", TB(4), "poison, tiled bwd: one NaN in grad_out (centre displacement), both directions", B=2, C=3, H=9, W=33,
     poison=("gout", "elem"))
_row("c2_bwd", TB(4), "poison, tiled bwd, second direction: one NaN in grad_out at displacement (0, +md) in the last column: its "
     "target lies outside the image, so grad_f2 stays finite -- unless the column mask of the transposed gradient lets the "
     "neighbouring row's vector in; only g2 asked for", B=2, C=3, H=9, W=33, grads=("g2",), poison=("gout", "edge"))
_row("c2_bwd", TB(4), "poison, tiled bwd: the last sample of grad_out is NaN", B=2, C=3, H=5, W=9, poison=("gout", "sample"))
_row("c3_fwd", TF(2), "poison, 3-D fwd: the last sample of f2 is NaN, C = 9", B=2, C=9, D=3, H=5, W=7, md=2,
     poison=("f2", "sample"))
_row("c3_fwd", TF(2), "poison, 3-D fwd: one NaN in f2", B=2, C=3, D=3, H=5, W=7, md=2, poison=("f2", "elem"))
_row("c3_bwd", TB(2), "poison, 3-D bwd: the last sample of f2 is NaN, C = 33", B=2, C=33, D=3, H=5, W=7, md=2,
     poison=("f2", "sample"))
_row("c3_bwd", TB(2), "poison, 3-D bwd: one NaN in grad_out (centre displacement)", B=2, C=3, D=3, H=5, W=7, md=2,
     poison=("gout", "elem"))
