"""Ledger of the unsupervised 3-D loss kernels: one row per raw call of one C-ABI entry point of csrc/census3d.hip
(fs_census3d_dist_{fwd,bwd}) and csrc/flowsmooth3d.hip (fs_flow_smooth3d_{fwd,bwd}), with the compute kernel the call must
launch.  Plain data, read by tests/test_unsup3d_ledger.py (every compiled kernel has a row, the inputs keep the fp32 oracle
inside a quarter of the band, the reference-side mutants leave it) and tests/test_gpu_unsup3d_ledger.py (the named kernel
runs and no other, every output element lies inside its own band of an fp64 reference, between NaN-patterned guard bands).
tests/unsup3d_ledger_inputs.py builds each row's inputs, reference, per-element scale and exact expectations.

The census entry points dispatch on the radius alone (one instantiation per radius and direction); the smoothness entry
points have one kernel each.  What the rows walk besides are the rungs INSIDE the kernels: the 8 x 16 x 32 brick with its
R-voxel halo (extents one below, at and one above the brick on every axis, several bricks, the blockIdx.z decode with a
batch), zero padding, every nullable gradient, the second trip of the smoothness grid-stride loops, the pair count at
2^24, every (guide, kappa) combination -- with a row on each side of every threshold.

Row fields:
  op       cen_fwd cen_bwd (fs_census3d_dist_*), fs_fwd fs_bwd (fs_flow_smooth3d_*)
  kernel   tuple of the compute kernel symbols the call must launch (one)
  B, C, D, H, W   batch, flow channels (smoothness), extents
  R        census radius
  kind     census: vol2 is "noise" (independent), "near" (vol1 plus a perturbation), "apart" (at least 0.25 from vol1: the
           volumes smaller than the patch, where most taps are the same padding term), "equal" (bitwise vol1), "const" (two constant
           volumes); "kzero": near, with a block of zeros in grad_dist.  Smoothness: "mix" (2 * randn with the
           special blocks where the volume has room), "heavy" (2 * randn, the last voxel 1e6), "plain" (2 * randn)
  grads    census backward: the gradients asked for (g1 g2); the other pointer is NULL
  guide, kappa   smoothness: guide given, the decay
  q, eps, coef   smoothness: exponent, Charbonnier eps, coef[0] of the backward
  mis      {operand name: misalignment in floats, 0..3}
  why      the rung

Shapes are as small as the rung allows; the rows on the two sides of a threshold differ in one quantity."""

ROWS = []
HELPERS = {"fs::reduce_final_kernel"}  # common.hpp's reduction finish, launched by fs_flow_smooth3d_fwd
UNREACHABLE = {}  # every kernel of the two sources is reached by a row

FS_REDUCE_BLOCKS = 1024
BZ, BY, BX = 8, 16, 32             # census3d.hip's brick (z, y, x)
BWD_BLOCKS = 16384                 # the grid cap of flow_smooth3d_bwd_kernel
FWD_CAP = FS_REDUCE_BLOCKS * 256   # 262 144 voxels: one more starts the second trip of the smoothness forward
BWD_CAP = BWD_BLOCKS * 256         # 4 194 304: the same for the backward
TWO24 = 1 << 24                    # the pair count is exact below, rounded once above
GRID_Z = 65535                     # B * ceil(D / 8) above it is refused

OPS = ("cen_fwd", "cen_bwd", "fs_fwd", "fs_bwd")
DEFAULTS = dict(B=1, C=1, D=1, H=1, W=1, R=0, kind="", grads=(), guide=False, kappa=0.0, q=0.25, eps=1e-9, coef=0.5, mis={})
_ID_ORDER = ("B", "C", "D", "H", "W", "R", "kind", "grads", "guide", "kappa", "q", "eps", "coef")
_ALWAYS = ("D", "H", "W")


def kernel_of(op, R=0):
    """The compute kernel an entry point launches: the census ones are instantiated per radius."""
    return {"cen_fwd": "census3d_fwd_kernel<%d>" % R, "cen_bwd": "census3d_bwd_kernel<%d>" % R,
            "fs_fwd": "flow_smooth3d_fwd_kernel", "fs_bwd": "flow_smooth3d_bwd_kernel"}[op]


def make(op, why, **kw):
    assert op in OPS and set(kw) <= set(DEFAULTS), (op, kw)
    r = dict(DEFAULTS, **kw)
    r.update(op=op, kernel=(kernel_of(op, r["R"]),), why=why, mis=dict(kw.get("mis", {})), grads=tuple(kw.get("grads", ())))
    return r


def _row(op, why, **kw):
    ROWS.append(make(op, why, **kw))


def kernels_of(r):
    return r["kernel"]


def row_id(r):
    bits = [r["op"]]
    for k in _ID_ORDER:
        v = r[k]
        if v == DEFAULTS[k] and k not in _ALWAYS:
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


def bricks(r):
    """Workgroups per batch item of a census row."""
    return -(-r["D"] // BZ) * -(-r["H"] // BY) * -(-r["W"] // BX)


# ---- fs_census3d_dist_{fwd,bwd}: the 8 x 16 x 32 brick with its R-voxel halo -------------------------------------------
_GRADS = (("g1",), ("g2",), ("g1", "g2"))


def _census_shapes(R):
    P = 2 * R + 1
    return (((1, 1, 1), "1x1x1: every neighbour is padding"),
            ((2, 3, 4), "2x3x4: smaller than every patch"),
            ((P, P, P), "%dx%dx%d: one patch" % (P, P, P)),
            ((7, 16, 32), "7x16x32: D one below the 8-voxel brick"),
            ((8, 16, 32), "8x16x32: one brick exactly"),
            ((9, 16, 32), "9x16x32: D one above the brick (a second z-brick of one plane)"),
            ((8, 15, 32), "8x15x32: H one below the 16-voxel brick"),
            ((8, 17, 32), "8x17x32: H one above the brick"),
            ((8, 16, 31), "8x16x31: W one below the 32-voxel brick"),
            ((8, 16, 33), "8x16x33: W one above the brick"),
            ((9, 17, 33), "9x17x33: one above on every axis, eight bricks, seven of them slivers"),
            ((17, 33, 65), "17x33x65: three bricks per axis"))


for _R in (1, 3):
    for _n, ((_D, _H, _W), _why) in enumerate(_census_shapes(_R)):
        # (in a volume smaller than the patch most taps of a voxel are the same padding term, e = T(-v1) - T(-v2): one
        # cancellation up to 342 times over, so vol2 is kept apart from vol1 there)
        _kind = "apart" if _n < 2 else "noise" if _n % 2 == 0 else "near"
        _g = _GRADS[(_n + _R) % 3]
        _row("cen_fwd", "census fwd R = %d, %s, vol2 %s" % (_R, _why, _kind), D=_D, H=_H, W=_W, R=_R, kind=_kind)
        _row("cen_bwd", "census bwd R = %d, %s, vol2 %s, %s" % (_R, _why, _kind, " and ".join(_g)), D=_D, H=_H, W=_W, R=_R,
             kind=_kind, grads=_g)
for _n, ((_D, _H, _W), _why) in enumerate((((8, 16, 32), "8x16x32: one brick exactly"),
                                          ((9, 17, 33), "9x17x33: one above on every axis, eight bricks"))):
    _kind = ("near", "noise")[_n]
    _row("cen_fwd", "census fwd R = 2, %s, vol2 %s" % (_why, _kind), D=_D, H=_H, W=_W, R=2, kind=_kind)
    _row("cen_bwd", "census bwd R = 2, %s, vol2 %s, %s" % (_why, _kind, " and ".join(_GRADS[_n + 1])), D=_D, H=_H, W=_W,
         R=2, kind=_kind, grads=_GRADS[_n + 1])
for _R in (1, 2, 3):
    _why = "B = 3 with 17x17x33: blockIdx.z = b * nbz + z-brick with nbz = 3"
    _row("cen_fwd", "census fwd R = %d, %s" % (_R, _why), B=3, D=17, H=17, W=33, R=_R, kind="near")
    _row("cen_bwd", "census bwd R = %d, %s, %s" % (_R, _why, " and ".join(_GRADS[(_R + 1) % 3])), B=3, D=17, H=17, W=33,
         R=_R, kind="near", grads=_GRADS[(_R + 1) % 3])
for _R in (1, 3):
    _kw = dict(D=9, H=17, W=33, R=_R)
    _row("cen_fwd", "census fwd R = %d: every operand misaligned (4-byte accesses only): the aligned call's bits" % _R,
         kind="near", mis=dict(vol1=1, vol2=2, dist=3), **_kw)
    _row("cen_bwd", "census bwd R = %d: every operand misaligned (4-byte accesses only): the aligned call's bits" % _R,
         kind="near", grads=("g1", "g2"), mis=dict(vol1=3, vol2=1, gdist=2, g1=1, g2=2), **_kw)
    _row("cen_fwd", "census fwd R = %d: vol2 bitwise equal to vol1, dist exactly 0" % _R, kind="equal", **_kw)
    _row("cen_bwd", "census bwd R = %d: vol2 bitwise equal to vol1, both gradients exactly 0" % _R, kind="equal",
         grads=("g1", "g2"), **_kw)
    _row("cen_bwd", "census bwd R = %d: a block of zeros in grad_dist, gradients exactly 0 further than R from any non-zero k"
         % _R, kind="kzero", grads=("g1", "g2"), **_kw)
for _R in (1, 2, 3):
    _row("cen_fwd", "census fwd R = %d: two constant volumes pin zero padding: dist exactly 0 inside, n_out * D on the border"
         % _R, D=9, H=17, W=33, R=_R, kind="const")
_row("cen_fwd", "census fwd: B = 65535 single voxels, the largest grid z the entry point accepts", B=GRID_Z, R=1, kind="apart")
_row("cen_bwd", "census bwd: B = 65535 single voxels, the largest grid z the entry point accepts", B=GRID_Z, R=1, kind="apart",
     grads=("g1", "g2"))

# ---- fs_flow_smooth3d_{fwd,bwd} ---------------------------------------------------------------------------------------------
GUIDES = ((False, 0.0, "guide NULL, kappa 0"),
          (True, 0.0, "guide given (NaN pattern), kappa 0: the bits of the NULL row"),
          (True, 12.5, "guide given, kappa 12.5"),
          (False, 12.5, "guide NULL, kappa 12.5: unweighted, the bits of the kappa 0 row"),
          (True, 1e4, "guide given, kappa 1e4: every weight is exactly 0 or 1"))
QEPS = ((0.25, 1e-9, "q = 0.25, eps = 1e-9 (the product's)"),
        (0.5, 1e-3, "q = 0.5, eps = 1e-3"),
        (1.0, 1e-6, "q = 1, eps = 1e-6: the exponent q - 1 is 0"),
        (0.25, 2e-19, "q = 0.25, eps = 2e-19: eps^2 just above FLT_MIN"))
COEFS = (0.5, -3.0, 0.0)
_BCS = ((1, 1), (2, 6), (1, 6), (2, 1))
_SM = (((1, 7, 9), "1x7x9: no pair along D"),
       ((5, 1, 9), "5x1x9: no pair along H"),
       ((5, 7, 1), "5x7x1: no pair along W"),
       ((1, 1, 1), "1x1x1: no pair, sums == (0, 0), gradient exactly 0"),
       ((2, 2, 2), "2x2x2: every voxel on a border of every axis"),
       ((3, 4, 5), "3x4x5"))
_i = 0
for _n, ((_D, _H, _W), _why) in enumerate(_SM):
    for _k, (_guide, _kappa, _gwhy) in enumerate(GUIDES):
        _B, _C = _BCS[(_n + _k) % 4]
        _q, _eps, _qwhy = QEPS[_i % 4]
        _coef = COEFS[_i % 3]
        _kw = dict(B=_B, C=_C, D=_D, H=_H, W=_W, kind="mix", guide=_guide, kappa=_kappa, q=_q, eps=_eps)
        _what = "%s, B x C = %dx%d, %s, %s" % (_why, _B, _C, _gwhy, _qwhy)
        _row("fs_fwd", "smooth fwd " + _what, **_kw)
        _row("fs_bwd", "smooth bwd %s, coef %g" % (_what, _coef), coef=_coef, **_kw)
        _i += 1
# room for the special blocks (d == 0, a few eps, around 1e4, equal guide values): every (q, eps) with every (guide, kappa)
for _k, (_guide, _kappa, _gwhy) in enumerate(GUIDES):
    for _j, (_q, _eps, _qwhy) in enumerate(QEPS):
        _coef = COEFS[(_k + _j) % 3]
        _kw = dict(B=2, C=6, D=6, H=10, W=12, kind="mix", guide=_guide, kappa=_kappa, q=_q, eps=_eps)
        _what = "6x10x12 with the special blocks, B x C = 2x6 (flow offset b * C * DHW, guide offset b * DHW), %s, %s" % (
            _gwhy, _qwhy)
        _row("fs_fwd", "smooth fwd " + _what, **_kw)
        _row("fs_bwd", "smooth bwd %s, coef %g" % (_what, _coef), coef=_coef, **_kw)
for _C in (1, 2):
    _row("fs_fwd", "smooth fwd: 262144 voxels (1x2x131072), C = %d: every thread of the 1024 blocks takes one voxel" % _C, C=_C,
         H=2, W=FWD_CAP // 2, kind="heavy")
    _row("fs_fwd", "smooth fwd: 262146 voxels (1x2x131073), C = %d: second trip, voxel 262144 owns the heavy x-pair" % _C, C=_C,
         H=2, W=FWD_CAP // 2 + 1, kind="heavy")
_row("fs_bwd", "smooth bwd: 4194304 voxels (1x1x4194304) at the 16384-block cap", W=BWD_CAP, kind="plain")
_row("fs_bwd", "smooth bwd: 4194305 voxels (1x1x4194305), second trip", W=BWD_CAP + 1, kind="plain")
_row("fs_bwd", "smooth bwd: 4194306 voxels (1x2x2097153), second trip with H > 1, guide given, kappa 12.5", H=2,
     W=BWD_CAP // 2 + 1, kind="plain", guide=True, kappa=12.5, coef=-3.0)
for _W, _why in ((TWO24 + 1, "16777216 pairs: sums[1] == 2^24 exactly"),
                 (TWO24 + 2, "16777217 pairs: sums[1] is the once-rounded 16777216.0"),
                 (TWO24 + 4, "16777219 pairs: sums[1] is the once-rounded 16777220.0")):
    _row("fs_fwd", "smooth fwd: 1x1x%d, 64 trips, %s" % (_W, _why), W=_W, kind="plain")
_kw = dict(B=2, C=6, D=6, H=10, W=12, kind="mix", guide=True, kappa=12.5)
_row("fs_fwd", "smooth fwd: every operand misaligned (4-byte accesses only): the aligned call's bits",
     mis=dict(flow=1, guide=2, sums=3, ws=1), **_kw)
_row("fs_bwd", "smooth bwd: every operand misaligned (4-byte accesses only): the aligned call's bits",
     mis=dict(flow=3, guide=1, coef=2, gflow=1), **_kw)


def twin_of(r):
    """The row whose outputs this row's must equal bit for bit (None: there is none): the aligned call of a misaligned
    one, the NULL-guide call of kappa == 0 with a guide, the kappa == 0 call of a NULL guide with kappa > 0."""
    if r["mis"]:
        return dict(r, mis={})
    if r["op"] in ("fs_fwd", "fs_bwd"):
        if r["guide"] and r["kappa"] == 0:
            return dict(r, guide=False)
        if not r["guide"] and r["kappa"] > 0:
            return dict(r, kappa=0.0)
    return None
