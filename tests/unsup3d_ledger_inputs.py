"""Inputs, fp64 references, fp32 oracles, per-element scales, exact expectations and reference-side mutants of the rows of
tests/unsup3d_ledger.py (CPU tensors only; shared by tests/test_unsup3d_ledger.py and tests/test_gpu_unsup3d_ledger.py).

Reference: tests/census3d_ref.py evaluated in float64 on the fp32 input values, gradients from float64 autograd (0 for a
flow without a pair).  The fp32 oracle is the same functions on the float32 operands.

Bands are local: band_i = tol * s_i, s_i made from reference quantities of element i alone --
  dist                 ref_i (every tap is >= 0: the value is the sum of the absolute terms)
  census gradients     sum over the element's taps of |(k[q] + k[q+delta]) * D'(e) * T'(u)| (census_terms, written from the
                       formula of the header and census_pair.hpp; its signed sum is held to autograd by the CPU test)
  smoothness gradient  |coef| * sum over the element's up to six differences of |w * dpen(d)| (smooth_terms)
  sums[0]              |ref|
  sums[1]              compared exactly with the float nearest to the pair count
-- and where s_i == 0 the element must be exactly 0 (no band).  Tolerances are the project's own of
tests/test_gpu_census3d.py: 1e-5 for values and sums, 2e-4 for gradients; tests/test_unsup3d_ledger.py holds the fp32
oracle to a quarter of every band, so the inputs are well conditioned at every element.

Inputs are seeded from the row's op family, shape, radius and kind, so the rows of a twin pair (a misaligned call and the
aligned one, a guide that must not be read and no guide) see the same values.  Census: vol1 = rand; vol2 independent
("noise"), (vol1 + 0.25 + 0.5 * rand) mod 1 ("apart"), clamp(vol1 + 0.1 * randn) ("near", "kzero"), vol1 itself ("equal")
or two constants ("const"); grad_dist = randn, for "kzero" zero at x < 20.  Flows are 2 * randn; where the volume has room (6 x 10 x 12) three blocks are overwritten: equal
values (d == 0: gradient terms exactly 0), small integers times eps (differences of a few eps, the fp32 subtraction is
exact), 1e4 * randn (differences around 1e4).  "heavy" rows hold 1e6 in the last voxel of every channel, so the one pair
the second trip owns moves sums[0] by far more than four bands.  The guide is rand with a block of equal values; under
kappa = 1e4 it is rand quantised to eighths, so that every weight is exp(0) == 1 or exp(<= -1250) == 0 in fp32 and in
fp64 alike; with kappa == 0 it holds the NaN pattern (the kernel must not read it).

Worst error over band per entry point on an MI355X (tests/test_gpu_unsup3d_ledger.py, the LEDGER lines):
  fs_census3d_dist_fwd   0.228 (dist, R = 3, B = 3 with 17x17x33; 37 rows)
  fs_census3d_dist_bwd   0.028 (g2, R = 3, 9x17x33; 36 rows)
  fs_flow_smooth3d_fwd   0.078 (sum0, 6x10x12 with the special blocks; 58 rows)
  fs_flow_smooth3d_bwd   0.026 (gflow, 6x10x12 with the special blocks; 54 rows)
Before the forward census kernel summed each column's 2r+1 taps first it reached 0.880 on the same row: (2r+1)^3 - 1 = 342
additions to one fp32 sum bound the error by 342 * 2^-24 = 2.0e-5 of the value, beyond the 1e-5 band, and a border voxel's
equal padding terms are rounded the same way each time; (2r+1)^2 - 1 + 2r = 54 roundings of a partial sum bound it by
3.2e-6.  The fp32 oracle had the same defect (0.83 of the band) until census3d_ref summed its taps with torch.sum.
"""
import torch
import torch.nn.functional as F

import census3d_ref as ref
import unsup3d_ledger as L
from ledger_harness import NAN_BITS

VAL_TOL, GRAD_TOL = 1e-5, 2e-4
HEAVY = 1e6
CONST_A, CONST_B = 0.3, 0.7
KZERO_X = 20       # "kzero": grad_dist is zero at x < KZERO_X
ROOM = (6, 10, 12)  # the smallest volume that takes the special blocks


def gen_of(r):
    key = "%s|%d|%d|%d|%d|%d|%d|%s" % (r["op"][:2], r["B"], r["C"], r["D"], r["H"], r["W"], r["R"], r["kind"])
    return torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(key)) % 1000003)


def f32(v):
    """The value a float argument has once it went through the C ABI."""
    return float(torch.tensor(v, dtype=torch.float32))


def roomy(r):
    return r["kind"] == "mix" and all(n >= m for n, m in zip((r["D"], r["H"], r["W"]), ROOM))


def pairs(r):
    B, C, D, H, W = (r[k] for k in "BCDHW")
    return B * C * ((D - 1) * H * W + D * (H - 1) * W + D * H * (W - 1))


def out_sizes(r):
    """{output or workspace name: floats} of the row's call (nullable outputs only when asked for)."""
    n = r["B"] * r["D"] * r["H"] * r["W"]
    if r["op"] == "cen_fwd":
        return dict(dist=n)
    if r["op"] == "cen_bwd":
        return {k: n for k in r["grads"]}
    if r["op"] == "fs_fwd":
        return dict(sums=2, ws=2 * L.FS_REDUCE_BLOCKS)
    return dict(gflow=r["C"] * n)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def data(r):
    """{name: fp32 CPU tensor} of the row's inputs."""
    g = gen_of(r)
    B, C, D, H, W = (r[k] for k in "BCDHW")
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    T = {}
    if r["op"] in ("cen_fwd", "cen_bwd"):
        v1 = rand(B, 1, D, H, W)
        if r["kind"] == "noise":
            v2 = rand(B, 1, D, H, W)
        elif r["kind"] in ("near", "kzero"):
            v2 = (v1 + 0.1 * randn(B, 1, D, H, W)).clamp(0, 1)
        elif r["kind"] == "apart":
            v2 = (v1 + 0.25 + 0.5 * rand(B, 1, D, H, W)) % 1.0
        elif r["kind"] == "equal":
            v2 = v1.clone()
        else:
            assert r["kind"] == "const", r
            v1, v2 = torch.full((B, 1, D, H, W), CONST_A), torch.full((B, 1, D, H, W), CONST_B)
        T["vol1"], T["vol2"] = v1, v2
        if r["op"] == "cen_bwd":
            T["gdist"] = randn(B, 1, D, H, W)
            if r["kind"] == "kzero":
                T["gdist"][..., :KZERO_X] = 0
        return T
    flow = 2 * randn(B, C, D, H, W)
    if r["kind"] == "heavy":
        flow[:, :, -1, -1, -1] = HEAVY
    if roomy(r):
        flow[:, :, 0:3, 0:4, 0:5] = 0.75
        flow[:, :, 3:6, 0:4, 6:12] = torch.randint(0, 9, (B, C, 3, 4, 6), generator=g).float() * f32(r["eps"])
        flow[:, :, 0:3, 5:10, 0:6] = 1e4 * randn(B, C, 3, 5, 6)
    T["flow"] = flow
    if r["guide"]:
        if r["kappa"] == 0:
            guide = torch.full((B, 1, D, H, W), NAN_BITS, dtype=torch.int32).view(torch.float32)
        else:
            guide = rand(B, 1, D, H, W)
            if r["kappa"] >= 1e4:
                guide = torch.floor(guide * 8) / 8
            if roomy(r):
                guide[:, :, 2:5, 3:8, 4:10] = 0.5
        T["guide"] = guide
    if r["op"] == "fs_bwd":
        T["coef"] = torch.tensor([r["coef"]], dtype=torch.float32)
    return T


def _guide(r, T, dt):
    """The guide the operation reads, or None."""
    return T["guide"].to(dt) if r["guide"] and r["kappa"] != 0 else None


# ---- scales, restated from the formulas of the header ---------------------------------------------------------------------
def census_terms(v1, v2, k, R, centre_weight_only=False):
    """(g1, g2, s1, s2): d sum(k * dist) / d vol1, vol2 and the sums of the absolute terms, by the pair formula
         d / d v1[q] = - sum over delta of (k[q] + k[q+delta]) D'(e) T'(u1),   d / d v2[q] = + ... T'(u2),
         u = v[q+delta] - v[q] (v zero-padded, k = 0 outside), e = T(u1) - T(u2), T(u) = u / sqrt(0.81 + u^2),
         T'(u) = 0.81 / (0.81 + u^2)^1.5, D(e) = e^2 / (0.1 + e^2), D'(e) = 0.2 e / (0.1 + e^2)^2.
    centre_weight_only: the mutant that forgets the voxel's second role, k[q] in place of k[q] + k[q+delta]."""
    D, H, W = v1.shape[2:]
    p1, p2, pk = F.pad(v1, [R] * 6), F.pad(v2, [R] * 6), F.pad(k, [R] * 6)
    g1, g2, s1, s2 = (torch.zeros_like(v1) for _ in range(4))
    for dz in range(2 * R + 1):
        for dy in range(2 * R + 1):
            for dx in range(2 * R + 1):
                sl = (slice(None), slice(None), slice(dz, dz + D), slice(dy, dy + H), slice(dx, dx + W))
                u1, u2 = p1[sl] - v1, p2[sl] - v2
                e = u1 / torch.sqrt(0.81 + u1 ** 2) - u2 / torch.sqrt(0.81 + u2 ** 2)
                c = (k if centre_weight_only else k + pk[sl]) * 0.2 * e / (0.1 + e ** 2) ** 2
                a1, a2 = c * 0.81 / (0.81 + u1 ** 2) ** 1.5, c * 0.81 / (0.81 + u2 ** 2) ** 1.5
                g1, g2, s1, s2 = g1 - a1, g2 + a2, s1 + a1.abs(), s2 + a2.abs()
    return g1, g2, s1, s2


def smooth_terms(flow, guide, q, eps, kappa, coef, own_weight=False):
    """(gradient, scale): coef * d S1 / d flow and |coef| * the sum of the absolute terms.  A pair (p, p + e_a) gives
    t = w_a(p) * 2 q d (d^2 + eps^2)^(q - 1), -t to voxel p and +t to voxel p + e_a.
    own_weight: the mutant that weighs the +t a voxel gets from its backward neighbour by its own w_a(p) (1 where p has no
    forward neighbour) in place of w_a(p - e_a)."""
    g, s = torch.zeros_like(flow), torch.zeros_like(flow)
    for ax in (2, 3, 4):
        m = flow.shape[ax] - 1
        if m < 1:
            continue
        d = flow.narrow(ax, 1, m) - flow.narrow(ax, 0, m)
        t = 2 * q * d * (d ** 2 + eps ** 2).pow(q - 1)
        lo = hi = t
        if guide is not None and kappa != 0:
            w = torch.exp(-kappa * (guide.narrow(ax, 1, m) - guide.narrow(ax, 0, m)).abs())
            lo = hi = t * w
            if own_weight:
                hi = t * torch.cat([w, torch.ones_like(w.narrow(ax, 0, 1))], ax).narrow(ax, 1, m)
        g.narrow(ax, 0, m).sub_(lo)
        g.narrow(ax, 1, m).add_(hi)
        s.narrow(ax, 0, m).add_(lo.abs())
        s.narrow(ax, 1, m).add_(hi.abs())
    return coef * g, abs(coef) * s


# ---- references ---------------------------------------------------------------------------------------------------------
def _census_outputs(r, v1, v2, k, dist_fn):
    if r["op"] == "cen_fwd":
        return {"dist": dist_fn(v1, v2, r["R"])}
    a, b = v1.clone().requires_grad_(), v2.clone().requires_grad_()
    g1, g2 = torch.autograd.grad((dist_fn(a, b, r["R"]) * k).sum(), [a, b])
    return {name: gi for name, gi in (("g1", g1), ("g2", g2)) if name in r["grads"]}


def results(r, T, dt=torch.float64):
    """{output name: (tensor in dtype dt, per-element scale or None, tolerance)} -- the reference (float64, with its scale)
    or the fp32 oracle (float32, scale None) of the row's entry point on the inputs T.  sumK is sums[K]; a scale of None in
    the reference means the output is compared exactly with the float nearest to it."""
    op = r["op"]
    t = lambda name: T[name].to(dt)
    with_scale = dt == torch.float64
    if op in ("cen_fwd", "cen_bwd"):
        k = t("gdist") if op == "cen_bwd" else None
        out = _census_outputs(r, t("vol1"), t("vol2"), k, ref.census3d_dist)
        if op == "cen_fwd":
            return {"dist": (out["dist"], out["dist"].abs() if with_scale else None, VAL_TOL)}
        s = dict(zip(("g1", "g2"), census_terms(t("vol1"), t("vol2"), k, r["R"])[2:])) if with_scale else {}
        return {name: (gi, s.get(name), GRAD_TOL) for name, gi in out.items()}
    q, eps, kappa = f32(r["q"]), f32(r["eps"]), f32(r["kappa"])
    guide = _guide(r, T, dt)
    if op == "fs_fwd":
        s1, n = ref.flow_smooth3d_sums(t("flow"), guide, q, eps, kappa)
        return {"sum0": (s1, s1.abs() if with_scale else None, VAL_TOL),
                "sum1": (torch.tensor(float(n), dtype=dt), None, 0.0)}
    a = t("flow").requires_grad_()
    s1, n = ref.flow_smooth3d_sums(a, guide, q, eps, kappa)
    gf = torch.autograd.grad(s1, [a])[0] * t("coef") if n else torch.zeros_like(a)
    scale = smooth_terms(t("flow"), guide, q, eps, kappa, float(T["coef"]))[1] if with_scale else None
    return {"gflow": (gf.detach(), scale, GRAD_TOL)}


def compare(got, rf, scale, tol):
    """(worst |got - ref| / band_i over the elements with s_i > 0, number of elements with s_i == 0 that are not exactly
    the reference's 0).  Without a scale: 0 or inf, got equal to the float nearest the reference or not."""
    g = got.double().reshape(rf.shape)
    if scale is None:
        return (0.0 if torch.equal(g, rf.float().double()) else float("inf")), 0
    if not bool(torch.isfinite(g).all()):
        return float("inf"), 0
    pos = scale > 0
    d = (g - rf).abs()
    worst = float((d[pos] / (tol * scale[pos])).max()) if bool(pos.any()) else 0.0
    return worst, int((d[~pos] != 0).sum())


def exact(r, T):
    """{output name: (fp32 tensor, bool mask or None)} -- elements (all of them without a mask) the kernel must give
    exactly, besides those whose scale is 0."""
    B, C, D, H, W, R = (r[k] for k in ("B", "C", "D", "H", "W", "R"))
    E = {}
    if r["op"] in ("cen_fwd", "cen_bwd"):
        names = ("dist",) if r["op"] == "cen_fwd" else r["grads"]
        zero = torch.zeros(B, 1, D, H, W)
        if r["kind"] == "equal":
            E = {name: (zero, None) for name in names}
        elif r["kind"] == "kzero":  # further than R from any non-zero k: no tap of the voxel carries a weight
            near = F.max_pool3d((T["gdist"] != 0).float(), 2 * R + 1, 1, R) > 0
            E = {name: (zero, ~near) for name in names}
        elif r["kind"] == "const":  # the whole neighbourhood inside the volume: every u is 0
            inside = torch.zeros(B, 1, D, H, W, dtype=torch.bool)
            inside[:, :, R:D - R, R:H - R, R:W - R] = True
            E = {"dist": (zero, inside)}
        return E
    n = pairs(r)
    if r["op"] == "fs_fwd":
        E["sum1"] = (torch.tensor(float(n), dtype=torch.float64).float(), None)
        if n == 0:
            E["sum0"] = (torch.zeros(()), None)
    elif n == 0 or r["coef"] == 0:
        E["gflow"] = (torch.zeros(B, C, D, H, W), None)
    return E


def decisions(r, T, dt):
    """{what: integer tensor} -- every discontinuity decision of the row's operation, evaluated in dtype dt: which pairs
    exist (their number), and under a guide which weights are exactly 1 and exactly 0."""
    if r["op"] in ("cen_fwd", "cen_bwd"):
        return {}
    Dn = {"pairs": torch.tensor(ref.flow_smooth3d_sums(T["flow"].to(dt), None, 0.25, 1e-3)[1])}
    guide = _guide(r, T, dt)
    if guide is not None:
        kappa = torch.tensor(r["kappa"], dtype=dt)
        for ax in (2, 3, 4):
            m = guide.shape[ax] - 1
            if m >= 1:
                w = torch.exp(-kappa * (guide.narrow(ax, 1, m) - guide.narrow(ax, 0, m)).abs())
                Dn["w%d == 1" % ax], Dn["w%d == 0" % ax] = (w == 1).to(torch.int8), (w == 0).to(torch.int8)
    return Dn


# ---- mutants: what a subtly wrong kernel would compute, applied to the reference ---------------------------------------------
def census3d_dist_replicate(vol1, vol2, radius):
    """Mutant 1: census3d_ref.census3d_dist with replicate padding in place of zero padding."""
    r = radius
    D, H, W = vol1.shape[2:]
    pad = lambda v: v[:, :, torch.arange(-r, D + r).clamp(0, D - 1)][:, :, :, torch.arange(-r, H + r).clamp(0, H - 1)][
        :, :, :, :, torch.arange(-r, W + r).clamp(0, W - 1)]
    p1, p2 = pad(vol1), pad(vol2)
    dist = torch.zeros_like(vol1)
    for dz in range(2 * r + 1):
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                u1 = p1[:, :, dz:dz + D, dy:dy + H, dx:dx + W] - vol1
                u2 = p2[:, :, dz:dz + D, dy:dy + H, dx:dx + W] - vol2
                t1, t2 = u1 / torch.sqrt(0.81 + u1 ** 2), u2 / torch.sqrt(0.81 + u2 ** 2)
                d = (t1 - t2) ** 2
                dist = dist + d / (0.1 + d)
    return dist


def census_mutant(r, T, which):
    """{output name: float64 tensor} of a census row under mutant 1 ("replicate"), 2 ("bricked": every 8 x 16 x 32 brick
    evaluated on its own with zeros around it, a halo that was never loaded) or 3 ("centre_weight")."""
    v1, v2 = T["vol1"].double(), T["vol2"].double()
    k = T["gdist"].double() if r["op"] == "cen_bwd" else None
    if which == "replicate":
        return _census_outputs(r, v1, v2, k, census3d_dist_replicate)
    if which == "centre_weight":
        g1, g2 = census_terms(v1, v2, k, r["R"], centre_weight_only=True)[:2]
        return {name: gi for name, gi in (("g1", g1), ("g2", g2)) if name in r["grads"]}
    assert which == "bricked"
    out = {}
    for z0 in range(0, r["D"], L.BZ):
        for y0 in range(0, r["H"], L.BY):
            for x0 in range(0, r["W"], L.BX):
                sl = (slice(None), slice(None), slice(z0, z0 + L.BZ), slice(y0, y0 + L.BY), slice(x0, x0 + L.BX))
                part = _census_outputs(r, v1[sl], v2[sl], None if k is None else k[sl], ref.census3d_dist)
                for name, p in part.items():
                    out.setdefault(name, torch.zeros_like(v1))[sl] = p
    return out


def near_brick_face(r):
    """[D,H,W] bool: voxels within R of a face between two bricks (where a missing halo can show)."""
    def axis(n, b):
        i = torch.arange(n)
        near = torch.zeros(n, dtype=torch.bool)
        for f in range(b, n, b):  # the face between voxels f - 1 and f
            near |= (i >= f - r["R"]) & (i < f + r["R"])
        return near
    z, y, x = axis(r["D"], L.BZ), axis(r["H"], L.BY), axis(r["W"], L.BX)
    return z[:, None, None] | y[None, :, None] | x[None, None, :]


def smooth_sums_mutant(r, T, which):
    """(S1, pairs) in float64 under mutant 5 ("first_trip": only the pairs owned by the first FS_REDUCE_BLOCKS * 256
    voxels) or 6 ("flat": x- and y-neighbours taken in the flattened volume without the x + 1 < W and y + 1 < H tests)."""
    flow, guide = T["flow"].double(), _guide(r, T, torch.float64)
    B, C, D, H, W = flow.shape
    q, eps, kappa = f32(r["q"]), f32(r["eps"]), f32(r["kappa"])
    pen = lambda d: (d ** 2 + eps ** 2).pow(q)
    wgt = lambda a, b: 1.0 if guide is None else torch.exp(-kappa * (b - a).abs())
    s1, n = torch.zeros((), dtype=torch.float64), 0
    if which == "first_trip":
        owner = torch.arange(B * D * H * W).view(B, 1, D, H, W)
        for ax in (2, 3, 4):
            m = flow.shape[ax] - 1
            if m < 1:
                continue
            own = (owner.narrow(ax, 0, m) < L.FWD_CAP).expand(B, C, *owner.narrow(ax, 0, m).shape[2:])
            p = pen(flow.narrow(ax, 1, m) - flow.narrow(ax, 0, m))
            if guide is not None:
                p = p * wgt(guide.narrow(ax, 0, m), guide.narrow(ax, 1, m))
            s1, n = s1 + (p * own).sum(), n + int(own.sum())
        return s1, n
    assert which == "flat"
    fl = flow.reshape(B, C, -1)
    gl = None if guide is None else guide.reshape(B, 1, -1)
    for stride in (H * W, W, 1):
        if stride >= fl.shape[2]:
            continue
        p = pen(fl[..., stride:] - fl[..., :-stride])
        if gl is not None:
            p = p * wgt(gl[..., :-stride], gl[..., stride:])
        s1, n = s1 + p.sum(), n + p.numel()
    return s1, n
