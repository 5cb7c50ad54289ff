"""Inputs, fp64 references, fp32 oracles, exact expectations and bands of the rows of tests/loss_ledger.py (CPU tensors only;
shared by tests/test_loss_ledger.py and tests/test_gpu_loss_ledger.py).

Reference: the operation in plain torch, evaluated in float64 on the fp32 input values (oracle/losses.py gives the
formulas; the census distance is restated here because the oracle's builds a float weight); gradients from float64 autograd,
written out where the ABI defines what autograd does not (distill: 0 at root == 0 and at coef == 0; PReLU).  The fp32
oracle is the same code in float32 (the census distance: oracle.losses.census_dist itself).

Bands, at every element, band(ref, tol) = tol * max(1, max|ref|): loss sums 1e-5 (test_photo_loss_function_vs_oracle,
test_census_vs_oracle_c3_shape), gradients 2e-4 (the relerr bound of test_gpu_losses.py), merged / sigmoid 1e-6
(test_merge_distill_l1_vs_oracle), census distance 2e-4 (test_census_vs_oracle_c3_shape).  Exact where the arithmetic is:
sums[1] of 0 / 1 weights and of the distill mask (integer partial sums below 2^24), sums[1] == 0 without a weight, grad_x
of PReLU (bit-equal to torch.where(x > 0, g, a * g) in fp32), every gradient element whose weight, mask, root or coef is 0.

Kinks and jumps: the inputs keep every element away from them (values are moved, never excluded): |x - y| and
|x - y + 1e-6| >= MARGIN_V for the penalties (sign / abs-robust derivative), |mean|mi - gt| - mean|mt - gt| - 0.01| >=
MARGIN_MASK for the distill mask, (1 - r) / 2 of wssim within [MARGIN_SSIM, 1 - MARGIN_SSIM] on textured images (uniform
noise, and noise plus a perturbation; near-constant images, where the fp32 variance cancels against c2, are no row),
|x| >= MARGIN_X for PReLU.  tests/test_loss_ledger.py accepts the margins: every decision is the same in fp32 and fp64.

Worst error over band per entry point on an MI355X (tests/test_gpu_loss_ledger.py, the LEDGER lines):
  fs_robust_sum        0.009 (sum0; 40 rows)
  fs_robust_sum_bwd    0.001 (gy; 38 rows)
  fs_census_dist_fwd   0.005 (dist; 13 rows)
  fs_census_dist_bwd   0.005 (g2; 19 rows)
  fs_wssim_fwd         0.130 (sum0; 29 rows)
  fs_wssim_bwd         0.025 (gy; 38 rows)
  fs_merge_fwd         0.129 (merged; 8 rows)
  fs_merge_bwd         0.001 (gm; 17 rows)
  fs_distill_fwd       0.004 (sum0; 13 rows)
  fs_distill_bwd       0.000 (gf0; 15 rows)
  fs_distill3_fwd      0.007 (sum2; 13 rows)
  fs_distill3_bwd      0.000 (gf2; 15 rows)
  fs_prelu_bwd         0.005 (gw; 21 rows)
"""
import math

import torch
import torch.nn.functional as F

import loss_ledger as L
from oracle import losses as olosses

SUM_TOL, GRAD_TOL, MERGE_TOL, CENSUS_TOL = 1e-5, 2e-4, 1e-6, 2e-4
MARGIN_V, MARGIN_MASK, MARGIN_SSIM, MARGIN_X = 0.02, 1e-3, 1e-3, 0.05
COEF = 0.37
LOGITS = (0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0)


def gen_of(r):
    return torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(L.row_id(r))) % 1000003)


def band(ref, tol):
    return tol * max(1.0, float(ref.abs().max()))


def f32(v):
    """The value a float argument has once it went through the C ABI."""
    return float(torch.tensor(v, dtype=torch.float32))


def nstud(r):
    return 3 if r["op"].startswith("d3_") else 1


def out_sizes(r):
    """{output or workspace name: floats} of the row's call (nullable outputs only when asked for)."""
    op, B, C, S, Fc = r["op"], r["B"], r["C"], r["S"], r["F"]
    n = B * C * S
    if op in ("rs_fwd", "ws_fwd", "ds_fwd"):
        return dict(sums=2, ws=2 * L.FS_REDUCE_BLOCKS)
    if op == "d3_fwd":
        return dict(sums=4, ws=4 * L.FS_REDUCE_BLOCKS)
    if op in ("rs_bwd", "ws_bwd"):
        return {k: n for k in r["grads"]}
    if op == "cen_fwd":
        return dict(dist=B * S)
    if op == "cen_bwd":
        return {k: B * 3 * S for k in r["grads"]}
    if op == "mg_fwd":
        return dict(merged=n, **({"sig": B * S} if r["sig"] else {}))
    if op == "mg_bwd":
        return {k: (B * S if k == "gm" else n) for k in r["grads"]}
    if op in ("ds_bwd", "d3_bwd"):
        return {"gf%d" % k: B * Fc * S for k in range(nstud(r))}
    assert op == "prelu"
    d = dict(gx=n, gw=r["nw"], ws=B * C * L.FS_PRELU_MAX_CHUNKS * (2 if r["bias"] else 1))
    if r["bias"]:
        d["gb"] = C
    return d


# ---- the operations, dtype-generic --------------------------------------------------------------------------------------
def pen(v, mode, q, eps):
    if mode == L.ABS_ROBUST:
        return (v.abs() + 0.01).pow(q)
    if mode == L.CHARBONNIER:
        return (v * v + eps).pow(q)
    if mode == L.L1_EPS:
        return (v + 1e-6).abs()
    return v.abs()


def rs_weight(r, T, dt):
    """The weight [B,1,S] with the border zeroed, or None."""
    if r["wkind"] is None:
        return None
    w = T["w"].to(dt)
    b = r["border"]
    if b > 0:
        inner = torch.zeros(r["H"], r["W"], dtype=dt)
        if r["H"] > 2 * b and r["W"] > 2 * b:
            inner[b:r["H"] - b, b:r["W"] - b] = 1
        w = w * inner.view(1, 1, -1)
    return w


def census_dist(i1, i2):
    """oracle.losses.census_dist (max_distance 3) without its float32 identity convolution: the 49 zero-padded shifts."""
    def ternary(img):
        gray = 0.2989 * img[:, 0:1] + 0.5870 * img[:, 1:2] + 0.1140 * img[:, 2:3]
        H, W = gray.shape[-2:]
        p = F.pad(gray, [3, 3, 3, 3])
        t = torch.cat([p[:, :, j:j + H, i:i + W] for j in range(7) for i in range(7)], 1) - gray
        return t / torch.sqrt(0.81 + t ** 2)

    d = (ternary(i1) - ternary(i2)) ** 2
    return torch.sum(d / (0.1 + d), 1, keepdim=True)


def ssim_half(x, y, w):
    """(1 - r) / 2 of weighted_ssim before its clamp (oracle.losses.weighted_ssim, c1 = inf)."""
    pool = lambda z: F.avg_pool2d(z, (3, 3), (1, 1))
    inv = 1.0 / (pool(w) + 0.01)
    wp = lambda z: pool(z * (w + 0.01)) * inv
    mx, my = wp(x), wp(y)
    n = 2 * (wp(x * y) - mx * my) + 9e-6
    d = (wp(x * x) - mx * mx) + (wp(y * y) - my * my) + 9e-6
    return (1 - n / d) / 2


def distill_margin(mi, mt, gt):
    return (mi - gt).abs().mean(1, True) - ((mt - gt).abs().mean(1, True) + 0.01)


def distill_root(fi, ft):
    return ((ft - fi) ** 2).mean(1, True).sqrt()


# ---- inputs -------------------------------------------------------------------------------------------------------------
HEAVY = 1000.0


def second_trip(r):
    """Work items (elements, windows, voxels) a forward reduction has beyond the FS_REDUCE_BLOCKS * 256 of its first trip.
    Where that is a single item it is made heavy (a difference of HEAVY, a weight of 50, a mask of 1): among 262 144
    ordinary items one more would move the sums by less than their band, and a kernel that dropped it would pass."""
    op, B, C, S = r["op"], r["B"], r["C"], r["S"]
    units = {"rs_fwd": B * C * S, "ws_fwd": B * C * (r["H"] - 2) * (r["W"] - 2), "ds_fwd": B * S, "d3_fwd": B * S}.get(op, 0)
    return max(0, units - L.FWD_CAP)


def _equal_block(r, k):
    S = r["S"]
    n = max(1, S // 7)
    lo = (3 + k * (S // 3)) % (S - n + 1)
    return lo, lo + n


def data(r):
    """{name: fp32 CPU tensor} of the row's inputs."""
    g = gen_of(r)
    op, B, C, S = r["op"], r["B"], r["C"], r["S"]
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    T = {}
    heavy = second_trip(r) == 1
    if op in ("rs_fwd", "rs_bwd"):
        d = (MARGIN_V * 1.25 + rand(B, C, S)) * torch.where(rand(B, C, S) < 0.5, -1.0, 1.0)
        if heavy:
            d.view(-1)[-1] = HEAVY
        if r["with_y"]:
            T["y"] = rand(B, C, S)
            T["x"] = T["y"] + d
        else:
            T["x"] = d
        if r["wkind"] == "01":
            T["w"] = (rand(B, 1, S) < 0.7).float()
        elif r["wkind"] == "float":
            T["w"] = rand(B, 1, S)
        if heavy:
            T["w"].view(-1)[-1] = 1.0
    elif op in ("cen_fwd", "cen_bwd"):
        T["img1"], T["img2"] = rand(B, 3, r["H"], r["W"]), rand(B, 3, r["H"], r["W"])
        if op == "cen_bwd":
            T["gdist"] = randn(B, 1, r["H"], r["W"])
    elif op in ("ws_fwd", "ws_bwd"):
        H, W = r["H"], r["W"]
        x, w = rand(B, C, H, W), rand(B, 1, H, W)
        if heavy:
            w[..., -3:] = 50.0  # the last window
        y = rand(B, C, H, W) if r["ykind"] == "noise" else x + 0.3 * (rand(B, C, H, W) - 0.5)
        for _ in range(8):  # windows whose (1 - r) / 2 is near a clamp end: independent noise at their centre pixel
            h = ssim_half(x.double(), y.double(), w.double())
            bad = (h < 2 * MARGIN_SSIM) | (h > 1 - 2 * MARGIN_SSIM)
            if not bad.any():
                break
            y[:, :, 1:-1, 1:-1] = torch.where(bad, rand(B, C, H - 2, W - 2), y[:, :, 1:-1, 1:-1])
        T["x"], T["y"], T["w"] = x, y, w
    elif op in ("mg_fwd", "mg_bwd"):
        T["w0"], T["w1"], T["m"] = randn(B, C, S), randn(B, C, S), randn(B, 1, S) * 3
        m = T["m"].view(-1)
        m[:7] = torch.tensor(LOGITS)
        m[-7:] = torch.tensor(LOGITS[::-1])  # (the last voxels: the second trip of the large rows)
        if op == "mg_bwd":
            T["gmerged"] = randn(B, C, S)
            if r["gsig"]:
                T["gsig"] = randn(B, 1, S)
    elif op in ("ds_fwd", "ds_bwd", "d3_fwd", "d3_bwd"):
        Fc = r["F"]
        T["gt"] = rand(B, C, S)
        T["mt"] = T["gt"] + 0.05 * randn(B, C, S)
        T["ft"] = randn(B, Fc, S)
        if heavy:
            T["mt"][..., -1] = T["gt"][..., -1]
        for k in range(nstud(r)):
            mi = T["gt"] + (0.06 + 0.02 * k) * randn(B, C, S)
            if heavy:
                mi[..., -1] = T["gt"][..., -1] + 1.0  # mask 1
            for _ in range(4):  # voxels whose mask margin is near 0: the first channel moves away from gt
                bad = distill_margin(mi.double(), T["mt"].double(), T["gt"].double()).abs() < 2 * MARGIN_MASK
                if not bad.any():
                    break
                d0 = mi[:, 0:1] - T["gt"][:, 0:1]
                mi[:, 0:1] = torch.where(bad, T["gt"][:, 0:1] + d0 + torch.where(d0 < 0, -1.0, 1.0) * 6 * MARGIN_MASK * C,
                                         mi[:, 0:1])
            T["mi%d" % k] = mi
            fi = T["ft"] + (0.5 + 0.25 * k) * randn(B, Fc, S)
            lo, hi = _equal_block(r, k)
            fi[:, :, lo:hi] = T["ft"][:, :, lo:hi]  # root == 0
            if heavy:
                fi[..., -1] = T["ft"][..., -1] + HEAVY
            if r["coef0"]:
                fi[:, :, 5], fi[:, 0, 11], fi[:, -1, 17] = float("nan"), float("inf"), float("-inf")
            T["fi%d" % k] = fi
    else:
        assert op == "prelu"
        T["x"] = (MARGIN_X + randn(B, C, S).abs()) * torch.where(rand(B, C, S) < 0.5, -1.0, 1.0)
        T["g"] = randn(B, C, S)
        T["a"] = 0.25 - 0.1 * torch.arange(r["nw"], dtype=torch.float32)
    if op in ("rs_bwd", "ws_bwd", "ds_bwd", "d3_bwd"):
        T["coef"] = torch.tensor([0.0 if r["coef0"] else COEF])
    return T


# ---- kinks: how far the inputs stay away, and what is decided -----------------------------------------------------------------
def margins(r, T):
    """[(what, smallest distance to the kink in float64, distance the inputs promise)]."""
    op = r["op"]
    if op in ("rs_fwd", "rs_bwd"):
        v = T["x"].double() - T["y"].double() if r["with_y"] else T["x"].double()
        out = [("|x - y|", float(v.abs().min()), MARGIN_V)]
        if r["mode"] == L.L1_EPS:
            out.append(("|x - y + 1e-6|", float((v + 1e-6).abs().min()), MARGIN_V))
        return out
    if op in ("ws_fwd", "ws_bwd"):
        h = ssim_half(T["x"].double(), T["y"].double(), T["w"].double())
        return [("(1 - r) / 2 above 0", float(h.min()), MARGIN_SSIM), ("(1 - r) / 2 below 1", float((1 - h).min()), MARGIN_SSIM)]
    if op in ("ds_fwd", "ds_bwd", "d3_fwd", "d3_bwd"):
        return [("mask margin %d" % k, float(distill_margin(T["mi%d" % k].double(), T["mt"].double(), T["gt"].double())
                                             .abs().min()), MARGIN_MASK) for k in range(nstud(r))]
    if op == "prelu":
        return [("|x|", float(T["x"].abs().min()), MARGIN_X)]
    return []


def decisions(r, T, dt):
    """{what: integer tensor} -- every discontinuity decision of the row's operation, evaluated in dtype dt."""
    op = r["op"]
    if op in ("rs_fwd", "rs_bwd"):
        v = T["x"].to(dt) - T["y"].to(dt) if r["with_y"] else T["x"].to(dt)
        return {"sign": torch.sign(v + 1e-6 if r["mode"] == L.L1_EPS else v).to(torch.int8)}
    if op in ("ws_fwd", "ws_bwd"):
        h = ssim_half(T["x"].to(dt), T["y"].to(dt), T["w"].to(dt))
        return {"clamp": (h < 0).to(torch.int8) - (h > 1).to(torch.int8)}
    if op in ("ds_fwd", "ds_bwd", "d3_fwd", "d3_bwd"):
        D = {}
        for k in range(nstud(r)):
            D["mask%d" % k] = (distill_margin(T["mi%d" % k].to(dt), T["mt"].to(dt), T["gt"].to(dt)) > 0).to(torch.int8)
            if not r["coef0"]:
                D["root%d" % k] = (distill_root(T["fi%d" % k].to(dt), T["ft"].to(dt)) > 0).to(torch.int8)
        return D
    if op == "prelu":
        return {"x > 0": (T["x"].to(dt) > 0).to(torch.int8)}
    return {}


# ---- references -------------------------------------------------------------------------------------------------------------
def results(r, T, dt=torch.float64):
    """{output name: (tensor in dtype dt, band tolerance)} -- the reference (float64) or the fp32 oracle (float32) of the
    row's entry point on the inputs T.  sumK is sums[K]."""
    op, B, C, S = r["op"], r["B"], r["C"], r["S"]
    t = lambda name: T[name].to(dt)
    R = {}
    if op in ("rs_fwd", "rs_bwd"):
        x = t("x").requires_grad_(op == "rs_bwd")
        v = x - t("y") if r["with_y"] else x
        p = pen(v, r["mode"], f32(r["q"]), f32(r["eps"]))
        w = rs_weight(r, T, dt)
        s0 = (p * w).sum() if w is not None else p.sum()
        if op == "rs_fwd":
            R["sum0"] = (s0, SUM_TOL)
            R["sum1"] = (w.sum() if w is not None else torch.zeros((), dtype=dt), SUM_TOL)
            return R
        (gx,) = torch.autograd.grad(s0, [x])
        gx = gx * t("coef")
        if "gx" in r["grads"]:
            R["gx"] = (gx, GRAD_TOL)
        if "gy" in r["grads"]:
            R["gy"] = (-gx, GRAD_TOL)
        return R
    if op in ("cen_fwd", "cen_bwd"):
        dist = olosses.census_dist if dt == torch.float32 else census_dist
        if op == "cen_fwd":
            R["dist"] = (dist(t("img1"), t("img2")), CENSUS_TOL)
            return R
        i1, i2 = t("img1").requires_grad_(), t("img2").requires_grad_()
        g1, g2 = torch.autograd.grad((dist(i1, i2) * t("gdist")).sum(), [i1, i2])
        for name, gi in (("g1", g1), ("g2", g2)):
            if name in r["grads"]:
                R[name] = (gi, GRAD_TOL)
        return R
    if op in ("ws_fwd", "ws_bwd"):
        x, y = t("x").requires_grad_(op == "ws_bwd"), t("y").requires_grad_(op == "ws_bwd")
        ld, apw = olosses.weighted_ssim(x, y, t("w"))
        s0 = (ld * apw).sum() if r["use_occ"] else ld.sum()
        if op == "ws_fwd":
            R["sum0"], R["sum1"] = (s0, SUM_TOL), (apw.sum(), SUM_TOL)
            return R
        gx, gy = torch.autograd.grad(s0, [x, y])
        for name, gi in (("gx", gx), ("gy", gy)):
            if name in r["grads"]:
                R[name] = (gi * t("coef"), GRAD_TOL)
        return R
    if op in ("mg_fwd", "mg_bwd"):
        w0, w1, m = (t(k).requires_grad_(op == "mg_bwd") for k in ("w0", "w1", "m"))
        s = torch.sigmoid(m)
        merged = w0 * s + w1 * (1 - s)  # oracle.losses.merge, with the sigmoid kept
        if op == "mg_fwd":
            R["merged"] = (merged, MERGE_TOL)
            if r["sig"]:
                R["sig"] = (s, MERGE_TOL)
            return R
        tot = (merged * t("gmerged")).sum()
        if r["gsig"]:
            tot = tot + (s * t("gsig")).sum()
        grads = torch.autograd.grad(tot, [w0, w1, m])
        for name, gi in zip(("gw0", "gw1", "gm"), grads):
            if name in r["grads"]:
                R[name] = (gi, GRAD_TOL)
        return R
    if op in ("ds_fwd", "ds_bwd", "d3_fwd", "d3_bwd"):
        for k in range(nstud(r)):
            if r["coef0"]:  # the caller has discarded the term: exactly 0, also where the flows are not finite
                R["gf%d" % k] = (torch.zeros(B, r["F"], S, dtype=dt), GRAD_TOL)
                continue
            lm = (distill_margin(t("mi%d" % k), t("mt"), t("gt")) > 0).to(dt)
            d = t("ft") - t("fi%d" % k)
            root = distill_root(t("fi%d" % k), t("ft"))
            if op.endswith("fwd"):
                R["sum%d" % k] = ((root * lm).sum(), SUM_TOL)
                if op == "ds_fwd":
                    R["sum1"] = (lm.sum(), SUM_TOL)
            else:  # d/df sqrt(mean_c d_c^2) = -d_c / (F root); 0 at root == 0 (the ABI's rule, autograd has NaN there)
                sc = torch.where(root > 0, t("coef") * lm / (r["F"] * root.clamp_min(1e-300 if dt == torch.float64 else 1e-30)),
                                 torch.zeros_like(root))
                R["gf%d" % k] = (-d * sc, GRAD_TOL)
        return R
    assert op == "prelu"
    x, gg, a = t("x"), t("g"), t("a")
    slope = a.view(1, -1, 1)
    gx = torch.where(x > 0, gg, slope * gg)
    integrand = torch.where(x > 0, torch.zeros_like(x), x * gg)
    R["gx"] = (gx, GRAD_TOL)
    R["gw"] = (integrand.sum((0, 2)) if r["nw"] == C and C > 1 else integrand.sum().view(1), GRAD_TOL)
    if r["bias"]:
        R["gb"] = (gx.sum((0, 2)), GRAD_TOL)
    return R


def exact(r, T):
    """{output name: (fp32 tensor, bool mask or None)} -- elements (all of them without a mask) the kernel must give
    exactly."""
    op, B, C, S = r["op"], r["B"], r["C"], r["S"]
    E = {}
    if op in ("rs_fwd", "rs_bwd"):
        w = rs_weight(r, T, torch.float32)
        if op == "rs_fwd":
            if w is None:
                E["sum1"] = (torch.zeros(()), None)
            elif r["wkind"] == "01":
                E["sum1"] = (w.sum(dtype=torch.float64).float(), None)
            if w is not None and not bool(w.any()):
                E["sum0"], E["sum1"] = (torch.zeros(()), None), (torch.zeros(()), None)
        elif w is not None:
            for name in r["grads"]:
                E[name] = (torch.zeros(B, C, S), (w == 0).expand(B, C, S))
        return E
    if op in ("ds_fwd", "ds_bwd", "d3_fwd", "d3_bwd"):
        for k in range(nstud(r)):
            lm = distill_margin(T["mi%d" % k].double(), T["mt"].double(), T["gt"].double()) > 0
            if op == "ds_fwd":
                E["sum1"] = (lm.sum(dtype=torch.float64).float(), None)
            elif op.endswith("bwd"):
                zero = torch.ones_like(lm) if r["coef0"] else (~lm | (distill_root(T["fi%d" % k], T["ft"]) == 0))
                E["gf%d" % k] = (torch.zeros(B, r["F"], S), zero.expand(B, r["F"], S))
        return E
    if op == "prelu":
        E["gx"] = (torch.where(T["x"] > 0, T["g"], T["a"].view(1, -1, 1) * T["g"]), None)
    return E


def numel(shape):
    return math.prod(shape)
