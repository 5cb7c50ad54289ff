"""Inputs, fp64 references, fp32 oracles, bands, margins, decisions and exact expectations of the rows of
tests/w2lap_ledger.py (CPU tensors only; shared by tests/test_w2lap_ledger.py and tests/test_gpu_w2lap_ledger.py).

Warps.  Reference: oracle/warps.py evaluated in float64 on the fp32 input values, gradients from autograd in float64; the
fp32 oracle is the same code in float32.  Bands (no pixel left out): 2e-5 x max(1, max|ref|) on outputs, 2e-4 x
max(1, max|ref|) on gradients, grad_flow (a sum over C) times max(1, C / 8) -- OUT_ATOL / GRAD_ATOL of test_gpu_warps.py.
Unmasked rows keep every sample coordinate at least delta px from every integer it could cross (the clamp ends and the
first corner outside included): build the flow from its kind, compute the coordinates in float64 from the fp32 flow
values, move every component whose coordinate is within delta of such an integer by 2 delta, recompute, re-check.  delta
is 0.05, and 0.25 on the one row 131071 px wide, where the fp32 chain itself is off by ~0.02 px.  A few samples far
outside are mixed in.  Masked rows are "dyadic" (tests/w2lap_ledger.py); `chain` restates w2_sample + w2_mask op for op
in a dtype of choice, and tests/test_w2lap_ledger.py requires its fp32 and fp64 decisions (floor, corner validity, clamp
multiplier, mask) to be equal at every pixel of every row.

Occlusion check.  Reference: oracle.warps.occ_check_ref in float64.  The outputs are 0/1 and compared for equality, so the
inputs keep |lhs - thresh| >= OCC_MARGIN and every outgoing position >= OCC_MARGIN from 0 and n - 1 (offending pixels
get their flow moved by a few margins, then everything is re-checked); the "integer" row lands exactly on 0 and n - 1.

Laplacian pyramids.  `pyramid` is a separable restatement of oracle/ifnet_ref.lap_loss / lap_loss3d in a dtype of choice
(the CPU test holds it to those).  Forward rows take the first seed from the row's base seed for which every pyramid entry
has |lap| >= the row's margin in float64; loss is held to 2e-6 x max(1, |ref|) and sgn to sign(lap64) x
float(1 / float(numel_l)) bit for bit.  Backward rows feed O(1) noise as `sgn` (the entry point is linear in it) and
compare with the float64 adjoint of the pyramid map at 1e-5 x max(1, max|ref|)."""
import math

import torch

import w2lap_ledger as L
from oracle import warps as owarps

DELTA, DELTA_WIDE = 0.05, 0.25
OUT_TOL, GRAD_TOL, LOSS_TOL, ADJ_TOL = 2e-5, 2e-4, 2e-6, 1e-5
OCC_MARGIN = 2e-4
ALPHA1, ALPHA2S = 0.1, 0.5
FLOW_KINDS = ("smooth", "shift", "noise", "wide", "small", "dyadic", "occ", "integer")
SEEDS = 200  # seeds a forward pyramid row may try


def base_seed(r):
    return sum((i + 1) * ord(c) for i, c in enumerate(L.row_id(r))) % 1000003


def gen_of(r, k=0):
    return torch.Generator().manual_seed(base_seed(r) + k)


def img_ext(r):
    return r["inp"] or r["ext"]


def numel(shape):
    return math.prod(shape)


def delta_of(r):
    return DELTA_WIDE if max(r["ext"] + img_ext(r)) > 20000 else DELTA


def band(ref, tol):
    return tol * max(1.0, float(ref.abs().max()))


# ---- warps: flows ---------------------------------------------------------------------------------------------------
def _raw_flow(kind, B, H, W, g):
    if kind in ("smooth", "occ"):
        h = torch.linspace(0, 6.28318, H).view(H, 1)
        w = torch.linspace(0, 6.28318, W).view(1, W)
        return torch.stack([1.5 * torch.sin(h) * torch.cos(w), 1.2 * torch.cos(2 * w) + 0.8 * torch.sin(h)], 0).expand(
            B, 2, H, W).contiguous()
    if kind == "shift":
        f = torch.empty(B, 2, H, W)
        f[:, 0], f[:, 1] = 2.25, -1.5
        return f
    amp = {"noise": 3.0, "wide": 6.0, "small": 0.9}[kind]
    return (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * amp


def coords(r, flow, start=None):
    """float64 sample coordinates [B,2,H,W] (x, y) of a [B,2,H,W] flow, unclamped, d(coordinate)/d(flow component) and
    the last index per axis."""
    H, W = r["ext"]
    Hi, Wi = img_ext(r)
    f = flow.double()
    out, ks = [], []
    for a, (n, ni) in enumerate(((W, Wi), (H, Hi))):
        i = torch.arange(n, dtype=torch.float64).view((1, 1, n) if a == 0 else (1, n, 1))
        u = f[:, a]
        if r["mode"] == L.RIFE:
            lin = torch.linspace(-1.0, 1.0, n, dtype=torch.float64).view(i.shape)
            c, k = (lin + u / ((ni - 1.0) / 2.0) + 1) / 2 * (ni - 1), 1.0
        elif r["mode"] == L.PWC:
            d = max(n - 1, 1)
            c, k = (i + u) * n / d - 0.5, n / d
        elif r["mode"] == L.PHOTO:
            fw = float(torch.tensor(2.0 / n, dtype=torch.float32))
            c, k = (i + u) * fw * n / 2 - 0.5, fw * n / 2
        else:
            s = start.double()[:, a].view(-1, 1, 1) if start is not None else 0.0
            c, k = (i + s) + u, 1.0
        out.append(c)
        ks.append(k)
    return torch.stack(out, 1), ks, (Wi - 1, Hi - 1)


def _near(c, top, delta):
    bad = torch.zeros_like(c, dtype=torch.bool)
    for a in range(2):
        ca = c[:, a]
        bad[:, a] = ((ca - ca.round()).abs() < delta) & (ca > -1 - delta) & (ca < top[a] + 1 + delta)
    return bad


def keep_off_cells(r, flow, start, delta):
    flow = flow.clone()
    for _ in range(12):
        c, k, top = coords(r, flow, start)
        bad = _near(c, top, delta)
        if not bad.any():
            return flow
        for a in range(2):
            flow[:, a] += torch.where(bad[:, a], torch.full_like(flow[:, a], 2 * delta / k[a]), torch.zeros_like(flow[:, a]))
    return flow  # (the CPU test re-checks the margin on every row)


def cell_margin(r, flow, start):
    """The smallest distance of a sample coordinate from an integer it could cross."""
    c, _, top = coords(r, flow, start)
    d = (c - c.round()).abs()
    for a in range(2):
        inside = (c[:, a] > -1.5) & (c[:, a] < top[a] + 1.5)
        d[:, a] = torch.where(inside, d[:, a], torch.ones_like(d[:, a]))
    return float(d.min())


def dyadic_flow(B, H, W, g):
    """Odd multiples of 1/8, |flow| below min(H, W) / 4 px (at least 3/8; 191/8 at most, on the 65 x 257 rows, whose mask
    would be 1 nearly everywhere with flows below 5 px)."""
    m = int(max(2, min(96, min(H, W) * 3 // 2 if min(H, W) > 33 else min(H, W))))  # k in [-m, m): |2k + 1| / 8 <= (2m - 1) / 8
    k = torch.randint(-m, m, (B, 2, H, W), generator=g)
    return (2 * k + 1).float() / 8.0


def make_flow(r, start, g):
    B, (H, W) = r["B"], r["ext"]
    if r["flow"] == "dyadic":
        return dyadic_flow(B, H, W, g)
    f = _raw_flow(r["flow"], B, H, W, g)
    # a few samples far outside: every corner out of range.  (Not for DILATED: its weights are taken against the clamped
    # corners, (edge - x) and (x - edge), and cancel only in exact arithmetic -- at |x| of a few hundred px the fp32
    # oracle itself leaves the gradient band of grad_in.)
    if r["flow"] in ("smooth", "shift", "noise") and r["mode"] != L.DILATED:
        far = torch.rand(B, 2, H, W, generator=g) < 0.03
        sign = torch.where(torch.rand(B, 2, H, W, generator=g) < 0.5, -1.0, 1.0)
        Hi, Wi = img_ext(r)
        reach = torch.tensor([W + Wi + 3.0, H + Hi + 3.0]).view(1, 2, 1, 1)
        f = torch.where(far, sign * reach * 2, f)
    return keep_off_cells(r, f, start, delta_of(r))


def make_image(B, C, Hi, Wi, g):
    """White noise in [0, 1) up to 65 px; above, a smooth wave (3 and 2 periods) with a phase per plane, windowed to zero
    at the ends of every axis longer than 65."""
    if max(Hi, Wi) <= 65:
        return torch.rand(B, C, Hi, Wi, generator=g)
    p = torch.rand(2, B, C, 1, 1, generator=g)
    x = torch.linspace(0, 1, Wi).view(1, 1, 1, Wi)
    y = torch.linspace(0, 1, Hi).view(1, 1, Hi, 1)
    img = 0.5 + 0.5 * torch.sin(6.28318 * (3 * x + p[0])) * torch.cos(6.28318 * (2 * y + p[1]))
    # (zeros padding makes the image's edge a step: a window takes the long axes to ~0 there, so that the slope stays
    # small across the border as well)
    for n, shape in ((Wi, (1, 1, 1, Wi)), (Hi, (1, 1, Hi, 1))):
        if n > 65:
            img = img * torch.sin(3.14159265 * (torch.arange(n, dtype=torch.float32) + 0.5) / n).view(shape)
    return img


# ---- warps: the kernel's sampling chain, op for op, in a dtype of choice ------------------------------------------------
def chain(r, flow, start, dt):
    """w2_sample<MODE> + w2_mask restated with torch ops in dtype dt (no contraction): dict of the decisions (floor_x,
    floor_y, valid = the four corner flags, clip = RIFE's gradient multipliers, mask, msum = the in-bounds weight sum)."""
    H, W = r["ext"]
    Hi, Wi = img_ext(r)
    c = lambda v: torch.tensor(float(v), dtype=dt)
    f = flow.to(dt)
    res = {}
    ixy, clip = [], []
    for a, (n, ni) in enumerate(((W, Wi), (H, Hi))):
        ii = torch.arange(n).view((1, 1, n) if a == 0 else (1, n, 1))
        i = ii.to(dt)
        u = f[:, a]
        if r["mode"] == L.RIFE:
            step = c(2) / c(n - 1)
            s = (c(ni) - c(1)) / c(2)
            lin = torch.where(ii < n // 2, c(-1) + step * i, c(1) - step * (c(n - 1) - i))
            gx = lin + u / s
            x = ((gx + c(1)) / c(2)) * c(ni - 1)
            clip.append(((x > 0) & (x < ni - 1)).to(dt))
            x = x.clamp(0, ni - 1)
        elif r["mode"] == L.PWC:
            vx = c(2) * (i + u) / c(max(n - 1, 1)) - c(1)
            x = ((vx + c(1)) * c(n) - c(1)) / c(2)
        elif r["mode"] == L.PHOTO:
            fw = torch.tensor(2.0 / n, dtype=torch.float32).to(dt)
            gx = (u + i) * fw - c(1)
            x = ((gx + c(1)) * c(n) - c(1)) / c(2)
        else:
            s = start.to(dt)[:, a].view(-1, 1, 1) if start is not None else c(0)
            x = (i + s) + u
        ixy.append(x.expand(f.shape[0], H, W))
    fl = [torch.floor(x.clamp(-2, ni + 1)) for x, ni in zip(ixy, (Wi, Hi))]
    # (beyond -1 and n every corner is out of range, or clamps to the same edge pixel, whatever the floor)
    res["floor_x"], res["floor_y"] = fl[0].long().clamp(-1, Wi), fl[1].long().clamp(-1, Hi)
    if clip:
        res["clip"] = torch.stack([k.expand(f.shape[0], H, W) for k in clip], 0)
    if r["mode"] != L.DILATED:
        ok = [[(fl[a] + d >= 0) & (fl[a] + d < ni) for d in (0, 1)] for a, ni in enumerate((Wi, Hi))]
        v00, v10, v01, v11 = ok[0][0] & ok[1][0], ok[0][1] & ok[1][0], ok[0][0] & ok[1][1], ok[0][1] & ok[1][1]
        res["valid"] = torch.stack([v00, v10, v01, v11], 0)
        if r["mask"]:
            ax, bx = ixy[0] - fl[0], (fl[0] + 1) - ixy[0]
            ay, by = ixy[1] - fl[1], (fl[1] + 1) - ixy[1]
            z = torch.zeros_like(ax)
            m = torch.where(v00, bx * by, z)
            m = m + torch.where(v10, ax * by, z)
            m = m + torch.where(v01, bx * ay, z)
            m = m + torch.where(v11, ax * ay, z)
            res["msum"] = m
            res["mask"] = m >= 1
            res["interior"] = v00 & v10 & v01 & v11
    return res


# ---- occlusion check --------------------------------------------------------------------------------------------------
_occ_cache = {}


def occ_terms(r, T, dt):
    """(lhs_f, lhs_b, thresh, positions [2 flows][2 axes]) in dtype dt; None for the first three in mode OUT."""
    key = (L.row_id(r), dt, T["flow_f"].data_ptr())
    if key not in _occ_cache:
        _occ_cache.clear()
        f, b = T["flow_f"].to(dt), T["flow_b"].to(dt)
        H, W = r["ext"]
        xs = torch.arange(W).to(dt).view(1, 1, W)
        ys = torch.arange(H).to(dt).view(1, H, 1)
        pos = [[xs + t[:, 0], ys + t[:, 1]] for t in (f, b)]
        lhs = (None, None, None) if r["mode"] == L.OCC_OUT else owarps.occ_fb_lhs_thresh(f, b, ALPHA1, ALPHA2S)
        _occ_cache[key] = (*lhs, pos)
    return _occ_cache[key]


def _occ_margins(r, T):
    """[(what, boolean tensor of offenders at `slack` x OCC_MARGIN)] in float64."""
    lf, lb, th, pos = occ_terms(r, T, torch.float64)
    H, W = r["ext"]
    out = {}
    for name, p in zip(("flow_f", "flow_b"), pos):
        out[name + ".pos"] = [torch.minimum(p[a].abs(), (p[a] - top).abs()) for a, top in enumerate((W - 1, H - 1))]
    if lf is not None:
        out["flow_f.lhs"], out["flow_b.lhs"] = (lf - th).abs()[:, 0], (lb - th).abs()[:, 0]
    return out


def make_occ_flows(r, g):
    B, (H, W) = r["B"], r["ext"]
    if r["flow"] == "integer":
        T = {}
        for name in ("flow_f", "flow_b"):
            x = torch.arange(W).view(1, 1, W).expand(B, H, W)
            y = torch.arange(H).view(1, H, 1).expand(B, H, W)
            kind = torch.randint(0, 6, (2, B, H, W), generator=g)
            stay = [torch.randint(0, n, (B, H, W), generator=g) for n in (W, H)]
            fl = []
            for a, (i, n) in enumerate(((x, W), (y, H))):
                k = kind[a]
                tgt = torch.where(k == 0, torch.zeros_like(i), torch.where(k == 1, torch.full_like(i, n - 1), torch.where(
                    k == 2, torch.full_like(i, -1), torch.where(k == 3, torch.full_like(i, n), stay[a]))))
                fl.append((tgt - i).float())
            T[name] = torch.stack(fl, 1)
        return T
    f = _raw_flow("occ", B, H, W, g)
    h = torch.linspace(0, 6.28318, H).view(H, 1)
    w = torch.linspace(0, 6.28318, W).view(1, W)
    if max(H, W) <= 65:  # (white noise only where the fp32 coordinate error times its slope stays far below the margin)
        b = -f + torch.stack([0.9 * torch.sin(h + 1.0) * torch.sin(2 * w), 0.6 * torch.cos(h) * torch.cos(w + 0.5)], 0)
        f = f + (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 0.4
        b = b + (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 0.4
    else:  # the long rows: consistent flows, and 1.5 px of disagreement on every other 256-px block -- lhs is then far
        # from thresh except where a sample straddles a block edge, and the repair below is done in a few passes
        blocks = ((torch.arange(H).view(H, 1) // 256 + torch.arange(W).view(1, W) // 256) % 2).float()
        b = -f + torch.stack([1.5 * blocks, torch.zeros(H, W)], 0)
    T = {"flow_f": f.contiguous(), "flow_b": b.contiguous()}
    for it in range(10):
        clean = True
        for what, d in _occ_margins(r, T).items():
            name, kind = what.split(".")
            if kind == "pos":
                for a in range(2):
                    bad = d[a] < 1.5 * OCC_MARGIN
                    if bad.any():
                        clean = False
                        T[name][:, a] += torch.where(bad, 4 * OCC_MARGIN, 0.0)
            else:
                bad = d < 1.5 * OCC_MARGIN
                if bad.any():
                    clean = False
                    T[name][:, it % 2] += torch.where(bad, (4 + 2 * it) * OCC_MARGIN, 0.0)
        if clean:
            break
        T = {k: t.clone() for k, t in T.items()}  # (new storage: the cache keys on it)
    return T


# ---- Laplacian pyramids -------------------------------------------------------------------------------------------------
_G = (1.0 / 16, 4.0 / 16, 6.0 / 16, 4.0 / 16, 1.0 / 16)


def _blur(x, ax):
    n = x.shape[ax]
    idx = torch.arange(-2, n + 2).abs()
    idx = torch.where(idx >= n, 2 * n - 2 - idx, idx)
    xp = x.index_select(ax, idx)
    out = _G[0] * xp.narrow(ax, 0, n)
    for i in range(1, 5):
        out = out + _G[i] * xp.narrow(ax, i, n)
    return out


def pyramid(x, levels):
    """[lap_0 .. lap_{levels-1}] of x [N, *ext] (2-D or 3-D), Flow-2D/model/laplacian.py:49-74 with separable filters."""
    nd = x.dim() - 1
    ev = (slice(None),) + (slice(None, None, 2),) * nd
    cur, out = x, []
    for _ in range(levels):
        d = cur
        for ax in range(1, nd + 1):
            d = _blur(d, ax)
        d = d[ev]
        z = d.new_zeros((d.shape[0],) + tuple(2 * n for n in d.shape[1:]))
        z[ev] = d
        for ax in range(1, nd + 1):
            z = _blur(z, ax)
        up = (z * float(2 ** nd))[(slice(None),) + tuple(slice(0, n) for n in cur.shape[1:])]
        out.append(cur - up)
        cur = d
    return out


def lap_sizes(r):
    """(extents per level incl. the last down, sgn floats, ws_fwd floats, ws_bwd floats) as make_dims computes them."""
    N, ext = r["B"], tuple(r["ext"])
    cap = 512 if len(ext) == 2 else 1024
    exts, sgn, down, blk = [ext], 0, 0, 0
    for _ in range(r["levels"]):
        n = N * numel(ext)
        sgn += n
        blk += min((n + 255) // 256, cap)
        ext = tuple((e + 1) // 2 for e in ext)
        exts.append(ext)
        down += N * numel(ext)
    return exts, sgn, down + 2 * blk, down


def inv_numel(n):
    """float(1 / float(n)) as the entry points compute it."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32))


def _lap_inputs(r, g):
    N, ext = r["B"], r["ext"]
    T = {}
    if r["data"] == "cb":
        par = sum(torch.arange(n).view((1,) + tuple(n if j == i else 1 for j in range(len(ext)))) for i, n in enumerate(ext))
        T["input"] = (1.0 - 2.0 * (par % 2).float()).expand(N, *ext) + 0.1 * torch.randn(N, *ext, generator=g)
        if r["target"]:
            T["target"] = 0.1 * torch.randn(N, *ext, generator=g)
    else:
        T["input"] = torch.randn(N, *ext, generator=g)
        if r["data"] == "same":
            T["target"] = T["input"].clone()
        elif r["target"]:
            T["target"] = torch.randn(N, *ext, generator=g)
    if r["spike"]:
        T["input"].view(-1)[-1] += 100.0
    return T


def lap_diff(T, dt):
    return T["input"].to(dt) - T["target"].to(dt) if "target" in T else T["input"].to(dt)


_lap_cache = {}


def lap_of(r, T, dt):
    key = (L.row_id(r), dt, T["input"].data_ptr())
    if key not in _lap_cache:
        _lap_cache.clear()
        _lap_cache[key] = pyramid(lap_diff(T, dt), r["levels"])
    return _lap_cache[key]


# ---- inputs -----------------------------------------------------------------------------------------------------------
def data(r):
    """{name: fp32 CPU tensor} of the row's inputs."""
    g = gen_of(r)
    op, B, C = r["op"], r["B"], r["C"]
    if op in L.WARP_OPS:
        npair = 2 if op in L.PAIR_OPS else 1
        Hi, Wi = img_ext(r)
        T = {}
        for i in range(npair):
            T["in%d" % i] = make_image(B, C, Hi, Wi, g)
        if r["start"]:
            T["start"] = (torch.rand(B, 2, generator=g) * 2 - 1) * 1.5
        T["flow"] = torch.cat([make_flow(r, T.get("start"), g) for _ in range(npair)], 1)
        if op in L.BWD_OPS:
            for i in range(npair):
                T["gout%d" % i] = torch.randn(B, C, *r["ext"], generator=g)
        return T
    if op == "occ":
        return make_occ_flows(r, g)
    if op.endswith("bwd"):
        return {"sgn": torch.randn(lap_sizes(r)[1], generator=g), "gl": torch.tensor([r["gl"]])}
    if r["data"] == "same":
        return _lap_inputs(r, g)
    for k in range(SEEDS):
        T = _lap_inputs(r, gen_of(r, k))
        if min(float(p.abs().min()) for p in lap_of(r, T, torch.float64)) >= r["margin"]:
            return T
    raise AssertionError("no seed keeps |lap| >= %g: %s" % (r["margin"], L.row_id(r)))


# ---- references ---------------------------------------------------------------------------------------------------------
def _warp(r, img, flow, start):
    if r["mode"] == L.RIFE:
        return owarps.warp2d_rife_ref(img, flow)
    if r["mode"] == L.PWC:
        return owarps.warp2d_pwc_ref(img, flow, bool(r["mask"]))
    if r["mode"] == L.PHOTO:
        return owarps.warp2d_photo_ref(img, flow)
    return owarps.warp2d_dilated_ref(img, flow, None if start is None else start.view(-1, 2, 1, 1))


def results(r, T, dt=torch.float64):
    """{output name: (tensor, band tolerance or None)} -- the reference (float64) or the project's fp32 oracle (float32)
    of the row's entry point on the inputs T.  Tolerance None: an exact expectation, compared for equality."""
    op = r["op"]
    R = {}
    if op in L.WARP_OPS:
        npair = 2 if op in L.PAIR_OPS else 1
        start = T["start"].to(dt) if "start" in T else None
        if op in ("w_fwd", "wp_fwd"):
            for i in range(npair):
                R["out%d" % i] = (_warp(r, T["in%d" % i].to(dt), T["flow"][:, 2 * i:2 * i + 2].to(dt), start), OUT_TOL)
            return R
        flow = T["flow"].to(dt).requires_grad_()
        ins = [T["in%d" % i].to(dt).requires_grad_() for i in range(npair)]
        tot = 0
        for i in range(npair):
            tot = tot + (_warp(r, ins[i], flow[:, 2 * i:2 * i + 2], start) * T["gout%d" % i].to(dt)).sum()
        grads = torch.autograd.grad(tot, [flow] + ins)
        if r["gflow"]:
            R["gflow"] = (grads[0], GRAD_TOL * max(1.0, r["C"] / 8.0))
        if r["gin"]:
            if r["alias"]:
                R["gin0"] = (grads[1] + grads[2], GRAD_TOL)
            else:
                for i in range(npair):
                    R["gin%d" % i] = (grads[1 + i], GRAD_TOL)
        return R
    if op == "occ":
        if r["flow"] == "integer":
            H, W = r["ext"]
            for name, out in (("flow_f", "occ_f"), ("flow_b", "occ_b")):
                t = T[name].long()
                px = torch.arange(W).view(1, 1, W) + t[:, 0]
                py = torch.arange(H).view(1, H, 1) + t[:, 1]
                R[out] = ((~((px > W - 1) | (px < 0) | (py > H - 1) | (py < 0))).to(dt).unsqueeze(1), None)
            return R
        lf, lb, th, pos = occ_terms(r, T, dt)
        H, W = r["ext"]
        outg = [(~((p[0] > W - 1) | (p[0] < 0) | (p[1] > H - 1) | (p[1] < 0))).unsqueeze(1) for p in pos]
        for i, (name, lhs) in enumerate((("occ_f", lf), ("occ_b", lb))):
            if r["mode"] == L.OCC_OUT:
                o = outg[i]
            elif r["mode"] == L.OCC_ALL:
                o = lhs < th
            else:
                o = (lhs < th) | ~outg[i]
            R[name] = (o.to(dt), None)
        return R
    exts, sgn_n = lap_sizes(r)[:2]
    N = r["B"]
    if op.endswith("fwd"):
        laps = lap_of(r, T, dt)
        R["loss"] = (sum(p.abs().mean() for p in laps).reshape(1), None if r["data"] == "same" else LOSS_TOL)
        R["sgn"] = (torch.cat([(torch.sign(p) * inv_numel(p.numel())).float().reshape(-1) for p in laps]), None)
        return R
    x = torch.zeros(N, *r["ext"], dtype=dt, requires_grad=True)
    sg, o, tot = T["sgn"].to(dt), 0, 0
    for p in pyramid(x, r["levels"]):
        tot = tot + (p * sg[o:o + p.numel()].view(p.shape)).sum()
        o += p.numel()
    (gd,) = torch.autograd.grad(tot, [x])
    R["gdiff"] = (gd * r["gl"], ADJ_TOL)
    return R


# ---- what the CPU test asserts about the inputs -------------------------------------------------------------------------
def margins(r, T):
    """[(what, distance, promised)]"""
    op = r["op"]
    out = []
    if op in L.WARP_OPS and not r["mask"]:
        for i in range(2 if op in L.PAIR_OPS else 1):
            out.append(("cell margin, member %d" % i, cell_margin(r, T["flow"][:, 2 * i:2 * i + 2], T.get("start")),
                        0.9 * delta_of(r)))
    elif op == "occ" and r["flow"] != "integer":
        for what, d in _occ_margins(r, T).items():
            out.append((what, min(float(t.min()) for t in d) if isinstance(d, list) else float(d.min()), OCC_MARGIN))
    elif op in ("l2_fwd", "l3_fwd") and r["data"] != "same":
        l64, l32 = lap_of(r, T, torch.float64), pyramid(lap_diff(T, torch.float32), r["levels"])
        out.append(("|lap|", min(float(p.abs().min()) for p in l64), r["margin"]))
        worst = max(float((a.double() - b).abs().max()) for a, b in zip(l32, l64))
        out.append(("margin over 8 x the fp32 oracle's error of lap (%.3g)" % worst, r["margin"], 8 * worst))
    return out


def decisions(r, T, dt):
    op = r["op"]
    if op in L.WARP_OPS:
        D = {}
        for i in range(2 if op in L.PAIR_OPS else 1):
            for k, v in chain(r, T["flow"][:, 2 * i:2 * i + 2], T.get("start"), dt).items():
                if k != "msum":
                    D["%s.%d" % (k, i)] = v
        return D
    if op == "occ":
        return {k: v for k, (v, _) in results(r, T, dt).items()} if r["flow"] != "integer" else {}
    if op.endswith("fwd"):
        return {"sign": torch.cat([torch.sign(p).reshape(-1).to(torch.int8) for p in lap_of(r, T, dt)])}
    return {}


def dropped_second_trip(r, T):
    """Forward pyramid rows with a spike: (the loss without the last element's term, the loss, its band)."""
    laps = lap_of(r, T, torch.float64)
    loss = sum(p.abs().mean() for p in laps)
    short = loss - laps[0].reshape(-1)[-1].abs() / laps[0].numel()
    return float(short), float(loss), band(loss, LOSS_TOL)


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------
def predict(r):
    """(kernels, (NC, CG) or None) launch_fwd / launch_bwd must pick for a warp row."""
    B, C, (H, W) = r["B"], r["C"], r["ext"]
    Hi, Wi = img_ext(r)
    n = B * H * W
    sl = 1 if (n >= 131072 or C < 4) else (4 if (n * 4 >= 131072 or C < 16) else 16)
    if r["op"] in ("w_fwd", "wp_fwd"):
        return (L.FWD(r["mode"], r["mask"], sl),), None
    plane = Hi * Wi * 4
    if r["gin"] and not r["alias"] and plane <= 48 * 1024:
        nc = max(1, min(48 * 1024 // plane, C * B // 512, C))
        ks = ((L.BWD(r["mode"], r["mask"], 0, sl),) if r["gflow"] else ()) + (L.PLANE(r["mode"], r["mask"]),)
        return ks, (nc, (C + nc - 1) // nc)
    return (L.BWD(r["mode"], r["mask"], 1 if r["gin"] else 0, sl),), None
