"""Inputs, fp64 references, fp32 oracles and bands of the rows of tests/mem_ledger.py (CPU tensors only; shared by
tests/test_mem_ledger.py and tests/test_gpu_mem_ledger.py).

Reference: oracle.warps.warp3d_ref evaluated in float64 on the fp32 input values, gradients from autograd in float64;
F.interpolate in float64 (times scale, plus prev) for the resizes; the fused entry points compose the two.

Bands (no voxel left out): warps 2e-5 x max(1, max|ref|) on outputs and 2e-4 x max(1, max|ref|) on gradients (OUT_ATOL /
GRAD_ATOL of test_gpu_warps.py), forward resizes 2e-6 x (test_upsample3d_scale_add_vs_aten), adjoints 1e-5 x
(test_interpolate3d_backward_vs_aten).

The warp's flow gradient jumps where a sample coordinate crosses an integer (and is cut to zero outside [0, n - 1]), so the
rows' flows keep every coordinate at least DELTA px away from every integer it could round across: build the flow from
the kinds test_gpu_warps._rc_flows uses, compute the three coordinates in float64 from the fp32 flow values, move every
flow component whose coordinate is within DELTA of an integer (the clamp ends included) by 2 DELTA, recompute, re-check.
Voxels pushed out of range by more than DELTA (gradient exactly zero) are mixed in.  tests/test_mem_ledger.py accepts
DELTA: the project's own fp32 oracle must stay inside the band on the same inputs."""
import math

import torch
import torch.nn.functional as F

import mem_ledger as L
from oracle import warps as owarps

DELTA = 0.05
OUT_TOL, GRAD_TOL, RESIZE_TOL, ADJ_TOL = 2e-5, 2e-4, 2e-6, 1e-5
FLOW_KINDS = ("smooth", "shift", "bigshift", "noise", "jump", "ramp")


def gen_of(r):
    return torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(L.row_id(r))) % 1000003)


def flow_ext(r):
    f = r["factor"] if r["op"].startswith("uw_") else 1
    return tuple(n * f for n in r["ext"])


def img_ext(r):
    return r["inp"] or flow_ext(r)


def _raw_flow(kind, B, D, H, W, g):
    ax = lambda n: torch.linspace(0, 6.28318, n)
    d, h, w = ax(D).view(D, 1, 1), ax(H).view(1, H, 1), ax(W).view(1, 1, W)
    smooth = torch.stack([1.5 * torch.sin(d) * torch.cos(h) + 0 * w, 1.2 * torch.cos(2 * w) + 0 * d + 0 * h,
                          0.8 * torch.sin(h) * torch.sin(w) + 0 * d], 0).expand(B, 3, D, H, W).contiguous()
    if kind == "smooth":
        return smooth
    if kind == "shift":
        f = torch.empty(B, 3, D, H, W)
        f[:, 0], f[:, 1], f[:, 2] = 2.25, -1.5, 3.75
        return f
    if kind == "bigshift":  # _rc_flows' own constant shift (on the small volumes it would put every voxel out of range)
        f = torch.empty(B, 3, D, H, W)
        f[:, 0], f[:, 1], f[:, 2] = 9.25, -6.5, 11.75
        return f
    if kind == "noise":
        return (torch.rand(B, 3, D, H, W, generator=g) * 2 - 1) * 3.0
    if kind == "jump":
        smooth[:, 1, D // 2:] += 7.0
        return smooth
    assert kind == "ramp"
    smooth[:, 1] += 2.5 * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)
    return smooth


def coords(flow, iext):
    """float64 sample coordinates (ix, iy, iz) of a [B,3,D,H,W] flow into a volume of extent iext, unclamped, and
    d(coordinate)/d(flow component)."""
    B, _, D, H, W = flow.shape
    Di, Hi, Wi = iext
    f = flow.double()
    lin = lambda n: torch.linspace(-1.0, 1.0, n, dtype=torch.float64)
    gx = lin(H).view(1, 1, H, 1) + f[:, 0] / ((Hi - 1.0) / 2.0)
    gy = lin(D).view(1, D, 1, 1) + f[:, 1] / ((Di - 1.0) / 2.0)
    gz = lin(W).view(1, 1, 1, W) + f[:, 2] / ((Wi - 1.0) / 2.0)
    c = torch.stack([(gx + 1) / 2 * (Wi - 1), (gy + 1) / 2 * (Hi - 1), (gz + 1) / 2 * (Di - 1)], 1)
    k = ((Wi - 1.0) / (Hi - 1.0), (Hi - 1.0) / (Di - 1.0), (Di - 1.0) / (Wi - 1.0))
    return c, k, (Wi - 1, Hi - 1, Di - 1)


def _near(c, top, delta):
    bad = torch.zeros_like(c, dtype=torch.bool)
    for a in range(3):
        ca = c[:, a]
        bad[:, a] = ((ca - ca.round()).abs() < delta) & (ca > -delta) & (ca < top[a] + delta)
    return bad


def keep_off_cells(flow, iext, delta=DELTA):
    """`flow` (fp32) with every sample coordinate at least `delta` from an integer it could cross."""
    flow = flow.clone()
    for _ in range(12):
        c, k, top = coords(flow, iext)
        bad = _near(c, top, delta)
        if not bad.any():
            return flow
        for a in range(3):
            flow[:, a] += torch.where(bad[:, a], torch.full_like(flow[:, a], 2 * delta / k[a]), torch.zeros_like(flow[:, a]))
    c, k, top = coords(flow, iext)
    assert not _near(c, top, delta * 0.9).any(), "flow still within delta of a cell boundary"
    return flow


def make_flow(kind, B, fext, iext, g):
    D, H, W = fext
    f = _raw_flow(kind, B, D, H, W, g)
    # a few voxels far outside the volume: the clamped gradient is exactly zero there
    # (component 1 only for white noise: the row cache follows the y0 range of a tile, and stray rows in every tile would
    # pin its window to the whole height and keep the other kinds from driving it)
    far = torch.rand(B, 3, D, H, W, generator=g) < 0.03
    if kind != "noise":
        far[:, 1] = False
    sign = torch.where(torch.rand(B, 3, D, H, W, generator=g) < 0.5, -1.0, 1.0)
    reach = torch.tensor([H + iext[1] + 3.0, D + iext[0] + 3.0, W + iext[2] + 3.0]).view(1, 3, 1, 1, 1)
    f = torch.where(far, sign * reach * 2, f)
    return keep_off_cells(f, iext)


def _up(x, factor, nd=3):
    return F.interpolate(x, scale_factor=factor, mode="trilinear" if nd == 3 else "bilinear", align_corners=False)


def _down(x, factor, nd=3):
    return F.interpolate(x, scale_factor=1.0 / factor, mode="trilinear" if nd == 3 else "bilinear", align_corners=False)


def data(r):
    """{name: fp32 CPU tensor} of the row's inputs."""
    g = gen_of(r)
    op, B, C = r["op"], r["B"], r["C"]
    T = {}
    if op in L.WARP_OPS:
        fe, ie = flow_ext(r), img_ext(r)
        npair = 2 if op in L.PAIR_OPS else 1
        T["in0"] = torch.rand(B, C, *ie, generator=g)
        if npair == 2:
            T["in1"] = torch.rand(B, C, *ie, generator=g)
        if op == "uw_fwd":
            T["delta"] = torch.randn(B, 6, *r["ext"], generator=g) * 0.6
            if r["prev"]:
                T["prev"] = torch.cat([_raw_flow(k, B, *fe, g) for k in (r["flow"] * 2)[:2]], 1)
            return T
        T["flow"] = torch.cat([make_flow(k, B, fe, ie, g) for k in (r["flow"] * 2)[:npair]], 1)
        if op in L.BWD_OPS:
            for i in range(npair):
                T["gout%d" % i] = torch.randn(B, C, *fe, generator=g)
            for i in range(r["nadd"]):
                T["add%d" % i] = torch.randn(B, 6, *fe, generator=g)
        return T
    if op in ("up_add", "down", "down_ms"):
        T["small" if op == "up_add" else "in"] = torch.randn(B, C, *r["ext"], generator=g)
        if r["prev"]:
            T["prev"] = torch.randn(B, C, *(n * r["factor"] for n in r["ext"]), generator=g)
        return T
    if op in ("ibwd", "ibwd_s", "r2_bwd"):
        oe = tuple(n * r["factor"] if r["upsample"] else n // r["factor"] for n in r["ext"])
        T["gout"] = torch.randn(B, C, *oe, generator=g)
        return T
    assert op == "r2_fwd"
    T["in"] = torch.randn(B, C, *r["ext"], generator=g)
    return T


def _warp_grads(r, T, dt):
    """d(sum_i <warp(in_i, flow_i), gout_i>) / d(flow), d / d(in_i) in dtype dt."""
    npair = 2 if r["op"] in L.PAIR_OPS else 1
    flow = T["flow"].to(dt).requires_grad_()
    ins = [T["in%d" % i].to(dt).requires_grad_() for i in range(npair)]
    tot = 0
    for i in range(npair):
        tot = tot + (owarps.warp3d_ref(ins[i], flow[:, 3 * i:3 * i + 3]) * T["gout%d" % i].to(dt)).sum()
    grads = torch.autograd.grad(tot, [flow] + ins)
    return grads[0], grads[1:]


def results(r, T, dt=torch.float64):
    """{output name: (tensor in dtype dt, band tolerance)} -- the reference (float64) or the project's fp32 oracle
    (float32) of the row's entry point on the inputs T."""
    op, f = r["op"], r["factor"]
    R = {}
    if op in ("w_fwd", "wp_fwd"):
        for i in range(2 if op == "wp_fwd" else 1):
            R["out%d" % i] = (owarps.warp3d_ref(T["in%d" % i].to(dt), T["flow"][:, 3 * i:3 * i + 3].to(dt)), OUT_TOL)
        return R
    if op == "uw_fwd":
        fo = _up(T["delta"].to(dt), f) * r["scale"]
        if r["prev"]:
            fo = T["prev"].to(dt) + fo
        R["fout"] = (fo, OUT_TOL)
        for i in range(2):
            R["out%d" % i] = (owarps.warp3d_ref(T["in%d" % i].to(dt), fo[:, 3 * i:3 * i + 3]), OUT_TOL)
        return R
    if op in L.BWD_OPS:
        gf, gins = _warp_grads(r, T, dt)
        for i in range(r["nadd"]):
            gf = gf + T["add%d" % i].to(dt)
        if r["with_grad_flow"]:
            R["gflow"] = (gf, GRAD_TOL)
        if r["with_grad_in"]:
            for i, gi in enumerate(gins):
                R["gin%d" % i] = (gi, GRAD_TOL)
        if op.startswith("uw_"):
            small = torch.zeros(r["B"], 6, *r["ext"], dtype=dt, requires_grad=True)
            (gd,) = torch.autograd.grad((_up(small, f) * gf).sum(), [small])
            R["gdelta"] = (gd * r["scale"], GRAD_TOL)
        return R
    if op == "up_add":
        o = _up(T["small"].to(dt), f) * r["scale"]
        R["out"] = ((T["prev"].to(dt) + o) if r["prev"] else o, RESIZE_TOL)
        return R
    if op in ("down", "down_ms"):
        R["out"] = (_down(T["in"].to(dt), f) * r["scale"], RESIZE_TOL)
        return R
    if op == "r2_fwd":
        x = T["in"].to(dt)
        R["out"] = ((_up(x, f, 2) if r["upsample"] else _down(x, f, 2)) * r["scale"], RESIZE_TOL)
        return R
    assert op in ("ibwd", "ibwd_s", "r2_bwd")
    nd = 2 if op == "r2_bwd" else 3
    x = torch.zeros(r["B"], r["C"], *r["ext"], dtype=dt, requires_grad=True)
    y = _up(x, f, nd) if r["upsample"] else _down(x, f, nd)
    (gi,) = torch.autograd.grad((y * T["gout"].to(dt)).sum(), [x])
    R["gin"] = (gi * r["scale"], ADJ_TOL)
    return R


def band(ref, tol):
    return tol * max(1.0, float(ref.abs().max()))


def ws_floats(r):
    """Floats of workspace the header asks for (0: none passed)."""
    f, B = r["factor"], r["B"]
    if r["op"] in ("uw_bwd", "uw_bwd3"):
        Ds, Hs, Ws = r["ext"]
        return B * 6 * (Ds * f * Hs * f * Ws + Ds * f * Hs * Ws)
    if r["op"] in ("ibwd", "ibwd_s") and r["with_ws"]:
        Di, Hi, Wi = r["ext"]
        return B * r["C"] * (Di * f * Hi * f * Wi + Di * f * Hi * Wi)
    return 0


def numel(shape):
    return math.prod(shape)
