"""The flow-side unsupervised terms of Flow-3D at 2 x 256^3: ops.census3d_dist (r = 1, 2, 3) and ops.flow_smooth3d,
forward and backward, against the stock formulation of the same arithmetic in torch ops on the same GPU.  Times are HIP
events around `iters` calls after `warmup` calls, the two alternating per case (the stock census runs fewer
iterations: one call takes seconds at r = 3; its backward is taken tap by tap, the whole graph of 343 taps would not
fit the card).  Beside each time, the floor it is held against:
  census r >= 2   taps x 20 lane-cycles (2 v_rsq, 1 v_rcp, ~8 FMAs: an estimate from the instruction mix) over the
                  vector rate, 256 CUs x 128 lanes x 2.4 GHz
  census r = 1, smoothness   the algorithmic bytes over the 8 TB/s HBM peak (AMD's MI355X spec), with a same-call
                  `copy_` of 403 MB for what a plain stream reaches on this box today.

With --step: one Flow-3D training step (eager, 2 x 256^3) without the terms, with all three at r = 1 and at r = 3.

    python scripts/unsup3dbench.py [--step] [--size 256] [--out profiles/unsup3dbench.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402

HBM_BPS = 8.0e12
LANE_CYCLES_PER_S = 256 * 128 * 2.4e9
TAP_LANE_CYCLES = 20


def _tap(n1, c1, n2, c2):
    u1, u2 = n1 - c1, n2 - c2
    t1, t2 = u1 * torch.rsqrt(0.81 + u1 * u1), u2 * torch.rsqrt(0.81 + u2 * u2)
    d = (t1 - t2) ** 2
    return d / (0.1 + d)


def _taps(shape, r):
    D, H, W = shape[2:]
    for dz in range(2 * r + 1):
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                yield (slice(None), slice(None), slice(dz, dz + D), slice(dy, dy + H), slice(dx, dx + W))


def torch_census_fwd(v1, v2, r):
    with torch.no_grad():
        p1, p2 = F.pad(v1, [r] * 6), F.pad(v2, [r] * 6)
        dist = torch.zeros_like(v1)
        for s in _taps(v1.shape, r):
            dist += _tap(p1[s], v1, p2[s], v2)
    return dist


def torch_census_bwd(v1, v2, G, r):
    a, b = v1.detach().requires_grad_(), v2.detach().requires_grad_()
    p1, p2 = F.pad(a, [r] * 6), F.pad(b, [r] * 6)
    g1, g2 = torch.zeros_like(v1), torch.zeros_like(v2)
    for s in _taps(v1.shape, r):  # tap by tap: the intermediates of one tap are alive at a time
        ga, gb = torch.autograd.grad((_tap(p1[s], a, p2[s], b) * G).sum(), [a, b], retain_graph=True)
        g1 += ga
        g2 += gb
    return g1, g2


def torch_smooth(flow, guide, q, eps, kappa):
    s1, n = 0, 0
    for ax in (2, 3, 4):
        m = flow.shape[ax] - 1
        pen = ((flow.narrow(ax, 1, m) - flow.narrow(ax, 0, m)) ** 2 + eps ** 2).pow(q)
        if kappa:
            pen = pen * torch.exp(-kappa * (guide.narrow(ax, 1, m) - guide.narrow(ax, 0, m)).abs())
        s1 = s1 + pen.sum()
        n += pen.numel()
    return s1 / n


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternating(hip, stock, warmup, iters, stock_iters):
    ms = timed(hip, warmup, iters)
    ms_t = timed(stock, 1, stock_iters)
    ms = min(ms, timed(hip, 1, iters))
    ms_t = min(ms_t, timed(stock, 0, stock_iters))
    return ms, ms_t


def relerr(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


def row(name, ms, ms_t, floor_ms, bound, err):
    r = {"case": name, "hip_ms": ms, "torch_ms": ms_t, "speedup_vs_torch": ms_t / ms, "floor_ms": floor_ms,
         "floor": bound, "share_of_floor": floor_ms / ms, "max_deviation_from_torch": err}
    print("%-28s HIP %8.3f ms  torch %10.3f ms  x%7.1f  floor %6.3f ms (%s): %.2f of it  dev %.1e" % (
        name, ms, ms_t, ms_t / ms, floor_ms, bound, floor_ms / ms, err), flush=True)
    return r


def census_cases(S, warmup, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    v1 = torch.rand(2, 1, S, S, S, device="cuda", generator=g)
    v2 = (v1 + 0.05 * torch.randn(v1.shape, device="cuda", generator=g)).clamp(0, 1)
    G = torch.randn(v1.shape, device="cuda", generator=g)
    rows = []
    for r in (1, 2, 3):
        taps, n = (2 * r + 1) ** 3, v1.numel()
        valu = n * taps * TAP_LANE_CYCLES / LANE_CYCLES_PER_S * 1e3
        a, b = v1.clone().requires_grad_(), v2.clone().requires_grad_()
        dist = ops.census3d_dist(a, b, r)
        hip_bwd = lambda: torch.autograd.grad(dist, [a, b], G, retain_graph=True)
        for way, hip, stock, nbytes in (
                ("fwd", lambda: ops.census3d_dist(v1, v2, r), lambda: torch_census_fwd(v1, v2, r), 12 * n),
                ("bwd", hip_bwd, lambda: torch_census_bwd(v1, v2, G, r), 20 * n)):
            ms, ms_t = alternating(hip, stock, warmup, iters, 2 if r > 1 else 5)
            hbm = nbytes / HBM_BPS * 1e3
            floor, bound = (hbm, "bytes / 8 TB/s") if r == 1 else (valu, "taps x 20 lane-cycles / vector rate")
            err = (relerr(hip(), stock()) if way == "fwd" else
                   max(relerr(x, y) for x, y in zip(hip(), stock())))
            rows.append(row("census3d r=%d %s" % (r, way), ms, ms_t, floor, bound, err))
            rows[-1].update(hbm_floor_ms=hbm, valu_floor_ms=valu, taps=taps)
        del dist, a, b
    return rows


def smooth_cases(S, warmup, iters):
    g = torch.Generator(device="cuda").manual_seed(2)
    flow = torch.randn(2, 6, S, S, S, device="cuda", generator=g)
    guide = torch.rand(2, 1, S, S, S, device="cuda", generator=g)
    rows = []
    for kappa in (0.0, 10.0):
        f = flow.clone().requires_grad_()
        loss = ops.flow_smooth3d(f, guide, 0.25, 1e-9, kappa)
        ft = flow.clone().requires_grad_()
        loss_t = torch_smooth(ft, guide, 0.25, 1e-9, kappa)
        nb = 4 * (flow.numel() + (guide.numel() if kappa else 0))
        for way, hip, stock, nbytes in (
                ("fwd", lambda: ops.flow_smooth3d(flow, guide, 0.25, 1e-9, kappa),
                 lambda: torch_smooth(flow, guide, 0.25, 1e-9, kappa), nb),
                ("bwd", lambda: torch.autograd.grad(loss, [f], retain_graph=True)[0],
                 lambda: torch.autograd.grad(loss_t, [ft], retain_graph=True)[0], nb + 4 * flow.numel())):
            ms, ms_t = alternating(hip, stock, warmup, iters, 5)
            a, b = hip(), stock()
            err = relerr(a, b) if way == "bwd" else abs(float(a) - float(b)) / abs(float(b))
            rows.append(row("flow_smooth3d kappa=%g %s" % (kappa, way), ms, ms_t, nbytes / HBM_BPS * 1e3,
                            "bytes / 8 TB/s", err))
        del loss, loss_t, f, ft
    return rows


def copy_case(warmup, iters):
    a = torch.empty(2 * 3 * 256 ** 3, device="cuda").normal_()
    b = torch.empty_like(a)
    ms = timed(lambda: b.copy_(a), warmup, iters)
    return {"case": "torch copy_ of 403 MB", "ms": ms, "TBps": 2 * a.numel() * 4 / ms / 1e9,
            "share_of_hbm_roof": 2 * a.numel() * 4 / HBM_BPS * 1e3 / ms}


def step_cases(S):
    from opticalflowscivis_amd.data import synthetic
    from opticalflowscivis_amd.flow3d.model.RIFE import Model
    from opticalflowscivis_amd.rife import UnsupLoss
    torch.manual_seed(1)
    m = Model(local_rank=-1, device="cuda")
    data = synthetic.droplet3d_batch(2, S, seed=1, device="cuda")
    imgs, gt = data[:, :2].contiguous(), data[:, 2:3].contiguous()
    cases = [("plain step (1)", None), ("photo + census r=1 + smooth", UnsupLoss(1e-3, 1e-3, 1e-4, 1, smooth_kappa=10.)),
             ("photo + census r=3 + smooth", UnsupLoss(1e-3, 1e-3, 1e-4, 3, smooth_kappa=10.)), ("plain step (2)", None)]
    rows = []
    for name, u in cases:
        kw = {} if u is None else {"unsup": u}
        ms = timed(lambda: m.update(imgs, gt, learning_rate=1e-5, training=True, **kw), 2, 5)
        rows.append({"case": name, "ms_per_step": ms})
        print("%-30s %8.2f ms/step (eager, 2 x %d^3)" % (name, ms, S), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "unsup3dbench needs a GPU"
    doc = {"device": torch.cuda.get_device_name(0), "size": args.size}
    doc["census3d"] = census_cases(args.size, args.warmup, args.iters)
    torch.cuda.empty_cache()
    doc["flow_smooth3d"] = smooth_cases(args.size, args.warmup, args.iters)
    torch.cuda.empty_cache()
    doc["copy"] = cp = copy_case(args.warmup, args.iters)
    print("%-28s %8.3f ms  %5.2f TB/s  %.2f of the 8 TB/s roof" % (cp["case"], cp["ms"], cp["TBps"], cp["share_of_hbm_roof"]))
    torch.cuda.empty_cache()
    if args.step:
        doc["train_step"] = step_cases(args.size)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
