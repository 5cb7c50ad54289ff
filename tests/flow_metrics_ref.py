"""fp64 restatement of ops.flow_metrics / fs_flow_metrics{2,3}d (numpy, CPU): the per-flow sums in the kernel's order
(include/flowsci_hip.h, FS_FLOW_METRICS_K) and the statistics ops.flow_metrics derives from them.

The squared error, |g|^2, the rife3d conversion and the outlier test use the same fp64 operations in the same order as
the kernel (no fused multiply-adds there), so every count here equals the kernel's exactly; the angle is evaluated in
fp64 throughout (the kernel's atan2 is fp32)."""
import numpy as np


def rife3d_to_disp_np(flow):
    """[N,3,D,H,W] Flow-3D flow -> displacement, fp64, the kernel's operation order."""
    f = flow.astype(np.float64)
    N, _, D, H, W = f.shape
    d = np.arange(D, dtype=np.float64).reshape(1, D, 1, 1)
    h = np.arange(H, dtype=np.float64).reshape(1, 1, H, 1)
    w = np.arange(W, dtype=np.float64).reshape(1, 1, 1, W)
    rx, ry, rz = (W - 1) / (H - 1), (H - 1) / (D - 1), (D - 1) / (W - 1)
    return np.stack([(h + f[:, 0]) * rx - w, (d + f[:, 1]) * ry - h, (w + f[:, 2]) * rz - d], 1)


def per_element(pred, gt, convention="disp"):
    """(e2, epe, ae, g2, finite) per element, fp64 [N,*sp]."""
    p = rife3d_to_disp_np(pred) if convention == "rife3d" else pred.astype(np.float64)
    g = gt.astype(np.float64)
    C = p.shape[1]
    fin = np.all(np.isfinite(pred), 1) & np.all(np.isfinite(gt), 1)
    with np.errstate(invalid="ignore", over="ignore"):
        e2 = np.zeros(p.shape[:1] + p.shape[2:])
        g2 = np.zeros_like(e2)
        dot = np.ones_like(e2)
        for c in range(C):
            dc = p[:, c] - g[:, c]
            e2 = e2 + dc * dc
            g2 = g2 + g[:, c] * g[:, c]
            dot = dot + p[:, c] * g[:, c]
        c2 = e2.copy()
        for i in range(C):
            for j in range(i + 1, C):
                t = p[:, i] * g[:, j] - p[:, j] * g[:, i]
                c2 = c2 + t * t
        ae = np.arctan2(np.sqrt(c2), dot)
    return e2, np.sqrt(e2), ae, g2, fin


def sums(pred, gt, valid=None, noc=None, convention="disp", tau=(3.0, 0.05)):
    """out [N, 13] in the kernel's order."""
    e2, epe, ae, g2, fin = per_element(pred, gt, convention)
    N = e2.shape[0]
    v = np.ones(e2.shape, bool) if valid is None else valid.astype(bool)
    nc = np.zeros(e2.shape, bool) if noc is None else (noc.astype(bool) & v)
    ta2, tr2 = float(np.float32(tau[0])) ** 2, float(np.float32(tau[1])) ** 2
    with np.errstate(invalid="ignore"):
        out_ = ~fin | ((e2 > ta2) & (e2 > tr2 * g2))
    res = np.zeros((N, 13))
    for n in range(N):
        for base, m in ((0, v[n]), (6, nc[n])):
            f = m & fin[n]
            res[n, base + 0] = m.sum()
            res[n, base + 1] = epe[n][f].sum()
            res[n, base + 2] = e2[n][f].sum()
            res[n, base + 3] = ae[n][f].sum()
            res[n, base + 4] = (out_[n] & m).sum()
            if base == 0:
                res[n, 5] = epe[n][f].max() if f.any() else -np.inf
        res[n, 11] = (v[n] & ~fin[n]).sum()
        res[n, 12] = (nc[n] & ~fin[n]).sum()
    return res


def stats(pred, gt, valid=None, noc=None, convention="disp", tau=(3.0, 0.05)):
    """The dict ops.flow_metrics returns (without the map), as fp64 numpy arrays."""
    s = sums(pred, gt, valid, noc, convention, tau)

    def div(a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(b > 0, a / np.where(b > 0, b, 1), np.nan)

    n, nf, nn, nfn = s[:, 0], s[:, 11], s[:, 6], s[:, 12]
    fin, finn = n - nf, nn - nfn
    r = {"epe": div(s[:, 1], fin), "rmse": np.sqrt(div(s[:, 2], fin)), "ae_deg": np.degrees(div(s[:, 3], fin)),
         "fl": div(s[:, 4], n), "max_epe": np.where(fin > 0, s[:, 5], np.nan), "n_valid": n, "n_nonfinite": nf}
    if noc is not None:
        r.update(epe_noc=div(s[:, 7], finn), epe_occ=div(s[:, 1] - s[:, 7], fin - finn), fl_noc=div(s[:, 10], nn),
                 fl_occ=div(s[:, 4] - s[:, 10], n - nn), n_noc=nn)
    else:
        r.update({k: np.full(len(n), np.nan) for k in ("epe_noc", "epe_occ", "fl_noc", "fl_occ", "n_noc")})
    return r


def epe_map(pred, gt, convention="disp"):
    _, epe, _, _, fin = per_element(pred, gt, convention)
    return np.where(fin, epe, np.nan).astype(np.float32)
