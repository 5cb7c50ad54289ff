"""fp64 restatement of ops.flow_consistency / fs_flow_consistency{2,3}d (numpy, CPU; nothing of the package is
imported): the per-element classes, residual and photometric error, the per-pair sums in the kernel's order
(include/flowsci_hip.h, FS_FLOW_CONSISTENCY_K) and the statistics ops.flow_consistency derives from them.

Every operation that decides a class (the sample point, the corner weights, the corner sums, r2, m2 and the threshold)
is the same fp64 operation in the same order as in the kernel, which uses no fused multiply-adds: the counts and the
class map are equal exactly."""
import numpy as np

NOT_VALID, CONSISTENT, OCCLUDED, OUTGOING, NONFINITE = 0, 1, 2, 3, 4
K = 13


def _grid(sp):
    """x_c per channel c (0 along the LAST axis), broadcastable against [N,*sp]."""
    nd = len(sp)
    out = []
    for c in range(nd):
        ax = nd - 1 - c
        shape = [1] * (nd + 1)
        shape[ax + 1] = sp[ax]
        out.append(np.arange(sp[ax], dtype=np.float64).reshape(shape))
    return out


def per_element(flow_f, flow_b, img0=None, img1=None, alpha=(0.01, 0.5)):
    """(cls uint8 [N,*sp] as if every element were valid, r fp64 [N,*sp] (NaN where outgoing / nonfinite), r2, e)."""
    ff = np.asarray(flow_f, dtype=np.float32)
    fb = np.asarray(flow_b, dtype=np.float32).astype(np.float64)
    N, C = ff.shape[:2]
    sp = ff.shape[2:]
    assert C == len(sp) and fb.shape == ff.shape
    images = img0 is not None
    if images:
        i0 = np.asarray(img0, dtype=np.float32).astype(np.float64).reshape((N,) + sp)
        i1 = np.asarray(img1, dtype=np.float32).astype(np.float64).reshape((N,) + sp)
    S = [sp[C - 1 - c] for c in range(C)]  # extent along channel c's axis
    x = _grid(sp)
    fd = ff.astype(np.float64)
    nonfin = ~np.all(np.isfinite(ff), 1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = [x[c] + fd[:, c] for c in range(C)]
        out = np.zeros(nonfin.shape, bool)
        for c in range(C):
            out |= (p[c] < 0.0) | (p[c] > float(S[c] - 1))
        out &= ~nonfin
        inside = ~nonfin & ~out
        # sample only where inside; elsewhere a harmless stand-in point (index 0, weights (1, 0))
        i0c, i1c, fr, gr = [], [], [], []
        for c in range(C):
            pc = np.where(inside, p[c], 0.0)
            fl = np.floor(pc)
            a = fl.astype(np.int64)
            i0c.append(a)
            i1c.append(np.minimum(a + 1, S[c] - 1))
            fr.append(pc - fl)
            gr.append(1.0 - (pc - fl))
        nidx = np.arange(N).reshape((N,) + (1,) * C)
        Fbw = [np.zeros(nonfin.shape) for _ in range(C)]
        I1w = np.zeros(nonfin.shape)
        for k in range(1 << C):
            bits = [(k >> c) & 1 for c in range(C)]  # bit c belongs to channel c: bx, by, bz
            t = [fr[c] if bits[c] else gr[c] for c in range(C)]
            w = (t[2] * t[1]) * t[0] if C == 3 else t[1] * t[0]
            idx = tuple((i1c[c] if bits[c] else i0c[c]) for c in reversed(range(C)))  # axes order: (D,) H, W
            for c in range(C):
                Fbw[c] = Fbw[c] + w * fb[:, c][(nidx,) + idx]
            if images:
                I1w = I1w + w * i1[(nidx,) + idx]
        r2 = np.zeros(nonfin.shape)
        sa = np.zeros(nonfin.shape)
        sb = np.zeros(nonfin.shape)
        sfin = np.ones(nonfin.shape, bool)
        fz = np.where(inside[:, None], fd, 0.0)
        for c in range(C):
            s = fz[:, c] + Fbw[c]
            r2 = r2 + s * s
            sa = sa + fz[:, c] * fz[:, c]
            sb = sb + Fbw[c] * Fbw[c]
            sfin &= np.isfinite(Fbw[c])
        m2 = sa + sb
        r = np.sqrt(r2)
        e = np.zeros(nonfin.shape)
        if images:
            sfin &= np.isfinite(i0) & np.isfinite(I1w)
            e = I1w - i0
        occ = r2 > float(alpha[0]) * m2 + float(alpha[1])
    cls = np.full(nonfin.shape, CONSISTENT, np.uint8)
    cls[occ] = OCCLUDED
    cls[~sfin] = NONFINITE
    cls[out] = OUTGOING
    cls[nonfin] = NONFINITE
    ok = (cls == CONSISTENT) | (cls == OCCLUDED)
    return cls, np.where(ok, r, np.nan), np.where(ok, r2, np.nan), np.where(ok, e, np.nan)


def sums(flow_f, flow_b, img0=None, img1=None, valid=None, alpha=(0.01, 0.5)):
    """out [N, 13] in the kernel's order."""
    cls, r, r2, e = per_element(flow_f, flow_b, img0, img1, alpha)
    N = cls.shape[0]
    v = np.ones(cls.shape, bool) if valid is None else np.asarray(valid).astype(bool).reshape(cls.shape)
    res = np.zeros((N, K))
    for n in range(N):
        c = np.where(v[n], cls[n], NOT_VALID)
        ins = (c == CONSISTENT) | (c == OCCLUDED)
        noc = c == CONSISTENT
        res[n, 0] = v[n].sum()
        res[n, 1] = (c == NONFINITE).sum()
        res[n, 2] = (c == OUTGOING).sum()
        res[n, 3] = (c == OCCLUDED).sum()
        res[n, 4] = noc.sum()
        res[n, 5] = r[n][ins].sum()
        res[n, 6] = r2[n][ins].sum()
        res[n, 7] = r[n][ins].max() if ins.any() else -np.inf
        res[n, 8] = r[n][noc].sum()
        if img0 is not None:
            res[n, 9] = np.abs(e[n][ins]).sum()
            res[n, 10] = (e[n][ins] * e[n][ins]).sum()
            res[n, 11] = np.abs(e[n][noc]).sum()
            res[n, 12] = (e[n][noc] * e[n][noc]).sum()
    return res


COUNTS = ("n_valid", "n_inside", "n_noc", "n_occ", "n_out", "n_nonfinite")
RATIOS = ("fb_mean", "fb_rmse", "fb_mean_noc", "occ_frac", "out_frac", "warp_l1", "warp_l1_noc", "warp_psnr",
          "warp_psnr_noc")


def stats(flow_f, flow_b, img0=None, img1=None, valid=None, alpha=(0.01, 0.5)):
    """The dict ops.flow_consistency returns (without the maps), as fp64 numpy arrays."""
    s = sums(flow_f, flow_b, img0, img1, valid, alpha)

    def div(a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(b > 0, a / np.where(b > 0, b, 1), np.nan)

    n, nf, nout, nocc, nnoc = (s[:, k] for k in range(5))
    nin = nocc + nnoc
    nan = np.full(len(n), np.nan)
    with np.errstate(divide="ignore"):
        r = {"fb_mean": div(s[:, 5], nin), "fb_rmse": np.sqrt(div(s[:, 6], nin)),
             "fb_max": np.where(nin > 0, s[:, 7], np.nan), "fb_mean_noc": div(s[:, 8], nnoc),
             "occ_frac": div(nocc, nin), "out_frac": div(nout, n),
             "n_valid": n, "n_inside": nin, "n_noc": nnoc, "n_occ": nocc, "n_out": nout, "n_nonfinite": nf}
        if img0 is not None:
            r.update(warp_l1=div(s[:, 9], nin), warp_l1_noc=div(s[:, 11], nnoc),
                     warp_psnr=-10.0 * np.log10(div(s[:, 10], nin)), warp_psnr_noc=-10.0 * np.log10(div(s[:, 12], nnoc)))
        else:
            r.update(warp_l1=nan, warp_l1_noc=nan.copy(), warp_psnr=nan.copy(), warp_psnr_noc=nan.copy())
    return r


def class_map(flow_f, flow_b, img0=None, img1=None, valid=None, alpha=(0.01, 0.5)):
    cls = per_element(flow_f, flow_b, img0, img1, alpha)[0]
    if valid is None:
        return cls
    return np.where(np.asarray(valid).astype(bool).reshape(cls.shape), cls, NOT_VALID).astype(np.uint8)


def res_map(flow_f, flow_b, img0=None, img1=None, alpha=(0.01, 0.5)):
    return per_element(flow_f, flow_b, img0, img1, alpha)[1].astype(np.float32)
