"""numpy fp64 restatement of fs_velgrad2d / fs_velgrad3d (include/flowsci_hip.h "Velocity gradient"): the difference
selection, J, div, vort, q and M with the header's operations in the header's order, vectorised over the nodes (every
node's arithmetic is independent).  lambda2 comes from np.linalg.eigvalsh, not from a copy of the kernel's solver.
Imports nothing from the product."""
import numpy as np

CENTRAL, FORWARD, BACKWARD = 0, 1, 2
FIELDS = {"div": 1, "vort": 2, "vmag": 4, "q": 8, "l2": 16, "grad": 32}  # FS_VG_*, in the order of the planes
ALL = tuple(FIELDS)
FLAG_Q, FLAG_L2, FLAG_NONFINITE = 1, 2, 128


def planes(fields, C):
    """name -> slice of the selected planes, in the kernel's order."""
    width = {"div": 1, "vort": 3 if C == 3 else 1, "vmag": 1, "q": 1, "l2": 1, "grad": C * C}
    out, p = {}, 0
    for name in FIELDS:
        if name in fields:
            out[name] = slice(p, p + width[name])
            p += width[name]
    return out


def jacobian(u, inv_h, inv_2h, scale):
    """u [C, *sp] fp32 (component 0 = x), inv_h / inv_2h per axis (axis 0 = x) -> (J [C, C, *sp] fp64 with
    J[r, c] = d u_r / d x_c, kinds [C, *sp]: the difference taken along axis c)."""
    C = u.shape[0]
    sp = u.shape[1:]
    idx = np.indices(sp)
    J = np.zeros((C, C) + sp, np.float64)
    kinds = np.zeros((C,) + sp, np.int64)
    for c in range(C):
        ax = C - 1 - c  # numpy axis of axis c
        i = idx[ax]
        hm, hp = i > 0, i + 1 < sp[ax]
        kinds[c] = np.where(hm & hp, CENTRAL, np.where(hp, FORWARD, BACKWARD))
        lo, hi = list(idx), list(idx)
        lo[ax] = np.where(hm, i - 1, i)
        hi[ax] = np.where(hp, i + 1, i)
        w = np.where(hm & hp, inv_2h[c], inv_h[c])
        for r in range(C):
            J[r, c] = ((u[r][tuple(hi)].astype(np.float64) - u[r][tuple(lo)].astype(np.float64)) * w) * scale
    return J, kinds


def velgrad(flows, fields=ALL, spacing=1.0, scale=1.0):
    """flows [K, C, *sp] fp32; spacing one value or one per axis in the array's axis order; scale one value or K.
    -> dict: out fp32 [K, NP, *sp], planes, flags uint8 [K, *sp], l2_64 / normM / J (fp64, [K, ...]: lambda2 before its
    rounding, ||M||_F and the gradient), l2_decides (fp64: the eigenvalue whose sign decides l2 < 0 -- lambda2 itself in
    3-D, the larger of the plane's two in 2-D, where the median with the embedding's 0 is exactly 0 at every node whose
    two straddle it) and kinds [C, *sp]."""
    flows = np.asarray(flows, np.float32)
    K, C = flows.shape[:2]
    sp = flows.shape[2:]
    fields = [f.strip() for f in fields.split(",")] if isinstance(fields, str) else list(fields)
    hs = [float(v) for v in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * C
    hs = hs[::-1]  # axis 0 runs along x, the array's last axis
    inv_h = [1.0 / h for h in hs]
    inv_2h = [1.0 / (2.0 * h) for h in hs]
    ss = [float(v) for v in scale] if hasattr(scale, "__len__") else [float(scale)] * K
    pl = planes(fields, C)
    NP = max(s.stop for s in pl.values())
    out = np.zeros((K, NP) + sp, np.float32)
    flags = np.zeros((K,) + sp, np.uint8)
    l2_64 = np.zeros((K,) + sp, np.float64)
    normM = np.zeros((K,) + sp, np.float64)
    decides = np.zeros((K,) + sp, np.float64)
    Jall = np.zeros((K, C, C) + sp, np.float64)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(K):
            J, kinds = jacobian(flows[k], inv_h, inv_2h, ss[k])
            Jall[k] = J
            fin = np.isfinite(J).all((0, 1))
            vals = {}
            if C == 3:
                vals["div"] = f32((J[0, 0] + J[1, 1]) + J[2, 2])[None]
                w = [J[2, 1] - J[1, 2], J[0, 2] - J[2, 0], J[1, 0] - J[0, 1]]
                vals["vort"] = f32(np.stack(w))
                vals["vmag"] = f32(np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]))[None]
                s00, s11, s22 = J[0, 0], J[1, 1], J[2, 2]
                s01, s02, s12 = 0.5 * (J[0, 1] + J[1, 0]), 0.5 * (J[0, 2] + J[2, 0]), 0.5 * (J[1, 2] + J[2, 1])
                o01, o02, o12 = 0.5 * (J[0, 1] - J[1, 0]), 0.5 * (J[0, 2] - J[2, 0]), 0.5 * (J[1, 2] - J[2, 1])
                nS = ((s00 * s00 + s11 * s11) + s22 * s22) + 2.0 * ((s01 * s01 + s02 * s02) + s12 * s12)
                nO = 2.0 * ((o01 * o01 + o02 * o02) + o12 * o12)
                M = np.zeros(sp + (3, 3), np.float64)
                M[..., 0, 0] = ((s00 * s00 + s01 * s01) + s02 * s02) - (o01 * o01 + o02 * o02)
                M[..., 1, 1] = ((s01 * s01 + s11 * s11) + s12 * s12) - (o01 * o01 + o12 * o12)
                M[..., 2, 2] = ((s02 * s02 + s12 * s12) + s22 * s22) - (o02 * o02 + o12 * o12)
                M[..., 0, 1] = M[..., 1, 0] = ((s00 * s01 + s01 * s11) + s02 * s12) - o02 * o12
                M[..., 0, 2] = M[..., 2, 0] = ((s00 * s02 + s01 * s12) + s02 * s22) + o01 * o12
                M[..., 1, 2] = M[..., 2, 1] = ((s01 * s02 + s11 * s12) + s12 * s22) - o01 * o02
            else:
                vals["div"] = f32(J[0, 0] + J[1, 1])[None]
                w0 = J[1, 0] - J[0, 1]
                vals["vort"] = f32(w0)[None]
                vals["vmag"] = f32(np.abs(w0))[None]
                s00, s11 = J[0, 0], J[1, 1]
                s01, o01 = 0.5 * (J[0, 1] + J[1, 0]), 0.5 * (J[0, 1] - J[1, 0])
                nS = (s00 * s00 + s11 * s11) + 2.0 * (s01 * s01)
                nO = 2.0 * (o01 * o01)
                M = np.zeros(sp + (2, 2), np.float64)
                M[..., 0, 0] = (s00 * s00 + s01 * s01) - o01 * o01
                M[..., 1, 1] = (s01 * s01 + s11 * s11) - o01 * o01
                M[..., 0, 1] = M[..., 1, 0] = s00 * s01 + s01 * s11
            vals["q"] = f32(0.5 * (nO - nS))[None]
            okM = fin & np.isfinite(M).all((-1, -2))
            lam = np.full(sp, np.nan)
            dec = np.full(sp, np.nan)
            if okM.any():
                ev = np.linalg.eigvalsh(M[okM])
                dec[okM] = ev[:, 1]
                if C == 2:
                    ev = np.sort(np.concatenate([ev, np.zeros((ev.shape[0], 1))], 1), 1)
                lam[okM] = ev[:, 1]
            l2_64[k] = lam
            decides[k] = dec
            normM[k] = np.sqrt((M * M).sum((-1, -2)))
            vals["l2"] = f32(lam)[None]
            vals["grad"] = f32(J.reshape((C * C,) + sp))
            for name in pl:
                fin = fin & np.isfinite(vals[name]).all(0)
            for name, s in pl.items():
                out[k, s] = np.where(fin, vals[name], np.float32(np.nan))
            bq = fin & (vals["q"][0] > 0) if "q" in pl else np.zeros(sp, bool)
            bl = fin & (vals["l2"][0] < 0) if "l2" in pl else np.zeros(sp, bool)
            flags[k] = np.where(fin, bq * FLAG_Q + bl * FLAG_L2, FLAG_NONFINITE).astype(np.uint8)
    return {"out": out, "planes": pl, "flags": flags, "l2_64": l2_64, "normM": normM, "J": Jall, "l2_decides": decides,
            "kinds": kinds}
