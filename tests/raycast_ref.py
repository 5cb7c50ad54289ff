"""The arithmetic of fs_raycast3d (include/flowsci_hip.h) restated in numpy, vectorised over the pixels of one frame,
in fp64 or -- with dtype=np.float32 -- in fp32 with the kernel's operations in the kernel's order (numpy does not fuse
multiply-adds: the sample positions, and with them the cell every sample falls in, are the kernel's bit for bit).

A ray's samples lie at (k + 1/2) dt from its origin for k = 0, 1, ...; one outside the box grown by a cell weighs exactly
0, so the loop runs only over the k some ray of the frame can need (bound=True: a slab test in fp64 with two samples to
spare) -- bound=False walks every k from 0 to the same upper end and gives the same bits.
"""
import numpy as np

DVR, MIP = "dvr", "mip"


def rays(cam, image, dtype):
    """Origins and unit directions [Hi, Wi, 3] of the camera's pixels; pixel (i, j) is column i of row j."""
    Hi, Wi = image
    c = np.asarray(cam, np.float32).astype(dtype).reshape(6, 3)
    i = np.arange(Wi, dtype=dtype)[None, :, None]
    j = np.arange(Hi, dtype=dtype)[:, None, None]
    o = (c[0] + i * c[1]) + j * c[2]
    g = (c[3] + i * c[4]) + j * c[5]
    ln = np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        d = g / ln[..., None]
    return o.astype(dtype), d.astype(dtype)


def table(tf, u, dtype):
    """The table's row at position u in [0, 1]: [..., 4]."""
    n = tf.shape[0]
    s = u * dtype(n - 1)
    j = np.minimum(np.floor(s).astype(np.int64), n - 2)
    ft = (s - j.astype(dtype))[..., None]
    return tf[j] + ft * (tf[j + 1] - tf[j])


def k_range(o, d, N, h, dt):
    """(k0, k1): every sample of every ray that can weigh more than 0 has k0 <= k <= k1 (fp64; empty: k1 < k0)."""
    o, d = o.astype(np.float64).reshape(-1, 3), d.astype(np.float64).reshape(-1, 3)
    lo, hi = -1.001 * h, (N + 0.001) * h
    tn, tf = np.zeros(len(o)), np.full(len(o), np.inf)
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(3):
            z = d[:, a] == 0
            t1, t2 = (lo[a] - o[:, a]) / d[:, a], (hi[a] - o[:, a]) / d[:, a]
            tn = np.where(z, tn, np.maximum(tn, np.minimum(t1, t2)))
            tf = np.where(z, tf, np.minimum(tf, np.maximum(t1, t2)))
            ok &= ~z | ((o[:, a] > lo[a]) & (o[:, a] < hi[a]))
    ok &= tn <= tf
    if not ok.any():
        return 0, -1
    return max(0, int(np.floor(tn[ok].min() / dt)) - 2), int(np.ceil(tf[ok].max() / dt)) + 2


def raycast(vol, cam, tf, lo, hi, dt, spacing, image, mode=DVR, t_min=0.0, dtype=np.float64, bound=True):
    """One frame: vol [D, H, W], cam 18 numbers (o, ou, ov, d, du, dv in (x, y, z)), tf [n, 4], spacing one value or
    (D, H, W) -> image [Hi, Wi, 4] of `dtype`."""
    dtype = np.dtype(dtype).type
    vol = np.asarray(vol, np.float32)
    N = np.array(vol.shape[::-1])  # W, H, D
    h64 = np.broadcast_to(np.asarray(spacing, np.float64), (3,))[::-1]
    ih = (1.0 / h64).astype(dtype)
    tf = np.asarray(tf, np.float32).astype(dtype)
    lo_, inv_range, dt_, t_min_ = dtype(lo), dtype(1.0 / (float(hi) - float(lo))), dtype(dt), dtype(t_min)
    o, d = rays(cam, image, dtype)
    k0, k1 = k_range(o, d, N, h64, float(dt))
    if not bound:
        k0 = 0
    flat = vol.reshape(-1).astype(dtype)
    N1 = (N - 1).astype(dtype)
    one, zero = dtype(1), dtype(0)
    C = np.zeros(tuple(image) + (3,), dtype)
    T = np.ones(tuple(image), dtype)
    m = np.zeros(tuple(image), dtype)
    alive = np.ones(tuple(image), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(k0, k1 + 1):
            t = (dtype(k) + dtype(0.5)) * dt_
            q = (o + t * d) * ih
            out = np.maximum(zero, np.maximum(-q, q - N1))
            ca = np.maximum(zero, one - out)
            c = (ca[..., 0] * ca[..., 1]) * ca[..., 2]
            qc = np.minimum(np.maximum(q, zero), N1)
            qc = np.where(np.isnan(q), zero, qc)  # (such a ray misses: its weight below is 0)
            i0 = np.minimum(np.floor(qc).astype(np.int64), N - 2)
            f = qc - i0.astype(dtype)
            base = (i0[..., 2] * N[1] + i0[..., 1]) * N[0] + i0[..., 0]
            sy, sz = N[0], N[0] * N[1]
            fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
            lerp = lambda a, b, w: a + w * (b - a)
            v00 = lerp(flat[base], flat[base + 1], fx)
            v01 = lerp(flat[base + sy], flat[base + sy + 1], fx)
            v10 = lerp(flat[base + sz], flat[base + sz + 1], fx)
            v11 = lerp(flat[base + sz + sy], flat[base + sz + sy + 1], fx)
            v = lerp(lerp(v00, v01, fy), lerp(v10, v11, fy), fz)
            fin = np.isfinite(v) & np.isfinite(c)
            u = np.minimum(np.maximum((np.where(fin, v, lo_) - lo_) * inv_range, zero), one)
            if mode == MIP:
                m = np.where(fin, np.maximum(m, c * u), m)
                continue
            s = table(tf, u, dtype)
            e = np.exp(-((s[..., 3] * c) * dt_)).astype(dtype)
            on = fin & alive
            w = T * (one - e)
            C = np.where(on[..., None], C + w[..., None] * s[..., :3], C)
            T = np.where(on, T * e, T)
            alive &= ~(T < t_min_)
    if mode == MIP:
        return table(tf, m, dtype).astype(dtype)
    return np.concatenate([C, (one - T)[..., None]], -1).astype(dtype)


def raycast_frames(vols, cams, tf, lo, hi, dt, spacing, image, mode=DVR, t_min=0.0, dtype=np.float64):
    """K frames: vols [K, D, H, W], cams [K, 18] -> [K, Hi, Wi, 4]."""
    return np.stack([raycast(v, c, tf, lo, hi, dt, spacing, image, mode, t_min, dtype) for v, c in zip(vols, cams)])


def brick_ranges(vol, brick=8):
    """(range [nbz, nby, nbx, 2], nonfinite [nbz, nby, nbx]) of one volume: bricks of `brick` cells, brick + 1 nodes."""
    vol = np.asarray(vol, np.float32)
    nb = [(n - 1 + brick - 1) // brick for n in vol.shape]
    rng = np.empty(tuple(nb) + (2,), np.float32)
    bad = np.zeros(tuple(nb), np.uint8)
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                blk = vol[bz * brick:bz * brick + brick + 1, by * brick:by * brick + brick + 1, bx * brick:bx * brick + brick + 1]
                fin = np.isfinite(blk)
                bad[bz, by, bx] = not fin.all()
                rng[bz, by, bx] = (blk[fin].min(), blk[fin].max()) if fin.any() else (np.inf, -np.inf)
    return rng, bad
