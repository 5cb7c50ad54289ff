"""The numpy restatement of the parallel-vectors section of include/flowsci_hip.h: the same fp64 operations in the same
order on every owned face of the Kuhn split at once, so that ops.parallel_vectors must reproduce every bit of every
column.  `reject=False` switches step 2 (the Bernstein test) off: it may only save work, never remove a point."""
import numpy as np

# the owned faces of a node: slot s has the corners 0 < MID[s] < HI[s] of the cell the node is the origin of
MID = (1, 1, 2, 2, 4, 4, 3, 5, 6, 1, 2, 4)
HI = (3, 5, 3, 6, 5, 6, 7, 7, 7, 7, 7, 7)
C1 = (1, 1, 2, 2, 4, 4)
# face f of tetrahedron t (the triangle that omits corner f) -> (the corner of the cell that owns it, its slot there)
TET_FACE = tuple(((C1[t], (3, 5, 1, 4, 0, 2)[t]), (0, 6 + (0, 1, 0, 2, 1, 2)[t]), (0, 9 + (t >> 1)), (0, t)) for t in range(6))
BISECTIONS, NEWTONS = 64, 2


def det3(a, b, c):
    return (a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) -
            a[..., 1] * (b[..., 0] * c[..., 2] - b[..., 2] * c[..., 0])) + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _ss(a):
    return (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]


def solve_faces(V, W, live, vmin=0.0, wmin=0.0, reject=True):
    """Steps 1-5 for F faces.  V, W: fp64 [F, 3 corners, 3 components]; live: bool [F], the faces that exist and whose
    corners are finite.  Returns a dict: acc (bool [F, 3]: root r is an accepted point), lam, l ([F, 3, 3]: the
    barycentric coordinates of root r), nroots, swapped, degenerate, survived (the faces that passed steps 1 and 2)."""
    with np.errstate(all="ignore"):
        F = len(V)
        vm, wm = np.float64(np.float32(vmin)), np.float64(np.float32(wmin))
        quiet = (_ss(V) <= vm * vm) | (_ss(W) <= wm * wm)  # [F, 3]
        live = live & ~quiet.all(1)
        if reject:
            out = np.zeros(F, bool)
            for k in range(3):
                j, l = (k + 1) % 3, (k + 2) % 3
                cr = lambda p, q: V[:, p, j] * W[:, q, l] - V[:, p, l] * W[:, q, j]
                six = np.stack([cr(0, 0), cr(1, 1), cr(2, 2), cr(0, 1) + cr(1, 0), cr(0, 2) + cr(2, 0), cr(1, 2) + cr(2, 1)], 1)
                out |= (six > 0).all(1) | (six < 0).all(1)
            live = live & ~out
        survived = live.copy()
        dV, dW = det3(V[:, 0], V[:, 1], V[:, 2]), det3(W[:, 0], W[:, 1], W[:, 2])
        swapped = ~(np.abs(dW) >= np.abs(dV))
        s3 = swapped[:, None, None]
        A, B = np.where(s3, V, W), np.where(s3, W, V)
        dA, dB = np.where(swapped, dV, dW), np.where(swapped, dW, dV)
        degenerate = live & ((dA == 0) | ~np.isfinite(dA))
        live = live & ~degenerate
        m1 = (det3(A[:, 0], B[:, 1], B[:, 2]) + det3(B[:, 0], A[:, 1], B[:, 2])) + det3(B[:, 0], B[:, 1], A[:, 2])
        m2 = (det3(A[:, 0], A[:, 1], B[:, 2]) + det3(A[:, 0], B[:, 1], A[:, 2])) + det3(B[:, 0], A[:, 1], A[:, 2])
        a, b, c = -(m2 / dA), m1 / dA, -(dB / dA)
        p = lambda x: ((x + a) * x + b) * x + c
        dp = lambda x: (3.0 * x + 2.0 * a) * x + b
        mx = np.abs(a)
        mx = np.where(np.abs(b) > mx, np.abs(b), mx)
        mx = np.where(np.abs(c) > mx, np.abs(c), mx)
        R = 1.0 + mx
        disc = a * a - 3.0 * b
        two = disc > 0
        sq = np.sqrt(np.where(two, disc, 0.0))
        k1 = np.where(two, (-a - sq) / 3.0, -R)
        k2 = np.where(two, (-a + sq) / 3.0, -R)
        acc = np.zeros((F, 3), bool)
        lam = np.zeros((F, 3))
        bary = np.zeros((F, 3, 3))
        nroots = np.zeros(F, np.int64)
        for lo, hi in ((-R, k1), (k1, k2), (k2, R)):
            lo, hi = lo.copy(), hi.copy()
            sl = p(lo) < 0
            found = live & (lo < hi) & (sl != (p(hi) < 0))
            for _ in range(BISECTIONS):
                m = 0.5 * (lo + hi)
                left = (p(m) < 0) == sl
                lo, hi = np.where(left, m, lo), np.where(left, hi, m)
            x = 0.5 * (lo + hi)
            for _ in range(NEWTONS):
                xn = x - p(x) / dp(x)
                x = np.where(np.isfinite(xn) & (xn >= lo) & (xn <= hi), xn, x)
            N = B - x[:, None, None] * A  # [F, corner, component]
            rows = [N[:, :, r] for r in range(3)]
            n = _cross(rows[0], rows[1])
            best = _ss(n)
            for pr in ((0, 2), (1, 2)):
                n2 = _cross(rows[pr[0]], rows[pr[1]])
                s2 = _ss(n2)
                better = s2 > best
                n, best = np.where(better[:, None], n2, n), np.where(better, s2, best)
            ok = found & ((n > 0).all(1) | (n < 0).all(1))
            S = (n[:, 0] + n[:, 1]) + n[:, 2]
            at = np.nonzero(found)[0]
            r = nroots[at]
            acc[at, r] = ok[at]
            lam[at, r] = x[at]
            bary[at, r] = (n / S[:, None])[at]
            nroots[at] += 1
        return {"acc": acc, "lam": lam, "l": bary, "nroots": nroots, "swapped": swapped, "degenerate": degenerate,
                "survived": survived}


def gather_faces(f, D, H, W):
    """The three corner values of every slot of every node of one step.  f: [C, D, H, W].  Returns (vals fp64
    [P * 12, 3 corners, C], exists bool [P * 12], origin int64 [P * 12, 3] as (x, y, z))."""
    C = f.shape[0]
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    z, y, x = (np.repeat(g.reshape(-1), 12) for g in (z, y, x))
    P = D * H * W
    vals = np.zeros((P * 12, 3, C))
    exists = np.ones(P * 12, bool)
    flat = f.reshape(C, P).astype(np.float64)
    for i, corners in enumerate(((0,) * 12, MID, HI)):
        c = np.tile(np.array(corners), P)
        cz, cy, cx = z + (c >> 2 & 1), y + (c >> 1 & 1), x + (c & 1)
        ok = (cz < D) & (cy < H) & (cx < W)
        exists &= ok
        node = (np.minimum(cz, D - 1) * H + np.minimum(cy, H - 1)) * W + np.minimum(cx, W - 1)
        vals[:, i, :] = flat[:, node].T
    return vals, exists, np.stack([x, y, z], 1)


def _spacing(spacing):
    hs = [float(s) for s in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * 3
    return np.array([1.0 / h for h in hs[::-1]])  # inv_h by axis x, y, z


def step_faces(v, w, aux=None, vmin=0.0, wmin=0.0, reject=True):
    """solve_faces on every owned face of one step (v, w: [3, D, H, W]; aux: [D, H, W] or None), with the gathered
    values: adds V, W, AUX ([F, 3]), origin, exists, finite."""
    _, D, H, W = v.shape
    V, exists, origin = gather_faces(v, D, H, W)
    Wv, _, _ = gather_faces(w, D, H, W)
    AUX = gather_faces(aux[None], D, H, W)[0][:, :, 0] if aux is not None else None
    fin = np.isfinite(V).all((1, 2)) & np.isfinite(Wv).all((1, 2))
    if AUX is not None:
        fin &= np.isfinite(AUX).all(1)
    with np.errstate(all="ignore"):
        clean = lambda a: np.where(np.isfinite(a), a, 0.0)
        r = solve_faces(clean(V), clean(Wv), exists & fin, vmin, wmin, reject)
    r.update(V=V, W=Wv, AUX=AUX, origin=origin, exists=exists, finite=fin)
    return r


def parallel_vectors(v, w, aux=None, spacing=1.0, vmin=0.0, wmin=0.0, reject=True):
    """What ops.parallel_vectors returns, as host arrays.  v, w: [K, 3, D, H, W] fp32; aux: [K, D, H, W] fp32 or None."""
    v, w = np.asarray(v, np.float32), np.asarray(w, np.float32)
    K, _, D, H, W = v.shape
    inv_h = _spacing(spacing)
    P = D * H * W
    cols = {n: [] for n in ("cell", "simplex", "face", "key", "pos", "mu", "vel", "aux")}
    counts = np.zeros((K, 4), np.int64)
    zz, yy, xx = np.meshgrid(np.arange(D - 1), np.arange(H - 1), np.arange(W - 1), indexing="ij")
    cell = ((zz * H + yy) * W + xx).reshape(-1)
    corner_off = np.array([((c >> 2 & 1) * H + (c >> 1 & 1)) * W + (c & 1) for c in range(8)])
    fid = np.stack([np.stack([(cell + corner_off[o]) * 12 + s for o, s in TET_FACE[t]], 1) for t in range(6)], 1)  # [cells, 6, 4]
    for k in range(K):
        a_k = None if aux is None else np.asarray(aux[k], np.float32)
        fs = step_faces(v[k], w[k], a_k, vmin, wmin, reject)
        node_fin = np.isfinite(v[k]).all(0).reshape(-1) & np.isfinite(w[k]).all(0).reshape(-1)
        if a_k is not None:
            node_fin &= np.isfinite(a_k).reshape(-1)
        cell_fin = node_fin[cell[:, None] + corner_off[None, :]].all(1)
        acc = fs["acc"][fid].reshape(len(cell), 6, 12)  # (face, rank) order
        n = acc.sum(2)
        seg = (n == 2) & cell_fin[:, None]
        counts[k] = (seg.sum(), ((n != 2) & (n != 0) & cell_fin[:, None]).sum(), fs["degenerate"].sum(), (~cell_fin).sum())
        ci, ti = np.nonzero(seg)
        first = acc[ci, ti].argmax(1)
        second = 11 - acc[ci, ti][:, ::-1].argmax(1)
        ends = np.stack([first, second], 1)  # [N, 2]
        f, r = ends // 3, ends % 3
        face = fid[ci[:, None], ti[:, None], f]  # [N, 2]
        l = fs["l"][face, r]  # [N, 2, 3]
        lam = fs["lam"][face, r]
        with np.errstate(all="ignore"):
            mu = np.where(fs["swapped"][face], lam, 1.0 / lam)
            org = fs["origin"][face].astype(np.float64)  # [N, 2, 3]
            pos = np.zeros(org.shape, np.float32)
            slot = face % 12
            for a in range(3):
                c = org[..., a]
                for i, tab in ((1, MID), (2, HI)):
                    on = (np.array(tab)[slot] >> a & 1) == 1
                    c = np.where(on, c + l[..., i], c)
                pos[..., a] = (c / inv_h[a]).astype(np.float32)
            Vc = fs["V"][face]  # [N, 2, corner, comp]
            vel = ((l[..., 0, None] * Vc[:, :, 0] + l[..., 1, None] * Vc[:, :, 1]) + l[..., 2, None] * Vc[:, :, 2]).astype(np.float32)
            if a_k is not None:
                Ac = fs["AUX"][face]
                cols["aux"].append(((l[..., 0] * Ac[..., 0] + l[..., 1] * Ac[..., 1]) + l[..., 2] * Ac[..., 2]).astype(np.float32))
        cols["cell"].append(cell[ci].astype(np.int32))
        cols["simplex"].append(ti.astype(np.uint8))
        cols["face"].append(f.astype(np.uint8))
        cols["key"].append((4 * face + r).astype(np.int64))
        cols["pos"].append(pos)
        cols["mu"].append(mu)
        cols["vel"].append(vel)
    shapes = {"cell": (0,), "simplex": (0,), "face": (0, 2), "key": (0, 2), "pos": (0, 2, 3), "mu": (0, 2), "vel": (0, 2, 3),
              "aux": (0, 2)}
    res = {n: np.concatenate(c).reshape((-1,) + shapes[n][1:]) for n, c in cols.items() if c}
    res["offsets"] = np.concatenate([[0], np.cumsum(counts[:, 0])]).astype(np.int64)
    res["counts"] = counts
    res["status"] = np.zeros(1, np.int32)
    return res
