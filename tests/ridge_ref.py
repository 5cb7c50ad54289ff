"""numpy restatement of the ridge-surface definition in include/flowsci_hip.h ("Ridge surfaces"): the node pass (fp64
differences, a fixed number of cyclic Jacobi sweeps built from IEEE + - * / sqrt alone, the five stored fp32 operands and
the class byte) and the marching pass over the Kuhn split (which reads the stored operands only).  numpy rounds every
operation once and fuses nothing, so nodes() and extract() reproduce the kernels' stored bits and decisions; the vertex
values are formed in fp64 as well so that a test can bound what fp32 costs.  The orientation of every triangle comes
from tests/isosurface_ref.py's geometry, not from a copy of the kernel's table.

Not a test module: tests/test_ridge_cpu.py checks it against analysis and numpy.linalg.eigh, the GPU tests compare the
kernels against it."""
import numpy as np

from isosurface_ref import EDGE_NUMBER, EDGE_OFFSETS, PERMS, tet_corners, tet_triangles

BORDER, NONFINITE, WEAK, LOW, ELIGIBLE = 0, 1, 2, 3, 4  # FS_RIDGE_*
CLASS_NAMES = ("border", "nonfinite", "weak", "low", "eligible")
SWEEPS = 4  # FS_RIDGE_SWEEPS

# (dz, dy, dx) of the 19 stencil nodes: the centre, the 6 axis neighbours, the 12 planar diagonals
STENCIL = tuple((dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if abs(dz) + abs(dy) + abs(dx) <= 2)


def host_factors(spacing):
    """(inv_2h, inv_hh, inv_4hh) for the node spacing (x, y, z), formed in fp64 as the host forms them."""
    h = [float(v) for v in spacing]
    return ([1.0 / (2.0 * v) for v in h], [1.0 / (v * v) for v in h],
            [1.0 / (4.0 * h[0] * h[1]), 1.0 / (4.0 * h[0] * h[2]), 1.0 / (4.0 * h[1] * h[2])])


def _sh(f, dz, dy, dx):
    """f at offset (dz, dy, dx) from every interior node"""
    D, H, W = f.shape
    return f[1 + dz:D - 1 + dz, 1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]


def derivatives(vol, spacing=(1.0, 1.0, 1.0), valley=False):
    """fp64 (f, g [3], H as (h00, h11, h22, h01, h02, h12), finite) at the interior nodes [D-2, H-2, W-2]; axis 0 = x."""
    f = np.asarray(vol, dtype=np.float32).astype(np.float64)
    if valley:
        f = -f
    inv_2h, inv_hh, inv_4hh = host_factors(spacing)
    ax = ((0, 0, 1), (0, 1, 0), (1, 0, 0))  # axis c as (dz, dy, dx)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.ones(_sh(f, 0, 0, 0).shape, dtype=bool)
        for o in STENCIL:
            fin &= np.isfinite(_sh(f, *o))
        c = _sh(f, 0, 0, 0)
        g, hd = [], []
        for a in range(3):
            p, m = _sh(f, *ax[a]), _sh(f, *(-v for v in ax[a]))
            g.append((p - m) * inv_2h[a])
            hd.append(((p - 2.0 * c) + m) * inv_hh[a])
        ho = []
        for n, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
            pp = _sh(f, *(u + v for u, v in zip(ax[a], ax[b])))
            pm = _sh(f, *(u - v for u, v in zip(ax[a], ax[b])))
            mp = _sh(f, *(-u + v for u, v in zip(ax[a], ax[b])))
            mm = _sh(f, *(-u - v for u, v in zip(ax[a], ax[b])))
            ho.append(((pp - pm) - (mp - mm)) * inv_4hh[n])
    return c, g, hd + ho, fin


def _rotate(A, V, p, q):
    """One Jacobi rotation of the pair (p, q) on A = {(i, j): array, i <= j} and V = {(row, col): array}, in place."""
    r = 3 - p - q
    key = lambda i, j: (min(i, j), max(i, j))
    app, aqq, apq = A[(p, p)], A[(q, q)], A[(p, q)]
    arp, arq = A[key(r, p)], A[key(r, q)]
    skip = apq == 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        t = np.where(theta < 0.0, -t, t)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        new = {(p, p): app - t * apq, (q, q): aqq + t * apq, (p, q): np.zeros_like(apq),
               key(r, p): c * arp - s * arq, key(r, q): s * arp + c * arq}
        for k in new:
            A[k] = np.where(skip, A[k], new[k])
        for i in range(3):
            vp, vq = V[(i, p)], V[(i, q)]
            V[(i, p)], V[(i, q)] = np.where(skip, vp, c * vp - s * vq), np.where(skip, vq, s * vp + c * vq)


def jacobi(h, sweeps=SWEEPS):
    """h = (h00, h11, h22, h01, h02, h12) arrays -> (lam, e [3], residual, frobenius): the smallest diagonal entry after
    `sweeps` cyclic sweeps over (0,1), (0,2), (1,2) (ties: the lowest index), its column of the accumulated rotations, the
    remaining |a01| + |a02| + |a12| and the Frobenius norm of the input."""
    A = {(0, 0): h[0].copy(), (1, 1): h[1].copy(), (2, 2): h[2].copy(), (0, 1): h[3].copy(), (0, 2): h[4].copy(),
         (1, 2): h[5].copy()}
    one, zero = np.ones_like(h[0]), np.zeros_like(h[0])
    V = {(i, j): (one.copy() if i == j else zero.copy()) for i in range(3) for j in range(3)}
    with np.errstate(all="ignore"):
        fro = np.sqrt(h[0] ** 2 + h[1] ** 2 + h[2] ** 2 + 2 * (h[3] ** 2 + h[4] ** 2 + h[5] ** 2))
    for _ in range(sweeps):
        _rotate(A, V, 0, 1)
        _rotate(A, V, 0, 2)
        _rotate(A, V, 1, 2)
    lam = A[(0, 0)].copy()
    e = [V[(i, 0)].copy() for i in range(3)]
    for j in (1, 2):
        with np.errstate(invalid="ignore"):
            less = A[(j, j)] < lam
        lam = np.where(less, A[(j, j)], lam)
        e = [np.where(less, V[(i, j)], e[i]) for i in range(3)]
    res = np.abs(A[(0, 1)]) + np.abs(A[(0, 2)]) + np.abs(A[(1, 2)])
    return lam, e, res, fro


def nodes(vol, spacing=(1.0, 1.0, 1.0), strength=0.0, fmin=-np.inf, valley=False, sweeps=SWEEPS):
    """One volume [D,H,W] -> (operands fp32 [5,D,H,W] = e0, e1, e2, d, lam with NaN where the node is not eligible,
    cls uint8 [D,H,W])."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    D, H, W = vol.shape
    ops = np.full((5, D, H, W), np.nan, dtype=np.float32)
    cls = np.full((D, H, W), BORDER, dtype=np.uint8)
    if min(D, H, W) < 3:
        return ops, cls
    f, g, h, fin = derivatives(vol, spacing, valley)
    h = [np.where(fin, a, 0.0) for a in h]
    g = [np.where(fin, a, 0.0) for a in g]
    lam, e, _, _ = jacobi(h, sweeps)
    with np.errstate(all="ignore"):
        d = (e[0] * g[0] + e[1] * g[1]) + e[2] * g[2]
        st = np.stack([a.astype(np.float32) for a in (e[0], e[1], e[2], d, lam)])
        c = np.full(f.shape, ELIGIBLE, dtype=np.uint8)
        c[~(f >= fmin)] = LOW
        c[~(lam <= -float(strength))] = WEAK
        c[~np.isfinite(st).all(0)] = NONFINITE
        c[~fin] = NONFINITE
    st[:, c != ELIGIBLE] = np.nan
    ops[:, 1:-1, 1:-1, 1:-1] = st
    cls[1:-1, 1:-1, 1:-1] = c
    return ops, cls


def _dot(ea, eb):
    return (ea[0] * eb[0] + ea[1] * eb[1]) + ea[2] * eb[2]


def extract(operands, cls, vol=None, spacing=(1.0, 1.0, 1.0), valley=False):
    """The marching pass on the stored operands of one volume -> dict: vertices fp32 [V,3] (x, y, z), faces int32 [T,3],
    t fp64 [V], owner, edge int64 [V], face_cell int64 [T], twisted and tets (the twisted and the all-eligible
    tetrahedra), rows (int64 [D*H, 4]: per row (z, y) its vertices, triangles, twisted and all-eligible tetrahedra),
    mask uint8 [D,H,W] and, with vol, values32 / values64 [V,2] = f and lam at the vertex."""
    operands = np.asarray(operands, dtype=np.float32)
    D, H, W = cls.shape
    P = D * H * W
    el = cls == ELIGIBLE
    e = np.where(el, operands[:3], 0).astype(np.float64)
    d = np.where(el, operands[3], 0).astype(np.float64)
    sb = np.signbit(d)
    act = np.zeros((D, H, W, 7), dtype=bool)
    for n, (dz, dy, dx) in enumerate(EDGE_OFFSETS):
        a = (slice(0, D - dz), slice(0, H - dy), slice(0, W - dx))
        b = (slice(dz, D), slice(dy, H), slice(dx, W))
        flip = _dot(e[(slice(None),) + a], e[(slice(None),) + b]) < 0
        act[a + (n,)] = el[a] & el[b] & (sb[a] != (sb[b] ^ flip))
    vid = (np.cumsum(act.reshape(-1), dtype=np.int64) - 1).reshape(D, H, W, 7)
    owner, edge = np.nonzero(act.reshape(P, 7))
    z, y, x = np.unravel_index(owner, (D, H, W))
    off = np.asarray(EDGE_OFFSETS, dtype=np.int64)[edge]
    zb, yb, xb = z + off[:, 0], y + off[:, 1], x + off[:, 2]
    da, db = d[z, y, x], d[zb, yb, xb]
    flip = _dot(e[:, z, y, x], e[:, zb, yb, xb]) < 0
    db = np.where(flip, -db, db)
    with np.errstate(all="ignore"):
        den = da - db
        t = np.where(den == 0, 0.5, da / np.where(den == 0, 1.0, den))
        t = np.minimum(np.maximum(t, 0.0), 1.0)
    t32 = t.astype(np.float32)
    verts = np.empty((owner.size, 3), dtype=np.float32)
    for r, (i, dd) in enumerate(((x, off[:, 2]), (y, off[:, 1]), (z, off[:, 0]))):
        q = i.astype(np.float32) + np.where(dd != 0, t32, np.float32(0)).astype(np.float32)
        verts[:, r] = q * np.float32(spacing[r])
    res = {"vertices": verts, "t": t, "owner": owner, "edge": edge, "mask": (act * (1 << np.arange(7))).sum(-1).astype(np.uint8)}
    if vol is not None:
        f = np.asarray(vol, dtype=np.float32)
        f = -f if valley else f
        for name, dt in (("32", np.float32), ("64", np.float64)):
            tt = t32.astype(dt)
            cols = []
            for w in (f.astype(dt), operands[4].astype(dt)):
                wa, wb = w[z, y, x], w[zb, yb, xb]
                with np.errstate(all="ignore"):
                    cols.append(wa + tt * (wb - wa))
            res["values" + name] = np.stack(cols, 1).astype(dt) if owner.size else np.zeros((0, 2), dt)

    cz, cy, cx = D - 1, H - 1, W - 1
    at = lambda a, c: a[..., c[0]:c[0] + cz, c[1]:c[1] + cy, c[2]:c[2] + cx]
    faces, keys, cells = [], [], []
    rows = np.zeros((D * H, 4), dtype=np.int64)
    rows[:, 0] = np.bincount(owner // W, minlength=D * H)
    cell_row = (np.arange(cz)[:, None, None] * H + np.arange(cy)[None, :, None] + np.zeros((1, 1, cx), np.int64))
    twisted_total = tets_total = 0
    for ti, perm in enumerate(PERMS):
        C = tet_corners(perm)
        ok = at(el, C[0]) & at(el, C[1]) & at(el, C[2]) & at(el, C[3])
        ec = [at(e, c) for c in C]
        neg = {(i, j): _dot(ec[i], ec[j]) < 0 for i in range(4) for j in range(i + 1, 4)}
        sig = [np.zeros_like(ok), neg[(0, 1)], neg[(0, 2)], neg[(0, 3)]]
        tw = np.zeros_like(ok)
        for i in range(1, 4):
            for j in range(i + 1, 4):
                tw |= neg[(i, j)] != (sig[i] ^ sig[j])
        tw &= ok
        twisted_total += int(tw.sum())
        tets_total += int(ok.sum())
        rows[:, 2] += np.bincount(cell_row[tw], minlength=D * H)
        rows[:, 3] += np.bincount(cell_row[ok], minlength=D * H)
        inb = [~(at(sb, C[i]) ^ sig[i]) for i in range(4)]
        case = inb[0] * 1 + inb[1] * 2 + inb[2] * 4 + inb[3] * 8
        emit = ok & ~tw
        for cs in range(1, 15):
            idx = np.nonzero((emit & (case == cs)).reshape(-1))[0]
            if idx.size == 0:
                continue
            z0, y0, x0 = np.unravel_index(idx, (cz, cy, cx))
            cell = (z0 * H + y0) * W + x0
            for k, tri in enumerate(tet_triangles(perm, [(cs >> i) & 1 for i in range(4)])):
                cols = []
                for p, q in tri:
                    en = EDGE_NUMBER[tuple(b - a for a, b in zip(C[p], C[q]))]
                    zz, yy, xx = z0 + C[p][0], y0 + C[p][1], x0 + C[p][2]
                    assert act[zz, yy, xx, en].all(), "a used edge is not active"
                    cols.append(vid[zz, yy, xx, en])
                faces.append(np.stack(cols, 1))
                keys.append((cell * 6 + ti) * 2 + k)
                cells.append(cell)
    if faces:
        faces, keys, cells = np.concatenate(faces), np.concatenate(keys), np.concatenate(cells)
        order = np.argsort(keys, kind="stable")
        res["faces"], res["face_cell"] = faces[order].astype(np.int32), cells[order]
    else:
        res["faces"], res["face_cell"] = np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    rows[:, 1] = np.bincount(res["face_cell"] // W, minlength=D * H)
    res["rows"], res["twisted"], res["tets"] = rows, twisted_total, tets_total
    return res


def ridges(vol, spacing=(1.0, 1.0, 1.0), strength=0.0, fmin=-np.inf, valley=False):
    """nodes() then extract() of one volume; the dict of extract() plus operands and cls."""
    ops, cls = nodes(vol, spacing, strength, fmin, valley)
    res = extract(ops, cls, vol, spacing, valley)
    res["operands"], res["cls"] = ops, cls
    return res
