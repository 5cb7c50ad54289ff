"""The definition of ops.critical_points (include/flowsci_hip.h, "Critical points") restated in numpy fp64: the same
operations in the same order, so every array but vmax (a square root) is reproduced bit for bit.  Not a test module.

A cell is cut into its Kuhn simplices (3-D: six tetrahedra, one per permutation of the axes in lexicographic order;
2-D: two triangles), the field is taken as affine on each, and a simplex holds a critical point when the signed face
minors s_i = (-1)^i det(corners other than i) all have one sign: they are the barycentric coordinates of the zero up
to their sum.  A minor of a shared face is the same expression on the same nodes in both simplices, so a zero near
a face belongs to exactly one of them.
"""
import itertools

import numpy as np

CP_SPIRAL, CP_DEGENERATE, CP_MARGINAL = 4, 8, 16
MASK_DEGENERATE, MASK_NONFINITE = 64, 128


def simplices(nd):
    """[(pi, corner offsets)] of the Kuhn split: pi the permutation of the axes (x = 0, y = 1, z = 2), the corners as
    offsets (dx, dy(, dz)) from the cell's node, c0 .. c_nd."""
    out = []
    for pi in itertools.permutations(range(nd)):
        c = [np.zeros(nd, dtype=np.int64)]
        for a in pi:
            n = c[-1].copy()
            n[a] += 1
            c.append(n)
        out.append((pi, c))
    return out


def det2(a, b):
    return a[0] * b[1] - a[1] * b[0]


def det3(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0])


def signed_minors(v):
    """v: the corners' values, a list of nd + 1 sequences of nd arrays -> [s_0 .. s_nd]."""
    if len(v) == 4:
        return [det3(v[1], v[2], v[3]), -det3(v[0], v[2], v[3]), det3(v[0], v[1], v[3]), -det3(v[0], v[1], v[2])]
    return [det2(v[1], v[2]), -det2(v[0], v[2]), det2(v[0], v[1])]


def speed2(v):
    n = v[0] * v[0] + v[1] * v[1]
    return n + v[2] * v[2] if len(v) == 3 else n


def classify(inv, nd):
    """cls of the invariants [N,4] (3-D: P, Q, R, Delta; 2-D: tr, det, disc, 0)."""
    a, b, c, d = inv[:, 0], inv[:, 1], inv[:, 2], inv[:, 3]
    n = np.zeros(len(inv), dtype=np.int64)
    with np.errstate(all="ignore"):
        if nd == 3:
            P, Q, R, Delta = a, b, c, d
            PQ = P * Q
            n = np.where(R > 0, np.where((P > 0) & (PQ > R), 3, 1), n)
            n = np.where(R < 0, np.where((P < 0) & (PQ < R), 0, 2), n)
            fin = np.isfinite(P) & np.isfinite(Q) & np.isfinite(R) & np.isfinite(Delta)
            spiral, zero, marginal = Delta < 0, R == 0, PQ == R
        else:
            tr, det, disc = a, b, c
            n = np.where(det < 0, 1, n)
            n = np.where(det > 0, np.where(tr > 0, 2, 0), n)
            fin = np.isfinite(tr) & np.isfinite(det) & np.isfinite(disc)
            spiral, zero, marginal = disc < 0, det == 0, (det > 0) & (tr == 0)
    n = np.where(fin, n, 0)
    return (n | np.where(spiral, CP_SPIRAL, 0) | np.where(zero | ~fin, CP_DEGENERATE, 0) |
            np.where(marginal, CP_MARGINAL, 0)).astype(np.uint8)


def invariants(J, nd):
    """J: [N, nd, nd] fp64 -> inv [N, 4]."""
    inv = np.zeros((len(J), 4), dtype=np.float64)
    with np.errstate(all="ignore"):
        if nd == 3:
            j = lambda r, c: J[:, r, c]
            P = (j(0, 0) + j(1, 1)) + j(2, 2)
            Q = ((j(0, 0) * j(1, 1) - j(0, 1) * j(1, 0)) + (j(0, 0) * j(2, 2) - j(0, 2) * j(2, 0))) + \
                (j(1, 1) * j(2, 2) - j(1, 2) * j(2, 1))
            R = det3([j(0, 0), j(0, 1), j(0, 2)], [j(1, 0), j(1, 1), j(1, 2)], [j(2, 0), j(2, 1), j(2, 2)])
            Delta = (((((18.0 * P) * Q) * R - (4.0 * ((P * P) * P)) * R) + (P * P) * (Q * Q)) - 4.0 * ((Q * Q) * Q)) - \
                27.0 * (R * R)
            inv[:, 0], inv[:, 1], inv[:, 2], inv[:, 3] = P, Q, R, Delta
        else:
            tr = J[:, 0, 0] + J[:, 1, 1]
            det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
            inv[:, 0], inv[:, 1], inv[:, 2] = tr, det, tr * tr - 4.0 * det
    return inv


def critical_points(flows, spacing=1.0, scale=1.0, vmin=0.0):
    """flows: [K, C, *sp] fp32 (C = len(sp)), channel 0 along the last axis; spacing: one value or one per axis in the
    array's axis order; scale: one value or K.  Returns a dict of numpy arrays: cell int32 [N], simplex uint8 [N], pos
    fp32 [N, C], jac fp64 [N, C*C], inv fp64 [N, 4], cls uint8 [N], vmax fp32 [N], step int64 [N], offsets int64
    [K + 1], counts int64 [K, 4] (points, degenerate simplices, cells with a nonfinite corner, cells with a point) and
    mask uint8 [K, *sp]."""
    flows = np.asarray(flows)
    assert flows.dtype == np.float32
    K, C = flows.shape[:2]
    sp = flows.shape[2:]
    nd = len(sp)
    assert C == nd and nd in (2, 3) and min(sp) >= 2
    hs = [float(h) for h in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * nd
    ss = [float(s) for s in scale] if hasattr(scale, "__len__") else [float(scale)] * K
    inv_h = [1.0 / h for h in hs[::-1]]  # (x, y, z)
    ss = np.asarray(ss, dtype=np.float64)
    vm = float(np.float32(vmin))
    vmin2 = vm * vm
    f = flows.astype(np.float64)
    cs = tuple(s - 1 for s in sp)  # cells per axis, array order

    def corner(off):  # off = (dx, dy(, dz)) -> [C][K, *cells]
        sl = tuple(slice(off[nd - 1 - a], off[nd - 1 - a] + cs[a]) for a in range(nd))
        return [f[(slice(None), r) + sl] for r in range(C)]

    allc = [corner(off) for off in itertools.product((0, 1), repeat=nd)]
    fin = np.ones((K,) + cs, dtype=bool)
    for v in allc:
        for r in range(C):
            fin &= np.isfinite(v[r])
    sims = simplices(nd)
    NS = len(sims)
    point = np.zeros((K,) + cs + (NS,), dtype=bool)
    degen = np.zeros((K,) + cs + (NS,), dtype=bool)
    with np.errstate(all="ignore"):
        for t, (pi, offs) in enumerate(sims):
            v = [corner(o) for o in offs]
            n2 = [speed2(c) for c in v]
            quiet = np.ones((K,) + cs, dtype=bool)
            for n in n2:
                quiet &= n <= vmin2
            none = np.zeros((K,) + cs, dtype=bool)
            for r in range(C):
                allpos = np.ones((K,) + cs, dtype=bool)
                allneg = np.ones((K,) + cs, dtype=bool)
                for c in v:
                    allpos &= c[r] > 0
                    allneg &= c[r] < 0
                none |= allpos | allneg
            active = fin & ~quiet & ~none
            s = signed_minors(v)
            bad = np.zeros((K,) + cs, dtype=bool)
            pos = np.ones((K,) + cs, dtype=bool)
            neg = np.ones((K,) + cs, dtype=bool)
            for si in s:
                bad |= (si == 0) | ~np.isfinite(si)
                pos &= si > 0
                neg &= si < 0
            degen[..., t] = active & bad
            point[..., t] = active & ~bad & (pos | neg)
    mask = np.zeros((K,) + sp, dtype=np.uint8)
    inner = tuple(slice(0, c) for c in cs)
    m = np.zeros((K,) + cs, dtype=np.uint8)
    for t in range(NS):
        m |= (point[..., t].astype(np.uint8) << t)
    m |= np.where(degen.any(-1), MASK_DEGENERATE, 0).astype(np.uint8)
    m |= np.where(~fin, MASK_NONFINITE, 0).astype(np.uint8)
    mask[(slice(None),) + inner] = m
    idx = np.nonzero(point)  # ordered by step, cell (z, y, x), then t
    k, t = idx[0], idx[-1]
    coords = idx[1:-1][::-1]  # (x, y(, z))
    N = len(k)
    cell = np.zeros(N, dtype=np.int64)
    for a in range(nd):  # array order
        cell = cell * sp[a] + idx[1 + a]
    pos = np.zeros((N, nd), dtype=np.float32)
    J = np.zeros((N, nd, nd), dtype=np.float64)
    vmax = np.zeros(N, dtype=np.float32)
    for tt, (pi, offs) in enumerate(sims):
        sel = np.nonzero(t == tt)[0]
        if not len(sel):
            continue
        kk = k[sel]
        v = []
        for o in offs:
            at = tuple(coords[nd - 1 - a][sel] + o[nd - 1 - a] for a in range(nd))
            v.append([f[(kk, r) + at] for r in range(C)])
        s = signed_minors(v)
        S = s[0] + s[1]
        for si in s[2:]:
            S = S + si
        l = [si / S for si in s]
        if nd == 3:
            o = [(l[1] + l[2]) + l[3], l[2] + l[3], l[3]]
        else:
            o = [l[1] + l[2], l[2]]
        for e, a in enumerate(pi):
            pos[sel, a] = ((coords[a][sel].astype(np.float64) + o[e]) / inv_h[a]).astype(np.float32)
            for r in range(C):
                J[sel, r, a] = ((v[e + 1][r] - v[e][r]) * inv_h[a]) * ss[kk]
        n2 = speed2(v[0])
        for c in v[1:]:
            n2 = np.maximum(n2, speed2(c))
        vmax[sel] = (np.sqrt(n2) * ss[kk]).astype(np.float32)
    inv = invariants(J, nd)
    counts = np.zeros((K, 4), dtype=np.int64)
    red = tuple(range(1, nd + 1))
    counts[:, 0] = point.sum(axis=red + (nd + 1,))
    counts[:, 1] = degen.sum(axis=red + (nd + 1,))
    counts[:, 2] = (~fin).sum(axis=red)
    counts[:, 3] = point.any(-1).sum(axis=red)
    offsets = np.zeros(K + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts[:, 0])
    return {"cell": cell.astype(np.int32), "simplex": t.astype(np.uint8), "pos": pos, "jac": J.reshape(N, nd * nd),
            "inv": inv, "cls": classify(inv, nd), "vmax": vmax, "step": k.astype(np.int64), "offsets": offsets,
            "counts": counts, "mask": mask}


def class_from_eigenvalues(A):
    """(n_pos, spiral) read off numpy.linalg.eigvals of one matrix: what the class rule must agree with."""
    w = np.linalg.eigvals(np.asarray(A, dtype=np.float64))
    return int((w.real > 0).sum()), bool((np.abs(w.imag) > 0).any())


def winding_number(u):
    """The winding number of the 2-D field u [2, H, W] (component 0 along x) along the boundary nodes, counter-clockwise
    in (x, y): the sum of atan2(det2(a, b), a . b) over consecutive nodes, over 2 pi."""
    H, W = u.shape[1:]
    path = [(0, x) for x in range(W)] + [(y, W - 1) for y in range(1, H)] + \
           [(H - 1, x) for x in range(W - 2, -1, -1)] + [(y, 0) for y in range(H - 2, 0, -1)]
    vec = np.array([[u[0, y, x], u[1, y, x]] for y, x in path], dtype=np.float64)
    nxt = np.roll(vec, -1, axis=0)
    ang = np.arctan2(vec[:, 0] * nxt[:, 1] - vec[:, 1] * nxt[:, 0], (vec * nxt).sum(1))
    return ang.sum() / (2 * np.pi)
