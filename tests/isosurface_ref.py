"""numpy restatement of the isosurface definition in include/flowsci_hip.h ("Isosurfaces"): marching tetrahedra on the
Kuhn split of every cell.  Positions are formed in fp32 exactly as the header says (one rounding per operation, no fused
multiply-add); normals and values are formed twice, in fp32 and in fp64, so that a test can measure what fp32 costs
(E32) and bound the kernel by it.  The orientation of every triangle comes from the geometry of its tetrahedron (edge
midpoints against the direction from the inside corners to the outside ones), not from a copy of the kernel's table.

Not a test module: tests/test_isosurface_cpu.py checks it against invariants it does not assume, the GPU tests compare the
kernels against it."""
import itertools

import numpy as np

# the seven edges a node owns, as the (dz, dy, dx) offset of the other end: e0 .. e6
EDGE_OFFSETS = ((0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1))
EDGE_NUMBER = {off: e for e, off in enumerate(EDGE_OFFSETS)}
AXIS_OFFSET = {0: (0, 0, 1), 1: (0, 1, 0), 2: (1, 0, 0)}  # axis 0 = x (W), 1 = y, 2 = z, as (dz, dy, dx)
PERMS = tuple(itertools.permutations((0, 1, 2)))  # lexicographic: the order of a cell's six tetrahedra


def tet_corners(perm):
    """The four corners of the tetrahedron of permutation `perm`, as (dz, dy, dx) offsets from the cell's origin."""
    c0 = (0, 0, 0)
    c1 = tuple(a + b for a, b in zip(c0, AXIS_OFFSET[perm[0]]))
    c2 = tuple(a + b for a, b in zip(c1, AXIS_OFFSET[perm[1]]))
    return (c0, c1, c2, (1, 1, 1))


def tet_triangles(perm, inside):
    """The triangles of one tetrahedron whose corners c0..c3 are `inside` (4 bools): a list of triangles, each three
    (p, q) corner pairs with p < q naming the vertex on the edge between corners p and q, oriented by the geometry."""
    inside = [bool(b) for b in inside]
    n = sum(inside)
    if n in (0, 4):
        return []

    def E(p, q):
        return (min(p, q), max(p, q))

    if n in (1, 3):
        s = [i for i in range(4) if inside[i] == (n == 1)][0]
        a, b, c = [i for i in range(4) if i != s]
        tris = [[E(s, a), E(s, b), E(s, c)]]
    else:
        i0, i1 = [i for i in range(4) if inside[i]]
        o0, o1 = [i for i in range(4) if not inside[i]]
        q = [E(i0, o0), E(i0, o1), E(i1, o1), E(i1, o0)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    xyz = [np.array(c[::-1], dtype=np.float64) for c in tet_corners(perm)]
    out_c = np.mean([xyz[i] for i in range(4) if not inside[i]], axis=0)
    in_c = np.mean([xyz[i] for i in range(4) if inside[i]], axis=0)
    res = []
    for tri in tris:
        v = [(xyz[p] + xyz[q]) / 2 for p, q in tri]
        d = float(np.dot(np.cross(v[1] - v[0], v[2] - v[0]), out_c - in_c))
        assert d != 0.0, (perm, inside, tri)
        res.append(tri if d > 0 else [tri[0], tri[2], tri[1]])
    return res


def node_gradient(vol, spacing, dtype):
    """[3, D, H, W] in `dtype`: d/dx, d/dy, d/dz by central differences (f(i+1) - f(i-1)) / (2 h), one-sided
    (f(i+1) - f(i)) / h and (f(i) - f(i-1)) / h on the two boundary planes."""
    f = vol.astype(dtype)
    g = np.empty((3,) + vol.shape, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for r, ax in ((0, 2), (1, 1), (2, 0)):
            h = dtype(spacing[r])
            fm = np.moveaxis(f, ax, 0)
            gm = np.moveaxis(g[r], ax, 0)
            gm[1:-1] = (fm[2:] - fm[:-2]) / (dtype(2) * h)
            gm[0] = (fm[1] - fm[0]) / h
            gm[-1] = (fm[-1] - fm[-2]) / h
    return g


def extract(vol, iso, spacing=(1.0, 1.0, 1.0), values=None):
    """One volume [D,H,W] -> dict: vertices fp32 [V,3] (x, y, z), faces int32 [T,3], normals32 / normals64 [V,3],
    values32 / values64 [V,F] (values: [F,D,H,W] or None), t fp32 [V], owner int64 [V] (node index), edge int64 [V],
    face_cell int64 [T] (index of the cell's origin node).  spacing is (x, y, z)."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    D, H, W = vol.shape
    P = D * H * W
    iso = np.float32(iso)
    fin = np.isfinite(vol)
    with np.errstate(invalid="ignore"):
        ins = fin & (vol >= iso)
    act = np.zeros((D, H, W, 7), dtype=bool)
    for e, (dz, dy, dx) in enumerate(EDGE_OFFSETS):
        a = (slice(0, D - dz), slice(0, H - dy), slice(0, W - dx))
        b = (slice(dz, D), slice(dy, H), slice(dx, W))
        act[a + (e,)] = fin[a] & fin[b] & (ins[a] != ins[b])
    vid = (np.cumsum(act.reshape(-1), dtype=np.int64) - 1).reshape(D, H, W, 7)
    owner, edge = np.nonzero(act.reshape(P, 7))  # by node, then by edge number
    z, y, x = np.unravel_index(owner, (D, H, W))
    off = np.asarray(EDGE_OFFSETS, dtype=np.int64)[edge]
    zb, yb, xb = z + off[:, 0], y + off[:, 1], x + off[:, 2]
    fa, fb = vol[z, y, x], vol[zb, yb, xb]
    with np.errstate(over="ignore"):
        t = np.minimum(np.maximum((iso - fa) / (fb - fa), np.float32(0)), np.float32(1)).astype(np.float32)
    verts = np.empty((owner.size, 3), dtype=np.float32)
    for r, (i, d) in enumerate(((x, off[:, 2]), (y, off[:, 1]), (z, off[:, 0]))):
        q = i.astype(np.float32) + np.where(d != 0, t, np.float32(0)).astype(np.float32)
        verts[:, r] = q * np.float32(spacing[r])
    res = {"vertices": verts, "t": t, "owner": owner, "edge": edge}

    for name, dt in (("32", np.float32), ("64", np.float64)):
        g = node_gradient(vol, spacing, dt)
        tt = t.astype(dt)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ga, gb = g[:, z, y, x], g[:, zb, yb, xb]
            G = (ga + tt * (gb - ga)).T
            ln = np.sqrt((G * G).sum(1, dtype=dt))
            ok = np.isfinite(ln) & (ln > 0)
            n = np.where(ok[:, None], -G / np.where(ok, ln, 1)[:, None], 0)
        res["normals" + name] = n.astype(dt)
        if values is not None:
            w = np.asarray(values, dtype=np.float32).astype(dt)
            wa, wb = w[:, z, y, x], w[:, zb, yb, xb]
            with np.errstate(invalid="ignore", over="ignore"):
                res["values" + name] = (wa + tt * (wb - wa)).T.astype(dt)

    cz, cy, cx = D - 1, H - 1, W - 1
    ok = np.ones((cz, cy, cx), dtype=bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        ok &= fin[dz:dz + cz, dy:dy + cy, dx:dx + cx]
    faces, keys, cells = [], [], []
    for ti, perm in enumerate(PERMS):
        C = tet_corners(perm)
        inb = [ins[c[0]:c[0] + cz, c[1]:c[1] + cy, c[2]:c[2] + cx] for c in C]
        case = inb[0] * 1 + inb[1] * 2 + inb[2] * 4 + inb[3] * 8
        for cs in range(1, 15):
            idx = np.nonzero((ok & (case == cs)).reshape(-1))[0]
            if idx.size == 0:
                continue
            z0, y0, x0 = np.unravel_index(idx, (cz, cy, cx))
            cell = (z0 * H + y0) * W + x0
            for k, tri in enumerate(tet_triangles(perm, [(cs >> i) & 1 for i in range(4)])):
                cols = []
                for p, q in tri:
                    e = EDGE_NUMBER[tuple(b - a for a, b in zip(C[p], C[q]))]
                    zz, yy, xx = z0 + C[p][0], y0 + C[p][1], x0 + C[p][2]
                    assert act[zz, yy, xx, e].all()
                    cols.append(vid[zz, yy, xx, e])
                faces.append(np.stack(cols, 1))
                keys.append((cell * 6 + ti) * 2 + k)
                cells.append(cell)
    if faces:
        faces, keys, cells = np.concatenate(faces), np.concatenate(keys), np.concatenate(cells)
        order = np.argsort(keys, kind="stable")
        res["faces"], res["face_cell"] = faces[order].astype(np.int32), cells[order]
    else:
        res["faces"], res["face_cell"] = np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    return res


def extract_series(vols, iso, spacing=(1.0, 1.0, 1.0), values=None):
    """K volumes -> the concatenated arrays of extract() plus vertex_offsets and face_offsets (int64 [K+1])."""
    parts = [extract(v, iso, spacing, None if values is None else values[k]) for k, v in enumerate(vols)]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["vertex_offsets"] = np.concatenate([[0], np.cumsum([p["vertices"].shape[0] for p in parts])]).astype(np.int64)
    out["face_offsets"] = np.concatenate([[0], np.cumsum([p["faces"].shape[0] for p in parts])]).astype(np.int64)
    return out


def topology(faces, n_vertices):
    """Of an indexed triangle mesh: dict with edges (undirected edges), bad_edges (edges that are not used by exactly two
    faces in opposite directions), used_vertices, and euler = used_vertices - edges + faces."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * max(int(n_vertices), 1) + hi
    sign = np.where(a < b, 1, -1)
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    net = np.zeros(uk.size, dtype=np.int64)
    np.add.at(net, inv, sign)
    used = np.unique(f).size
    return {"edges": int(uk.size), "bad_edges": int(((cnt != 2) | (net != 0)).sum()), "used_vertices": int(used),
            "euler": int(used - uk.size + f.shape[0]), "degenerate": int((a == b).sum())}


def area_volume(vertices, faces):
    """(area, signed enclosed volume) in fp64: sum |(v1-v0) x (v2-v0)| / 2 and sum v0 . (v1 x v2) / 6."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.sqrt((np.cross(v1 - v0, v2 - v0) ** 2).sum(1)).sum()
    vol = (v0 * np.cross(v1, v2)).sum() / 6.0
    return float(area), float(vol)


# ---- the fields of the tests, on integer node coordinates, cast to fp32 ----
def _grid(shape):
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64),
                          indexing="ij")
    return x, y, z


def sphere_field(n=16, scale=1.0):
    x, y, z = _grid((n, n, n))
    c, r = (7.4 * scale, 7.6 * scale, 7.2 * scale), 5.3 * scale
    return (r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32), r


def torus_field():
    x, y, z = _grid((12, 24, 28))
    return (2.6 - np.sqrt((np.sqrt((x - 13.3) ** 2 + (y - 11.6) ** 2) - 6.2) ** 2 + (z - 5.4) ** 2)).astype(np.float32)


def two_balls_field():
    x, y, z = _grid((12, 12, 24))
    d1 = 3.7 - np.sqrt((x - 5.6) ** 2 + (y - 5.4) ** 2 + (z - 5.3) ** 2)
    d2 = 3.4 - np.sqrt((x - 17.3) ** 2 + (y - 6.2) ** 2 + (z - 5.8) ** 2)
    return np.maximum(d1, d2).astype(np.float32)


def integer_field():
    x, y, z = _grid((10, 10, 10))
    return (9.0 - ((x - 5) ** 2 + (y - 5) ** 2 + (z - 4) ** 2)).astype(np.float32)
