"""A numpy / plain-Python restatement of the region ops (include/flowsci_hip.h "Regions"): sequential union-find
labelling canonicalised to "1 + smallest linear index", the table through np.add.at / np.minimum.at in int64 / fp64,
follow through np.float32 addition and np.rint, links through np.unique.  No scipy."""
import itertools

import numpy as np

REGION_OUT, REGION_TO_BACKGROUND = -1, -2


def foreground(mask, require=1, reject=128):
    m = np.asarray(mask).astype(np.int64)
    return ((m & require) == require) & ((m & reject) == 0)


def _earlier(nd, full):
    """Offsets of the half-neighbourhood that precedes a node in row-major order."""
    offs = []
    for o in itertools.product((-1, 0, 1), repeat=nd):
        if o >= (0,) * nd:
            continue
        if not full and sum(abs(v) for v in o) != 1:
            continue
        offs.append(o)
    return offs


def label_one(fg, full):
    """Labels of one boolean map: int32, background 0, 1 + the smallest linear index of the component."""
    fg = np.asarray(fg, dtype=bool)
    sp, nd = fg.shape, fg.ndim
    P = fg.size
    idx = np.arange(P, dtype=np.int64).reshape(sp)
    parent = np.arange(P, dtype=np.int64)

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    for o in _earlier(nd, full):
        # the nodes x and x + o that both exist
        a_sl = tuple(slice(max(0, -v), s - max(0, v)) for v, s in zip(o, sp))
        b_sl = tuple(slice(max(0, v), s - max(0, -v)) for v, s in zip(o, sp))
        both = fg[a_sl] & fg[b_sl]
        for a, b in zip(idx[a_sl][both].tolist(), idx[b_sl][both].tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                if ra < rb:
                    parent[rb] = ra
                else:
                    parent[ra] = rb
    flat = fg.reshape(-1)
    out = np.zeros(P, dtype=np.int32)
    for i in np.nonzero(flat)[0].tolist():
        out[i] = find(i) + 1  # the root is the smallest index: parents only ever point downwards
    return out.reshape(sp)


def label_regions(mask, require=1, reject=128, full=False):
    """(labels int32 [K,*sp], n_regions int32 [K]) of a uint8 stack."""
    fg = foreground(mask, require, reject)
    labels = np.stack([label_one(f, full) for f in fg])
    K = labels.shape[0]
    ramp = np.arange(1, labels[0].size + 1, dtype=np.int64).reshape(labels.shape[1:])
    n = np.array([int((labels[k] == ramp).sum()) for k in range(K)], dtype=np.int32)
    return labels, n


def canonical(labels):
    """Any labelling of one map (0 = background) renamed to 1 + the smallest linear index of each label."""
    flat = np.asarray(labels).reshape(-1).astype(np.int64)
    out = np.zeros(flat.size, dtype=np.int32)
    idx = np.nonzero(flat)[0]
    if idx.size:
        first = np.full(int(flat.max()) + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat[idx], idx)
        out[idx] = first[flat[idx]] + 1
    return out.reshape(np.asarray(labels).shape)


def ranks(labels):
    """(dense id per node int64 [K,*sp] (-1 on background), offsets int64 [K+1]): ids in increasing label order."""
    K = labels.shape[0]
    dense = np.full(labels.shape, -1, dtype=np.int64)
    offsets = np.zeros(K + 1, dtype=np.int64)
    for k in range(K):
        u = np.unique(labels[k][labels[k] > 0])
        offsets[k + 1] = offsets[k] + u.size
        if u.size:
            dense[k][labels[k] > 0] = np.searchsorted(u, labels[k][labels[k] > 0])
    return dense, offsets


def _key(v):
    """fp32 <-> int32 with the same order (an involution on the bit patterns)."""
    b = np.ascontiguousarray(v).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7fffffff)).astype(np.int32)


def region_table(labels, weights=None):
    """The table's columns over R rows: step, label, count, coord_sum (int64 [R,nd]), bbox (int32 [R,2,nd]), offsets, and
    with weights wsum (fp64 [R,F]), wabs (the sum of |w|, for the summation bound), wmin, wmax (fp32 [R,F])."""
    K, nd = labels.shape[0], labels.ndim - 1
    dense, offsets = ranks(labels)
    R = int(offsets[-1])
    tab = {"step": np.zeros(R, np.int32), "label": np.zeros(R, np.int32), "count": np.zeros(R, np.int64),
           "coord_sum": np.zeros((R, nd), np.int64), "bbox": np.zeros((R, 2, nd), np.int32), "offsets": offsets}
    tab["bbox"][:, 0] = np.iinfo(np.int32).max
    tab["bbox"][:, 1] = np.iinfo(np.int32).min
    F = 0 if weights is None else weights.shape[1]
    if F:
        tab.update(wsum=np.zeros((R, F)), wabs=np.zeros((R, F)), wmin=np.full((R, F), np.inf, np.float32),
                   wmax=np.full((R, F), -np.inf, np.float32))
    for k in range(K):
        fg = labels[k] > 0
        rows = offsets[k] + dense[k][fg]
        tab["step"][offsets[k]:offsets[k + 1]] = k
        tab["label"][offsets[k]:offsets[k + 1]] = np.unique(labels[k][fg])
        np.add.at(tab["count"], rows, 1)
        for a, c in enumerate(np.nonzero(fg)):
            np.add.at(tab["coord_sum"][:, a], rows, c)
            np.minimum.at(tab["bbox"][:, 0, a], rows, c.astype(np.int32))
            np.maximum.at(tab["bbox"][:, 1, a], rows, c.astype(np.int32))
        for f in range(F):
            w = weights[k, f][fg]
            np.add.at(tab["wsum"][:, f], rows, w.astype(np.float64))
            np.add.at(tab["wabs"][:, f], rows, np.abs(w.astype(np.float64)))
            # through the order-preserving integer image of fp32 (-0 below +0), as the header defines the extrema
            key = _key(w)
            kmin = np.full(R, np.iinfo(np.int32).max, np.int32)
            kmax = np.full(R, np.iinfo(np.int32).min, np.int32)
            np.minimum.at(kmin, rows, key)
            np.maximum.at(kmax, rows, key)
            sel = slice(int(offsets[k]), int(offsets[k + 1]))
            tab["wmin"][sel, f] = _key(kmin[sel]).view(np.float32)
            tab["wmax"][sel, f] = _key(kmax[sel]).view(np.float32)
    return tab


def follow(labels, flows):
    """dst int32 [K-1,*sp]: np.float32 addition, np.rint, float comparisons before any conversion."""
    K, sp = labels.shape[0], labels.shape[1:]
    nd = len(sp)
    dst = np.zeros((K - 1,) + sp, dtype=np.int32)
    coords = np.indices(sp)
    for j in range(K - 1):
        inside = np.ones(sp, dtype=bool)
        tgt = []
        for a in range(nd):  # tensor axis a is flow channel nd - 1 - a
            with np.errstate(invalid="ignore", over="ignore"):
                r = np.rint(coords[a].astype(np.float32) + flows[j, nd - 1 - a].astype(np.float32))
                ok = (r >= np.float32(0)) & (r <= np.float32(sp[a] - 1))
            inside &= ok
            tgt.append(np.where(ok, r, 0).astype(np.int64))
        L = labels[j + 1][tuple(tgt)]
        d = np.where(inside, np.where(L > 0, L, REGION_TO_BACKGROUND), REGION_OUT)
        dst[j] = np.where(labels[j] > 0, d, 0)
    return dst


def links(labels, dst):
    """Per step pair: src, dst (dense ids), count, n_out, n_to_background -- the rows sorted by (src, dst)."""
    dense, offsets = ranks(labels)
    out = []
    for j in range(labels.shape[0] - 1):
        R = int(offsets[j + 1] - offsets[j])
        fg = labels[j] > 0
        s = dense[j][fg]
        d = dst[j][fg].astype(np.int64)
        n_out = np.bincount(s[d == REGION_OUT], minlength=R).astype(np.int64)
        n_bg = np.bincount(s[d == REGION_TO_BACKGROUND], minlength=R).astype(np.int64)
        to = d > 0
        nxt = dense[j + 1].reshape(-1)[d[to] - 1]
        pairs = np.stack([s[to], nxt], 1) if to.any() else np.zeros((0, 2), np.int64)
        u, c = np.unique(pairs, axis=0, return_counts=True) if pairs.shape[0] else (pairs, np.zeros(0, np.int64))
        out.append({"src": u[:, 0].astype(np.int64), "dst": u[:, 1].astype(np.int64), "count": c.astype(np.int64),
                    "n_out": n_out, "n_to_background": n_bg})
    return out


# ---- patterns ----------------------------------------------------------------------------------------------------------
def serpentine(sp):
    """One component threaded through the whole grid: every second row full, joined alternately at the right and the
    left end; in 3-D every second plane, joined alternately at the last and the first row."""
    m = np.zeros(sp, dtype=bool)
    if len(sp) == 2:
        H, W = sp
        m[0::2] = True
        for n, y in enumerate(range(1, H, 2)):
            if y + 1 < H:
                m[y, W - 1 if n % 2 == 0 else 0] = True
        return m
    D, H, W = sp
    for n, z in enumerate(range(0, D, 2)):
        m[z] = serpentine((H, W))
        if z + 2 < D:
            # the plane's path ends where its last full row ends; bridge from a node of the path to the next plane
            m[z + 1, 0 if n % 2 else 2 * ((H - 1) // 2), 0] = True
    return m


def comb(sp):
    m = np.zeros(sp, dtype=bool)
    m[..., 0, :] = True
    m[..., :, 0::2] = True
    return m


def diagonal(sp):
    m = np.zeros(sp, dtype=bool)
    n = min(sp)
    m[tuple(np.arange(n) for _ in sp)] = True
    return m


def rings(sp):
    """Nested box outlines two nodes apart: separate under either connectivity."""
    c = np.indices(sp)
    d = np.min([np.minimum(c[a], sp[a] - 1 - c[a]) for a in range(len(sp))], axis=0)
    return d % 3 == 0


def checkerboard(sp):
    return np.indices(sp).sum(0) % 2 == 0


def random_fill(sp, p, seed):
    return np.random.default_rng(seed).random(sp) < p


def discs(sp, centres, radius):
    c = np.indices(sp).astype(np.float64)
    m = np.zeros(sp, dtype=bool)
    for ctr in centres:
        m |= sum((c[a] - ctr[a]) ** 2 for a in range(len(sp))) <= radius * radius
    return m
