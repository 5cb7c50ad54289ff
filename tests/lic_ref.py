"""numpy fp64 restatement of fs_lic2d / fs_lic3d (include/flowsci_hip.h "Line integral convolution"): the same
operations in the same order, vectorised over the nodes (every node's arithmetic is independent, and what is computed
for a side that has ended is discarded by selection, so the vector form gives each node exactly the scalar chain).
`sample` and `classify` are advect_ref's: the rule shares them word for word.  Imports nothing from the product."""
import numpy as np

from advect_ref import ALIVE, classify, extents, sample

FULL, OUT, STAGNANT, NONFINITE = 0, 1, 2, 3
EULER, RK2 = "euler", "rk2"


def tsample(tex, q):
    """tex [*sp] fp32, q [C,P] fp64 -> [P] fp64: advect_ref.sample on a field of C identical planes (its channel count
    is the field's), of which one is kept."""
    C = q.shape[0]
    return sample(np.broadcast_to(tex, (C,) + tex.shape), q)[0]


def direction(field, q, vmin):
    """(d [C,P] fp64, code uint8 [P]): FULL where d is the unit vector of sample(field, q)."""
    v = sample(field, q)
    C = v.shape[0]
    fin = np.isfinite(v).all(0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n2 = v[0] * v[0] + v[1] * v[1]
        if C == 3:
            n2 = n2 + v[2] * v[2]
        n = np.sqrt(n2)
        moving = n > vmin
        d = v / n
    code = np.where(~fin, NONFINITE, np.where(~moving, STAGNANT, FULL)).astype(np.uint8)
    return d, code


def hann(L):
    """w[i] = 0.5 (1 + cos(pi i / (L + 1))), i = 0..L."""
    return np.array([0.5 * (1.0 + np.cos(np.pi * i / (L + 1))) for i in range(L + 1)], np.float64)


def box(L):
    return np.ones(L + 1, np.float64)


def lic_field(field, tex, w, h, vmin=0.0, method=RK2):
    """field [C,*sp] fp32, tex [*sp] fp32, w fp64 [L+1] -> (out fp32 [*sp], ends uint8 [*sp], count int32 [*sp])."""
    field = np.asarray(field, np.float32)
    tex = np.asarray(tex, np.float32)
    w = np.asarray(w, np.float64)
    C, sp = field.shape[0], field.shape[1:]
    S = extents(field)
    L = len(w) - 1
    axes = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sp], indexing="ij")
    node = np.stack([a.reshape(-1) for a in axes[::-1]], 0)  # component 0 = x
    P = node.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = w[0] * tsample(tex, node)
        wsum = np.full(P, w[0], np.float64)
        count = np.ones(P, np.int32)
        ends = np.zeros(P, np.uint8)
        for side, s in enumerate((1.0, -1.0)):
            hs = s * float(h)
            hh = 0.5 * hs
            p = node.copy()
            A = np.zeros(P, np.float64)
            Wt = np.zeros(P, np.float64)
            n = np.zeros(P, np.int32)
            end = np.zeros(P, np.uint8)
            live = np.ones(P, bool)
            for i in range(1, L + 1):
                if not live.any():
                    break
                d, code = direction(field, p, vmin)
                if method == RK2:
                    d2, code2 = direction(field, p + hh * np.where(code == FULL, d, 0.0), vmin)
                    d = d2
                    code = np.where(code != FULL, code, code2).astype(np.uint8)
                elif method != EULER:
                    raise ValueError(method)
                ok = code == FULL
                pn = p + hs * np.where(ok, d, 0.0)
                inside = classify(pn, S) == ALIVE
                code = np.where(ok & ~inside, OUT, code).astype(np.uint8)
                end = np.where(live, code, end).astype(np.uint8)
                live = live & (code == FULL)
                p = np.where(live, pn, p)
                t = tsample(tex, p)
                A = np.where(live, A + w[i] * t, A)
                Wt = np.where(live, Wt + w[i], Wt)
                n = n + live.astype(np.int32)
            acc = acc + A
            wsum = wsum + Wt
            count = count + n
            ends = ends | (end << (2 * side)).astype(np.uint8)
        out = (acc / wsum).astype(np.float32)
    return out.reshape(sp), ends.reshape(sp), count.reshape(sp)


def lic(flows, tex, w, h, vmin=0.0, method=RK2):
    """flows [K,C,*sp], tex [*sp] or [K,*sp] -> (out [K,*sp] fp32, ends [K,*sp] uint8, count [K,*sp] int32)."""
    flows = np.asarray(flows, np.float32)
    tex = np.asarray(tex, np.float32)
    K = flows.shape[0]
    per_step = tex.ndim == flows.ndim - 1
    res = [lic_field(flows[k], tex[k] if per_step else tex, w, h, vmin, method) for k in range(K)]
    return tuple(np.stack([r[j] for r in res]) for j in range(3))
