"""numpy fp64 restatement of fs_advect2d / fs_advect3d (include/flowsci_hip.h "Pathlines"): the same operations in the
same order, vectorised over the particles (every particle's arithmetic is independent, and results computed for a
particle that has ended are discarded by selection, so the vector form gives each particle exactly the scalar chain).
Imports nothing from the product."""
import numpy as np

ALIVE, OUT, NONFINITE = 0, 1, 2
EULER, RK2, RK4 = "euler", "rk2", "rk4"


def extents(field):
    """S_c of a [C,*sp] field: component 0 runs along the LAST axis (W)."""
    return [int(s) for s in field.shape[1:]][::-1]


def sample(field, q):
    """field [C,*sp] fp32, q [C,P] fp64 -> velocity [C,P] fp64."""
    C = field.shape[0]
    S = extents(field)
    P = q.shape[1]
    fin = np.isfinite(q).all(0)
    strides = [1]
    for c in range(C - 1):
        strides.append(strides[-1] * S[c])
    f, g, o0, o1 = [], [], [], []
    for c in range(C):
        qc = np.where(fin, q[c], 0.0)
        qc = np.where(qc < 0.0, 0.0, qc)
        qc = np.where(qc > float(S[c] - 1), float(S[c] - 1), qc)
        fl = np.floor(qc)
        i0 = fl.astype(np.int64)
        i1 = np.minimum(i0 + 1, S[c] - 1)
        fc = qc - fl
        f.append(fc)
        g.append(1.0 - fc)
        o0.append(i0 * strides[c])
        o1.append(i1 * strides[c])
    flat = field.reshape(C, -1).astype(np.float64)
    acc = np.zeros((C, P), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1 << C):
            b = [(k >> c) & 1 for c in range(C)]  # b[0] = bx, b[1] = by, b[2] = bz
            t = [f[c] if b[c] else g[c] for c in range(C)]
            wt = (t[2] * t[1]) * t[0] if C == 3 else t[1] * t[0]
            o = sum((o1[c] if b[c] else o0[c]) for c in range(C))
            for c in range(C):
                acc[c] = acc[c] + wt * flat[c][o]
    acc[:, ~fin] = np.nan
    return acc


def classify(p, S):
    """p [C,P] fp64 -> uint8 [P]."""
    fin = np.isfinite(p).all(0)
    out = np.zeros(p.shape[1], bool)
    with np.errstate(invalid="ignore"):
        for c in range(p.shape[0]):
            out |= (p[c] < 0.0) | (p[c] > float(S[c] - 1))
    return np.where(~fin, NONFINITE, np.where(out, OUT, ALIVE)).astype(np.uint8)


def advect(pos, flows, status=None, steps=None, method=EULER, substeps=1, scale=1.0):
    """pos [C,P] fp32, flows [K,C,*sp] fp32 -> (traj [K,C,P] fp32, status uint8 [P], steps int32 [P])."""
    pos = np.asarray(pos, np.float32)
    flows = np.asarray(flows, np.float32)
    K, C = flows.shape[:2]
    P = pos.shape[1]
    S = extents(flows[0])
    st = np.zeros(P, np.uint8) if status is None else np.array(status, np.uint8)
    n = np.zeros(P, np.int32) if steps is None else np.array(steps, np.int32)
    hs = float(scale) / float(substeps)
    hh = 0.5 * hs
    h6 = hs / 6.0
    traj = np.empty((K, C, P), np.float32)
    pf = pos.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            p = pf.astype(np.float64)
            st = np.where(st == ALIVE, classify(p, S), st).astype(np.uint8)
            moving = st == ALIVE  # the particles whose position this step rounds again (exact where nothing moved)
            for _ in range(substeps):
                alive = st == ALIVE
                if not alive.any():
                    break
                k1 = sample(flows[k], p)
                if method == EULER:
                    pn = p + hs * k1
                elif method == RK2:
                    k2 = sample(flows[k], p + hh * k1)
                    pn = p + hs * k2
                elif method == RK4:
                    k2 = sample(flows[k], p + hh * k1)
                    k3 = sample(flows[k], p + hh * k2)
                    k4 = sample(flows[k], p + hs * k3)
                    pn = p + h6 * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
                else:
                    raise ValueError(method)
                cn = classify(pn, S)
                p = np.where(alive & (cn != NONFINITE), pn, p)
                st = np.where(alive, cn, st).astype(np.uint8)
            n = n + (moving & (st == ALIVE)).astype(np.int32)
            pf = np.where(moving, p.astype(np.float32), pf)
            traj[k] = pf
    return traj, st, n
