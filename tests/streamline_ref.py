"""numpy fp64 restatement of fs_streamlines2d / fs_streamlines3d (include/flowsci_hip.h "Streamlines"): the same
operations in the same order.  Two forms of the one rule:

  streamline(...)   one line, scalar loops over steps, stages, corners and components on Python floats (IEEE fp64: every
                    product and sum is rounded once, math.sqrt and / are correctly rounded, nothing is fused).  This is
                    the statement of the rule.
  streamlines(...)  all S lines at once, vectorised over the lines on advect_ref.sample / classify and lic_ref.direction
                    (every line's arithmetic is independent, and what is computed for a line that has ended is discarded
                    by selection, so the vector form gives each line exactly the scalar chain).  It is what the large
                    comparisons run on; test_streamline_cpu.py holds the two to the same bits.

Imports nothing from the product."""
import math

import numpy as np

from advect_ref import ALIVE, classify, extents
from lic_ref import direction

FULL, OUT, STAGNANT, NONFINITE, CAPTURED, INVALID = 0, 1, 2, 3, 4, 5
EULER, RK2, RK4 = "euler", "rk2", "rk4"
END_NAMES = ("full", "out", "stagnant", "nonfinite", "captured", "invalid")


def _sample1(field, S, q):
    """field [C, n] fp64 (flattened planes), q a list of C floats -> list of C floats: the sample of one point."""
    C = len(q)
    if not all(math.isfinite(v) for v in q):
        return [math.nan] * C
    f, g, o0, o1 = [], [], [], []
    stride = 1
    for c in range(C):
        qc = 0.0 if q[c] < 0.0 else q[c]
        hi = float(S[c] - 1)
        qc = hi if qc > hi else qc
        fl = math.floor(qc)
        i0 = int(fl)
        i1 = min(i0 + 1, S[c] - 1)
        fc = qc - fl
        f.append(fc)
        g.append(1.0 - fc)
        o0.append(i0 * stride)
        o1.append(i1 * stride)
        stride *= S[c]
    acc = [0.0] * C
    for k in range(1 << C):
        b = [(k >> c) & 1 for c in range(C)]
        t = [f[c] if b[c] else g[c] for c in range(C)]
        wt = (t[2] * t[1]) * t[0] if C == 3 else t[1] * t[0]
        o = sum((o1[c] if b[c] else o0[c]) for c in range(C))
        for c in range(C):
            acc[c] = acc[c] + wt * float(field[c][o])
    return acc


def _dir1(field, S, q, vmin):
    """(d, code) of one point."""
    v = _sample1(field, S, q)
    if not all(math.isfinite(x) for x in v):
        return None, NONFINITE
    n2 = v[0] * v[0] + v[1] * v[1]
    if len(v) == 3:
        n2 = n2 + v[2] * v[2]
    n = math.sqrt(n2)  # (an overflowed sum: sqrt(inf) = inf > vmin, and v / inf below)
    if not n > vmin:
        return None, STAGNANT
    return [x / n for x in v], FULL


def _classify1(p, S):
    if not all(math.isfinite(v) for v in p):
        return NONFINITE
    for c in range(len(p)):
        if p[c] < 0.0 or p[c] > float(S[c] - 1):
            return OUT
    return ALIVE


def streamline(flows, seed, step, sign, home, capture, M, h, vmin=0.0, method=RK4, positions=None):
    """One line.  flows [K,C,*sp] fp32, seed C floats (x first), capture [K, plane] uint8 or None, home an int or None
    -> (verts fp32 [length+1, C], length, end, hit).  positions: a list that receives the fp64 position of every stored
    slot after slot 0 (what the line is integrated on; the vertices are its fp32 roundings)."""
    flows = np.asarray(flows, np.float32)
    K, C = flows.shape[:2]
    S = extents(flows[0])
    seed = [float(v) for v in seed]
    verts = [np.array(seed, np.float64).astype(np.float32)]
    hit, length = -1, 0
    hm = -1 if home is None else int(home)
    left = hm < 0
    k = int(step)
    if k < 0 or k >= K:
        return np.stack(verts), 0, INVALID, -1
    c0 = _classify1(seed, S)
    if c0 != ALIVE:
        return np.stack(verts), 0, (OUT if c0 == OUT else NONFINITE), -1
    field = flows[k].reshape(C, -1).astype(np.float64)
    h = float(h)
    hs, hh, h6 = h, 0.5 * h, h / 6.0
    if sign < 0:
        hs, hh, h6 = -hs, -hh, -h6
    p = seed
    end = FULL
    for i in range(1, M + 1):
        d1, code = _dir1(field, S, p, vmin)
        if code == FULL:
            if method == EULER:
                pn = [p[c] + hs * d1[c] for c in range(C)]
            elif method == RK2:
                d, code = _dir1(field, S, [p[c] + hh * d1[c] for c in range(C)], vmin)
                if code == FULL:
                    pn = [p[c] + hs * d[c] for c in range(C)]
            elif method == RK4:
                d2, code = _dir1(field, S, [p[c] + hh * d1[c] for c in range(C)], vmin)
                if code == FULL:
                    d3, code = _dir1(field, S, [p[c] + hh * d2[c] for c in range(C)], vmin)
                if code == FULL:
                    d4, code = _dir1(field, S, [p[c] + hs * d3[c] for c in range(C)], vmin)
                if code == FULL:
                    pn = [p[c] + h6 * (((d1[c] + 2.0 * d2[c]) + 2.0 * d3[c]) + d4[c]) for c in range(C)]
            else:
                raise ValueError(method)
        if code != FULL:
            end = code
            break
        if _classify1(pn, S) != ALIVE:
            end = OUT
            break
        p = pn
        verts.append(np.array(p, np.float64).astype(np.float32))
        if positions is not None:
            positions.append(list(p))
        length = i
        cell = [min(int(math.floor(p[c])), S[c] - 2) for c in range(C)]
        ci = ((cell[2] * S[1] + cell[1]) if C == 3 else cell[1]) * S[0] + cell[0]
        if ci != hm:
            left = True
        if capture is not None and left and capture[k][ci] != 0:
            end = CAPTURED
            hit = ci
            break
    return np.stack(verts), length, end, hit


def streamlines(flows, seeds, step, sign, home=None, capture=None, M=256, h=0.5, vmin=0.0, method=RK4):
    """All lines.  flows [K,C,*sp] fp32, seeds fp64 [C,S] (x first), step int [S], sign int [S], home int [S] or None,
    capture uint8 [K,*sp] or None -> (verts fp32 [M+1,C,S], NaN beyond a line's length; length int32 [S]; end uint8 [S];
    hit int32 [S])."""
    flows = np.asarray(flows, np.float32)
    seeds = np.asarray(seeds, np.float64)
    K, C = flows.shape[:2]
    Sx = extents(flows[0])
    n = seeds.shape[1]
    step = np.asarray(step, np.int64)
    back = np.asarray(sign, np.int64) < 0
    hm = np.full(n, -1, np.int64) if home is None else np.asarray(home, np.int64)
    cap = None if capture is None else np.asarray(capture).reshape(K, -1)
    verts = np.full((M + 1, C, n), np.nan, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        verts[0] = seeds.astype(np.float32)
    length = np.zeros(n, np.int32)
    end = np.zeros(n, np.uint8)
    hit = np.full(n, -1, np.int32)
    valid = (step >= 0) & (step < K)
    end[~valid] = INVALID
    c0 = classify(seeds, Sx)
    end[valid & (c0 == 1)] = OUT        # advect_ref.OUT
    end[valid & (c0 == 2)] = NONFINITE  # advect_ref.NONFINITE
    started = valid & (c0 == ALIVE)
    h = float(h)
    for k in range(K):
        idx = np.nonzero(started & (step == k))[0]
        if not len(idx):
            continue
        field = flows[k]
        hs = np.where(back[idx], -h, h)
        hh = np.where(back[idx], -(0.5 * h), 0.5 * h)
        h6 = np.where(back[idx], -(h / 6.0), h / 6.0)
        p = seeds[:, idx].copy()
        live = np.ones(len(idx), bool)
        left = hm[idx] < 0
        e = np.zeros(len(idx), np.uint8)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for i in range(1, M + 1):
                if not live.any():
                    break

                def stage(q, code):
                    d, c2 = direction(field, q, vmin)
                    return np.where(c2 == FULL, d, 0.0), np.where(code != FULL, code, c2).astype(np.uint8)

                d1, code = stage(p, np.zeros(len(idx), np.uint8))
                if method == EULER:
                    pn = p + hs * d1
                elif method == RK2:
                    d, code = stage(p + hh * d1, code)
                    pn = p + hs * d
                elif method == RK4:
                    d2, code = stage(p + hh * d1, code)
                    d3, code = stage(p + hh * d2, code)
                    d4, code = stage(p + hs * d3, code)
                    pn = p + h6 * (((d1 + 2.0 * d2) + 2.0 * d3) + d4)
                else:
                    raise ValueError(method)
                ok = code == FULL
                inside = classify(pn, Sx) == ALIVE
                code = np.where(ok & ~inside, OUT, code).astype(np.uint8)
                e = np.where(live, code, e).astype(np.uint8)
                live = live & (code == FULL)
                p = np.where(live, pn, p)
                verts[i][:, idx[live]] = p[:, live].astype(np.float32)
                length[idx[live]] = i
                cell = [np.minimum(np.floor(p[c]).astype(np.int64), Sx[c] - 2) for c in range(C)]
                ci = ((cell[2] * Sx[1] + cell[1]) if C == 3 else cell[1]) * Sx[0] + cell[0]
                left = left | (live & (ci != hm[idx]))
                if cap is not None:
                    got = live & left & (cap[k][ci] != 0)
                    e = np.where(got, CAPTURED, e).astype(np.uint8)
                    hit[idx[got]] = ci[got]
                    live = live & ~got
        end[idx] = e  # (a line still live after M steps holds FULL = 0)
    return verts, length, end, hit
