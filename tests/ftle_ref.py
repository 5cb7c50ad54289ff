"""numpy fp64 restatement of fs_ftle2d / fs_ftle3d (include/flowsci_hip.h "FTLE"): the difference selection, J and the
Cauchy-Green tensor with the header's operations in the header's order, vectorised over the nodes (every node's
arithmetic is independent; values computed for nodes of another class are discarded by selection).  lambda_max comes
from np.linalg.eigvalsh, not from a copy of the kernel's solver.  Imports nothing from the product."""
import numpy as np

ALIVE, OUT = 0, 1  # FS_ADV_*
NOT_VALID, OK, ENDED, NONFINITE, COLLAPSED = 0, 1, 2, 3, 4
CENTRAL, FORWARD, BACKWARD, NONE = 0, 1, 2, 3
PLANES = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))  # xx, xy, yy, xz, yz, zz


def lattice_seeds(shape, refine=1):
    """(seeds [C,P] fp32, lattice, spacing): (S_c - 1) * refine + 1 nodes per axis at the fp32 of i / refine, x fastest."""
    lattice = tuple((int(s) - 1) * refine + 1 for s in shape)
    axes = [(np.arange(n, dtype=np.float64) / refine).astype(np.float32) for n in lattice]
    mesh = np.meshgrid(*axes, indexing="ij")
    return np.stack([m.reshape(-1) for m in mesh[::-1]]), lattice, 1.0 / refine


def usable(status, accept_out=False):
    status = np.asarray(status)
    return (status == ALIVE) | ((status == OUT) if accept_out else False)


def selection(use, axis):
    """Per node the difference taken along lattice axis `axis` of the bool array `use` (shaped as the lattice):
    (kind, lo, hi) with lo / hi the offsets (-1, 0, +1) of the two nodes it reads (0, 0 where kind is NONE)."""
    u = np.moveaxis(use, axis, -1)
    um = np.zeros_like(u)
    up = np.zeros_like(u)
    um[..., 1:] = u[..., :-1]  # i - 1 exists and is usable
    up[..., :-1] = u[..., 1:]
    kind = np.where(um & up, CENTRAL, np.where(u & up, FORWARD, np.where(u & um, BACKWARD, NONE)))
    lo = np.where((kind == CENTRAL) | (kind == BACKWARD), -1, 0)
    hi = np.where((kind == CENTRAL) | (kind == FORWARD), 1, 0)
    back = lambda a: np.moveaxis(a, -1, axis)
    return back(kind), back(lo), back(hi)


def ftle(pos, status, lattice, spacing, T, valid=None, accept_out=False):
    """pos [C,P] fp32, status uint8 [P] -> dict: ftle fp32 [*lattice], cls uint8, cg fp32 [C(C+1)/2, *lattice], kinds
    ([C, *lattice], the per-axis outcome with axis 0 = x) and ftle64 (the exponent before its rounding)."""
    lattice = tuple(int(s) for s in lattice)
    C = len(lattice)
    hs = [float(v) for v in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * C
    hs = hs[::-1]  # axis 0 runs along x, the lattice's last axis
    inv_h = [1.0 / h for h in hs]
    inv_2h = [1.0 / (2.0 * h) for h in hs]
    inv_T = 1.0 / abs(float(T))
    phi = np.asarray(pos, np.float32).reshape((C,) + lattice)
    use = usable(np.asarray(status).reshape(lattice), accept_out)
    idx = np.indices(lattice)
    J = np.zeros((C, C) + lattice, np.float64)
    kinds = np.zeros((C,) + lattice, np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c in range(C):
            ax = C - 1 - c  # numpy axis of component / axis c
            kind, lo, hi = selection(use, ax)
            kinds[c] = kind
            w = np.where(kind == CENTRAL, inv_2h[c], inv_h[c])
            ilo = list(idx)
            ihi = list(idx)
            ilo[ax] = idx[ax] + lo
            ihi[ax] = idx[ax] + hi
            for r in range(C):
                a = phi[r][tuple(ihi)].astype(np.float64)
                b = phi[r][tuple(ilo)].astype(np.float64)
                J[r, c] = np.where(kind == NONE, 0.0, (a - b) * w)
        ended = (kinds == NONE).any(0)
        nonfin = ~np.isfinite(J).all((0, 1))
        NG = C * (C + 1) // 2
        G = np.zeros((NG,) + lattice, np.float64)
        for n in range(NG):
            a, b = PLANES[n]
            s2 = J[0, a] * J[0, b] + J[1, a] * J[1, b]
            G[n] = s2 + J[2, a] * J[2, b] if C == 3 else s2
        M = np.zeros(lattice + (C, C), np.float64)
        for n in range(NG):
            a, b = PLANES[n]
            M[..., a, b] = M[..., b, a] = G[n]
        good = ~(ended | nonfin)
        lam = np.zeros(lattice, np.float64)
        if good.any():
            lam[good] = np.linalg.eigvalsh(M[good])[:, -1]
        e64 = (0.5 * np.log(lam)) * inv_T
        e32 = e64.astype(np.float32)
    cls = np.where(ended, ENDED, np.where(nonfin, NONFINITE, np.where(lam == 0.0, COLLAPSED,
                                                                       np.where(np.isfinite(e32), OK, NONFINITE))))
    if valid is not None:
        cls = np.where(np.asarray(valid).reshape(lattice) != 0, cls, NOT_VALID)
    cls = cls.astype(np.uint8)
    out = np.where(cls == OK, e32, np.float32(np.nan)).astype(np.float32)
    cg = np.where((cls == OK) | (cls == COLLAPSED), G.astype(np.float32), np.float32(np.nan)).astype(np.float32)
    return {"ftle": out, "cls": cls, "cg": cg, "kinds": kinds, "ftle64": np.where(cls == OK, e64, np.nan)}
