"""The fields of the parallel-vectors tests, and their core operands (v, w, q) formed on the host from
tests/velgrad_ref.py exactly as cores.core_fields forms them on the device."""
import numpy as np

import velgrad_ref

COLUMN_AXIS = (3.3, 2.6)
RING = {"shape": (10, 14, 15), "centre": (7.2, 6.6, 4.4), "radius": 4.0, "width": 1.5}


def column(sp=(6, 7, 8)):
    """A rotating, slowly widening column around the axis x = 3.3, y = 2.6: [3, D, H, W] fp32."""
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sp], indexing="ij")
    cx, cy = COLUMN_AXIS
    return np.stack([-(y - cy) + 0.1 * (x - cx), (x - cx) + 0.1 * (y - cy), 0.7 - 0.2 * z]).astype(np.float32)


def ring():
    """A vortex ring in the plane z = 4.4 with swirl along the core and a uniform drift: [3, D, H, W] fp32."""
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in RING["shape"]], indexing="ij")
    x0, y0, z0 = RING["centre"]
    rho = np.sqrt((x - x0) ** 2 + (y - y0) ** 2)
    er = np.stack([(x - x0) / rho, (y - y0) / rho, np.zeros_like(rho)])
    ephi = np.stack([-(y - y0) / rho, (x - x0) / rho, np.zeros_like(rho)])
    ez = np.stack([np.zeros_like(rho), np.zeros_like(rho), np.ones_like(rho)])
    s, h = rho - RING["radius"], z - z0
    g = np.exp(-(s * s + h * h) / (2.0 * RING["width"] ** 2))
    return (g * (-h) * er + g * s * ez + 0.3 * g * ephi + 0.2 * ez).astype(np.float32)


def noise(seed=0, sp=(8, 8, 8), K=1):
    return np.random.default_rng(seed).standard_normal((K, 3) + tuple(sp)).astype(np.float32)


def core_fields(flows, criterion, spacing=1.0, scale=1.0):
    """(v, w, q, l2) of flows [K, 3, D, H, W]: v = (float)(u * scale); sujudi-haimes: w = (float)(J v) with the fp32 J of
    velgrad, the products summed in fp64 in the written order; levy: w = the vorticity planes."""
    flows = np.asarray(flows, np.float32)
    r = velgrad_ref.velgrad(flows, ("vort", "q", "l2", "grad"), spacing, scale)
    pl = r["planes"]
    K = flows.shape[0]
    ss = np.asarray(scale, np.float64) * np.ones(K)
    v = (flows.astype(np.float64) * ss[:, None, None, None, None]).astype(np.float32)
    if criterion == "levy":
        w = r["out"][:, pl["vort"]]
    else:
        J = r["out"][:, pl["grad"]].astype(np.float64)
        v64 = v.astype(np.float64)
        w = np.stack([(J[:, 3 * i] * v64[:, 0] + J[:, 3 * i + 1] * v64[:, 1]) + J[:, 3 * i + 2] * v64[:, 2] for i in range(3)],
                     1).astype(np.float32)
    return v, np.ascontiguousarray(w), r["out"][:, pl["q"]][:, 0], r["out"][:, pl["l2"]][:, 0]
