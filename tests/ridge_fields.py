"""The scalar volumes of the ridge tests, on integer node coordinates, cast to fp32: FIELDS maps a name to
(builder, strength, fmin); a builder returns (volume [D,H,W], what the analytic ridge is).  The Jacobi sweep count of the
ridge definition (include/flowsci_hip.h, "Ridge surfaces") is the smallest that converges on every one of them
(tests/test_ridge_cpu.py).  Not a test module."""
import numpy as np


def _grid(shape):
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64),
                          indexing="ij")
    return x, y, z


PLANE_C = 63.25  # between the nodes 63 and 64: the ridge straddles the boundary of the first 64-node chunk
CYL = {"cx": 13.4, "cy": 11.6, "r": 7.3}
SPHERE = {"c": (58.4, 11.6, 9.7), "r": 6.3, "sigma": 1.5}  # crosses x = 64


def plane(shape=(9, 24, 67), c=PLANE_C):
    """f = -(x - c)^2 + 0.1 y: the ridge is the plane x = c."""
    x, y, _ = _grid(shape)
    return (-(x - c) ** 2 + 0.1 * y).astype(np.float32), c


def cylinder(shape=(9, 24, 30)):
    """f = -(r - R)^2 around an axis along z that passes between the nodes: the ridge is the cylinder r = R."""
    x, y, _ = _grid(shape)
    r = np.sqrt((x - CYL["cx"]) ** 2 + (y - CYL["cy"]) ** 2)
    return (-(r - CYL["r"]) ** 2).astype(np.float32), CYL["r"]


def gauss_cylinder(shape=(9, 24, 30), sigma=1.5):
    x, y, _ = _grid(shape)
    r = np.sqrt((x - CYL["cx"]) ** 2 + (y - CYL["cy"]) ** 2)
    return np.exp(-(r - CYL["r"]) ** 2 / (2 * sigma ** 2)).astype(np.float32), CYL["r"]


def sphere_radius(shape=(20, 24, 67)):
    x, y, z = _grid(shape)
    c = SPHERE["c"]
    return np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)


def gauss_sphere(shape=(20, 24, 67)):
    """A Gaussian shell exp(-(r - R)^2 / (2 sigma^2)): the ridge is the sphere r = R."""
    r = sphere_radius(shape)
    return np.exp(-(r - SPHERE["r"]) ** 2 / (2 * SPHERE["sigma"] ** 2)).astype(np.float32), SPHERE["r"]


def noise(shape=(9, 12, 67), seed=11):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32), None


def noise_nan(shape=(9, 12, 67), seed=12, n=5):
    """White noise with n nodes that are not finite (NaN, and one +inf), some of them on the border."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape).astype(np.float32)
    idx = rng.choice(f.size, n, replace=False)
    f.reshape(-1)[idx] = np.nan
    f.reshape(-1)[idx[0]] = np.inf
    return f, None


def speckled_sphere(shape=(20, 24, 67)):
    """The Gaussian sphere shell plus three isolated bumps away from it: every bump carries a small ridge patch of its
    own (about 60 faces against the shell's 3900), which a component filter drops."""
    f, R = gauss_sphere(shape)
    x, y, z = _grid(shape)
    for cx, cy, cz in ((20.3, 6.4, 5.6), (30.6, 15.3, 12.4), (12.4, 12.7, 9.3)):
        f = f + (0.9 * np.exp(-((x - cx) ** 2 + 0.3 * (y - cy) ** 2 + 0.3 * (z - cz) ** 2) / (2 * 1.2 ** 2))).astype(np.float32)
    return f.astype(np.float32), R


# name -> (builder, strength, fmin)
FIELDS = {
    "plane": (plane, 1.0, -np.inf),
    "cylinder": (cylinder, 1.0, -np.inf),
    "gauss_cylinder": (gauss_cylinder, 0.1, 0.5),
    "gauss_sphere": (gauss_sphere, 0.1, 0.5),
    "noise": (noise, 0.0, -np.inf),
    "noise_nan": (noise_nan, 0.0, -np.inf),
    "speckled_sphere": (speckled_sphere, 0.1, 0.5),
}
