"""Fields and seeds shared by the streamline and skeleton tests (numpy only; imports nothing from the product)."""
import numpy as np

KINDS = ("noise", "smooth", "ball", "nonfinite")


def axes(sp):
    """The node coordinates (x, y(, z)) of a grid of spatial shape sp, each an fp64 array of that shape."""
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sp], indexing="ij")[::-1]


def double_well(nd):
    """(field [nd, *sp] fp32, centre (x, y(, z)), s): v = (u (1 - u^2), -(y - cy)(, -(z - cz))), u = (x - cx) / s: a saddle
    at the centre whose unstable manifold runs along x into the sinks at cx -+ s and whose stable manifold is the line
    (plane) x = cx.  The centres keep every zero off the nodes (a zero ON a node is a degenerate simplex)."""
    n, cx, s = (33, 16.3, 7.9) if nd == 2 else (21, 10.3, 4.6)
    c = [cx + 0.11 * a for a in range(nd)]
    ax = axes((n,) * nd)
    u = (ax[0] - c[0]) / s
    v = [u * (1.0 - u * u)] + [-(ax[a] - c[a]) for a in range(1, nd)]
    return np.stack(v).astype(np.float32), c, s


def linear_field(sp, A, centre):
    """v = A (x - centre) on a grid of spatial shape sp, fp32."""
    ax = axes(sp)
    d = np.stack([ax[a] - centre[a] for a in range(len(sp))])
    return np.einsum("rc,c...->r...", np.asarray(A, np.float64), d).astype(np.float32)


def stack_of(sp, kind, K, seed):
    """[K, C, *sp] fp32: white noise; a band-limited field (a few low sines); noise that is exactly zero outside a ball;
    noise with a NaN, a +inf and a -inf node in every field."""
    C = len(sp)
    rng = np.random.default_rng(seed)
    S = np.array(sp[::-1], np.float64)
    if kind == "smooth":
        ax = axes(sp)
        out = np.stack([np.stack([0.7 * np.sin(0.9 * ax[(c + 1) % C] + 0.5 * k + c) + 0.4 * np.cos(0.6 * ax[(c + 2) % C] - k)
                                  for c in range(C)]) for k in range(K)]).astype(np.float32)
    else:
        out = (0.6 * rng.standard_normal((K, C) + sp)).astype(np.float32)
    if kind == "ball":
        ax = axes(sp)
        r2 = sum(((ax[c] - 0.5 * (S[c] - 1)) / (0.35 * S[c])) ** 2 for c in range(C))
        out = out * (r2 <= 1.0).astype(np.float32)
    if kind == "nonfinite":
        n = out[0, 0].size
        flat = out.reshape(K, C, n)
        for k in range(K):
            for j, v in enumerate((np.nan, np.inf, -np.inf)):
                flat[k, (k + j) % C, (7 * k + 3 * j + 2) % n] = v
    return out


def lines_of(sp, K, S, seed):
    """Seeds and per-line arguments for S lines on K fields of spatial shape sp: seeds fp64 [S, C] spread over the grid
    and half an element beyond it, every 11th not finite; step mixed over 0..K-1 with every 13th out of range; sign of
    both kinds; home -1, the seed's own cell or another cell, by thirds."""
    C = len(sp)
    rng = np.random.default_rng(seed)
    ext = np.array(sp[::-1], np.float64)
    seeds = rng.uniform(-0.4, ext - 0.6, (S, C))
    bad = np.arange(S) % 11 == 7
    seeds[bad, np.arange(S)[bad] % C] = np.array([np.nan, np.inf, -np.inf])[np.arange(S)[bad] % 3]
    step = rng.integers(0, K, S).astype(np.int32)
    wrong = np.arange(S) % 13 == 5
    step[wrong] = np.where(np.arange(S)[wrong] % 2 == 0, -1, K)
    sign = rng.choice(np.array([1, -1, 0, -128, 127], np.int8), S)
    with np.errstate(invalid="ignore"):
        cell = [np.clip(np.floor(np.nan_to_num(seeds[:, c], nan=0.0, posinf=0.0, neginf=0.0)), 0, ext[c] - 2).astype(np.int64)
                for c in range(C)]
    own = ((cell[2] * sp[1] + cell[1]) if C == 3 else cell[1]) * sp[-1] + cell[0]
    plane = int(np.prod(sp))
    third = np.arange(S) % 3
    home = np.where(third == 0, -1, np.where(third == 1, own, rng.integers(0, plane, S))).astype(np.int32)
    return seeds, step, sign, home
