"""numpy restatement of fs_series_encode (include/flowsci_hip.h): values, the five stats, and the host conversion of
keyframes.  Written from the rule, not from the library's code:

    y = fl32(x * span);  y = fl32(y + lo)
    non-finite y          -> stored 0, counted as non-finite (neither low nor high)
    uint8 / uint16        -> low when y < 0, high when y > 255 / 65535; clamp, round to nearest even, convert
    float16               -> low when y < -65504, high when y > 65504; saturate, fp32 -> half round to nearest even
    float32               -> y
    stats[n] = {min y, max y over the finite y before clamping (+inf / -inf if none), n_low, n_high, n_nonfinite}"""
import numpy as np

RANGE = {np.dtype(np.uint8): (0.0, 255.0), np.dtype(np.uint16): (0.0, 65535.0),
         np.dtype(np.float16): (-65504.0, 65504.0), np.dtype(np.float32): (-np.inf, np.inf)}


def encode_ref(x, dtype, lo=0.0, span=1.0):
    """(stored [N,...] of `dtype`, stats [N,5] float64) of fp32 `x` [N,...] (already cropped)."""
    dtype = np.dtype(dtype)
    a, b = RANGE[dtype]
    x = np.asarray(x)
    assert x.dtype == np.float32
    with np.errstate(all="ignore"):
        y = np.multiply(x, np.float32(span), dtype=np.float32)
        y = np.add(y, np.float32(lo), dtype=np.float32)
    fin = np.isfinite(y)
    stats = np.empty((x.shape[0], 5), np.float64)
    for n in range(x.shape[0]):
        v = y[n][fin[n]]
        stats[n] = (v.min() if v.size else np.inf, v.max() if v.size else -np.inf,
                    np.count_nonzero(v < np.float32(a)), np.count_nonzero(v > np.float32(b)),
                    y[n].size - v.size)
    z = np.where(fin, y, np.float32(0))
    if dtype != np.float32:
        z = np.minimum(np.maximum(z, np.float32(a)), np.float32(b))
    if dtype.kind == "u":
        z = np.rint(z)  # round half to even
    return z.astype(dtype), stats


def crop(x, spatial):
    """The corner [..., :D, :H, :W] of padded planes."""
    return x[(Ellipsis,) + tuple(slice(0, s) for s in spatial)]


def decode_ref(v, lo, inv):
    """The gather's rule (data.series.gather_numpy): (fl32(v) - lo) * inv, non-finite v read as 0."""
    f = np.asarray(v).astype(np.float32)
    f = np.where(np.isfinite(f), f, np.float32(0))
    return np.multiply(np.subtract(f, np.float32(lo), dtype=np.float32), np.float32(inv), dtype=np.float32)


def lo_inv_span(lo, hi):
    """fp32 (lo, inv, span) of a range, as TripletPlan.records forms lo and inv; span = hi - lo in fp32, 1 if not > 0."""
    lo, hi = np.float32(lo), np.float32(hi)
    d = np.float32(hi - lo)
    if d > 0:
        return lo, np.float32(np.float32(1) / d), d
    return lo, np.float32(1), np.float32(1)


def keyframe_ref(v, dtype):
    """A stored keyframe in the output type: itself when the types agree, else the encode rule with lo = 0, span = 1."""
    v = np.asarray(v)
    if v.dtype == np.dtype(dtype):
        return v
    return encode_ref(v.astype(np.float32)[None], dtype)[0][0]
