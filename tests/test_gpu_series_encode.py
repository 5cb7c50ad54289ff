"""-m gpu: fs_series_encode / ops.series_encode against the numpy restatement of its rule (tests/series_encode_ref.py):
values bit for bit and all five stats exactly, for the four stored types, the vector and the scalar path, 2-D, several
channels, misaligned operands and a shape whose reduction spans many workgroups; destination and stats sit inside
sentinel-filled buffers whose guard bands must survive."""
import zlib

import numpy as np
import pytest
import torch

from series_encode_ref import crop, encode_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"uint8": (torch.uint8, 0), "uint16": (torch.uint16, 1), "float16": (torch.float16, 2),
          "float32": (torch.float32, 3)}
TOP = {"uint8": 255.0, "uint16": 65535.0, "float16": 65504.0, "float32": 1000.0}
GUARD = 64  # elements in front of and behind every destination (a multiple of 4: the aligned cases stay aligned)

# name -> (N, C, padded (Dp, Hp, Wp), kept (D, H, W), misaligned)
CASES = {
    "vector": (2, 1, (4, 8, 12), (3, 5, 8), False),
    "scalar_w7": (2, 1, (4, 8, 12), (3, 5, 7), False),
    "plane_2d": (2, 1, (1, 8, 12), (1, 5, 8), False),
    "two_channels": (2, 2, (4, 8, 12), (3, 5, 8), False),
    "misaligned": (2, 1, (4, 8, 12), (3, 5, 8), True),
    "many_workgroups": (1, 1, (32, 64, 64), (9, 33, 40), False),
}


def _input(name, N, C, padded, kept, flavour):
    """fp32 [N,C,*padded] whose kept corner mixes in-range values, exact halves, values beyond both clip limits (for
    float16: beyond +-65504), NaN and +-inf; everything outside the corner is NaN or huge -- it must not be read.
    flavour 0: the values are in the type's own units (lo = 0, span = 1); 1: in [0,1] and a bit around it, mapped
    with lo = -2.5 and span = 1.01 * top."""
    rng = np.random.default_rng(zlib.crc32(repr((name, N, C, padded, kept)).encode()))
    top = TOP[name]
    low = -top if name in ("float16", "float32") else 0.0
    shape = (N, C) + kept
    n = int(np.prod(shape))
    v = rng.uniform(low - 0.1 * top, 1.1 * top, n)
    k = n // 4
    v[:k] = np.floor(rng.uniform(0, min(top, 4000.0), k)) + 0.5        # exact halves: ties go to even
    v[k:k + 6] = [0.5, 1.5, 2.5, top - 0.5, top + 0.5, -0.5]
    v[k + 6:k + 10] = [top * 1.07, -top * 1.07, top, low]
    v[k + 13:k + 16] = [1e-6, -3e-5, 6.1e-5]                           # float16: subnormal results
    v = v.astype(np.float32)
    lo, span = 0.0, 1.0
    if flavour == 1:
        lo, span = -2.5, 1.01 * top
        v = ((v - np.float32(lo)) / np.float32(span)).astype(np.float32)
    v[k + 10:k + 13] = [np.nan, np.inf, -np.inf]
    v = v[rng.permutation(n)].reshape(shape)
    x = np.full((N, C) + padded, np.nan, np.float32)
    x[..., padded[2] - 1] = 3e38
    x[(Ellipsis,) + tuple(slice(0, s) for s in kept)] = v
    return x, lo, span


_refs = {}


def _case(name, case, flavour):
    key = (name, case, flavour)
    if key not in _refs:
        N, C, padded, kept, _ = CASES[case]
        x, lo, span = _input(name, N, C, padded, kept, flavour)
        want, stats = encode_ref(crop(x, kept).reshape(N, -1), name, lo, span)
        _refs[key] = (x, lo, span, want.reshape((N, C) + kept), stats)
    return _refs[key]


def _launch(x, name, kept, lo, span, misaligned, with_stats=True):
    """fs_series_encode itself, on buffers this test owns: -> (values, stats or None) as numpy; checks the guards."""
    from opticalflowscivis_amd import _lib
    tdt, code = DTYPES[name]
    N, C = x.shape[:2]
    padded = tuple(x.shape[2:])
    n_out = N * C * int(np.prod(kept))
    off = 1 if misaligned else 0
    xbuf = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    xs = xbuf[off:off + x.size].view(x.shape)
    xs.copy_(torch.from_numpy(x))
    esz = torch.empty(0, dtype=tdt).element_size()
    raw = torch.full(((2 * GUARD + n_out + 1) * esz,), 0xA5, dtype=torch.uint8, device=DEV)
    first = (GUARD + off) * esz
    assert xs.data_ptr() % 16 == (4 if misaligned else 0)
    assert (raw.data_ptr() + first) % (4 * esz) == (esz if misaligned else 0)
    L = _lib.lib()
    nb = L.fs_series_encode_ws_bytes(N, C, *kept)
    assert nb > 0
    st = torch.full((GUARD + 5 * N + GUARD,), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(nb // 8, dtype=torch.float64, device=DEV)
    rc = L.fs_series_encode(xs.data_ptr(), N, C, *padded, raw.data_ptr() + first, code, *kept, lo, span,
                            ws.data_ptr() if with_stats else None,
                            st.data_ptr() + 8 * GUARD if with_stats else None,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = raw.cpu().numpy()
    assert (got[:first] == 0xA5).all() and (got[first + n_out * esz:] == 0xA5).all(), "wrote outside the destination"
    values = got[first:first + n_out * esz].view(np.dtype(name)).reshape((N, C) + tuple(kept))
    stats = st.cpu().numpy()
    assert (stats[:GUARD] == -7.0).all() and (stats[GUARD + 5 * N:] == -7.0).all(), "wrote outside the stats"
    if not with_stats:
        assert (stats == -7.0).all()
        return values, None
    return values, stats[GUARD:GUARD + 5 * N].reshape(N, 5)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", list(DTYPES))
def test_kernel_matches_the_rule(name, case):
    from opticalflowscivis_amd import _lib
    N, C, padded, kept, mis = CASES[case]
    if case == "many_workgroups":  # 11880 elements: 12 workgroups contribute partials
        assert _lib.lib().fs_series_encode_ws_bytes(N, C, *kept) == 12 * 5 * 8
    for flavour in (0, 1):
        x, lo, span, want, wstats = _case(name, case, flavour)
        got, stats = _launch(x, name, kept, lo, span, mis)
        assert _same_bits(got, want), (flavour, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8])
        assert np.array_equal(stats, wstats), (flavour, stats, wstats)
        if name != "float32":
            assert wstats[:, 2:].sum(0).min() >= 1  # the input does clip on both sides and holds non-finite values
        plain, none = _launch(x, name, kept, lo, span, mis, with_stats=False)
        assert none is None and _same_bits(plain, want)


@pytest.mark.parametrize("name", list(DTYPES))
def test_misaligned_operands_give_the_aligned_stats(name):
    N, C, padded, kept, _ = CASES["vector"]
    x, lo, span, want, _ = _case(name, "vector", 1)
    a, sa = _launch(x, name, kept, lo, span, False)
    b, sb = _launch(x, name, kept, lo, span, True)
    assert _same_bits(a, b) and sa.tobytes() == sb.tobytes()


@pytest.mark.parametrize("name", list(DTYPES))
def test_op(name):
    from opticalflowscivis_amd import ops
    tdt, _ = DTYPES[name]
    N, C, padded, kept, _ = CASES["two_channels"]
    x, lo, span, want, wstats = _case(name, "two_channels", 1)
    xd = torch.from_numpy(x).to(DEV)
    out, stats = ops.series_encode(xd, tdt, kept, lo=lo, span=span)
    assert out.dtype == tdt and tuple(out.shape) == (N, C) + kept and stats.dtype == torch.float64
    assert _same_bits(out.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), wstats)
    # into a view of a larger staging buffer, numpy dtype, no stats; the neighbours stay untouched
    nbytes = (N + 2) * C * int(np.prod(kept)) * np.dtype(name).itemsize
    staging = torch.zeros(nbytes, dtype=torch.uint8, device=DEV).view(tdt).view((N + 2, C) + kept)
    out2, none = ops.series_encode(xd, np.dtype(name), kept, lo=lo, span=span, out=staging[1:N + 1], stats=False)
    assert none is None and out2.data_ptr() == staging[1].data_ptr()
    got = staging.cpu().numpy()
    assert _same_bits(got[1:N + 1], want) and not got[0].any() and not got[N + 1].any()
    # 2-D planes: [N,C,Hp,Wp] -> [N,C,H,W]
    x2, lo2, span2, want2, ws2 = _case(name, "plane_2d", 0)
    o2, s2 = ops.series_encode(torch.from_numpy(x2[:, :, 0]).to(DEV), tdt, (5, 8), lo=lo2, span=span2)
    assert _same_bits(o2.cpu().numpy(), want2[:, :, 0]) and np.array_equal(s2.cpu().numpy(), ws2)


def test_op_refusals():
    from opticalflowscivis_amd import ops
    x = torch.zeros(1, 1, 4, 8, 12)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.series_encode(x, torch.uint8, (3, 5, 8))
    xd = x.to(DEV)
    with pytest.raises(ValueError):
        ops.series_encode(xd, torch.int32, (3, 5, 8))
    with pytest.raises(ValueError):
        ops.series_encode(xd, torch.uint8, (5, 5, 8))           # kept > padded
    with pytest.raises(ValueError):
        ops.series_encode(xd, torch.uint8, (5, 8))              # rank
    with pytest.raises(ValueError):
        ops.series_encode(xd, torch.uint8, (3, 5, 8), out=torch.empty(1, 1, 3, 5, 8, dtype=torch.uint16, device=DEV))
