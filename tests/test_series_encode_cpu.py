"""CPU: the way back from fp32 to a stored type -- fs_series_encode's argument validation (made before any launch), the
numpy restatement of its rule (tests/series_encode_ref.py) and its round-trip properties, the chunk arithmetic of
reconstruct.reconstruct_series, SeriesWriter and the reconstruct parser."""
import os

import numpy as np
import pytest

from series_encode_ref import decode_ref, encode_ref, keyframe_ref, lo_inv_span

U8, U16, F16, F32 = 0, 1, 2, 3  # FS_SERIES_*


def test_entry_point_refusals_without_gpu():
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    enc = lambda src=64, dst=128, N=1, C=1, P=(4, 8, 12), dtype=U8, S=(3, 5, 8), ws=256, stats=512: L.fs_series_encode(
        src, N, C, *P, dst, dtype, *S, 0.0, 1.0, ws, stats, None)
    assert L.fs_series_encode(None, 1, 1, 4, 8, 12, 128, U8, 3, 5, 8, 0.0, 1.0, None, None, None) == 1
    assert enc(src=None) == 1 and enc(dst=None) == 1                       # NULLPTR
    assert enc(ws=None) == 1 and enc(stats=None) == 1                      # exactly one of ws / stats
    assert enc(S=(5, 5, 8)) == 2                                           # D > Dp
    assert enc(S=(3, 9, 8)) == 2 and enc(S=(3, 5, 13)) == 2 and enc(S=(0, 5, 8)) == 2 and enc(N=0) == 2
    assert enc(P=(2048, 2048, 2048), S=(1, 1, 1)) == 2                      # more padded elements than the file indexes
    assert enc(dtype=9) == 3 and enc(dtype=-1) == 3                        # unknown dtype
    assert enc(dtype=U16, dst=129) == 3 and enc(dtype=F32, dst=130) == 3   # dst not aligned to its element
    assert enc(dtype=U8, dst=129, S=(5, 5, 8)) == 2                        # (shape is judged before alignment)
    assert L.fs_series_encode_ws_bytes(2, 1, 3, 5, 8) > 0
    assert L.fs_series_encode_ws_bytes(2, 1, 3, 5, 8) % 40 == 0           # 5 doubles per workgroup
    assert L.fs_series_encode_ws_bytes(0, 1, 3, 5, 8) == -2
    assert L.fs_series_encode_ws_bytes(1, 1, 3, 0, 8) == -2


def test_ops_series_encode_refuses_cpu_tensors():
    import torch
    from opticalflowscivis_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.series_encode(torch.zeros(1, 1, 4, 8, 12), torch.uint8, (3, 5, 8))
    assert ops.series_encode_cost((2, 1, 3, 5, 8), 2) == (240 * 6, 480)


def test_rule_on_halves_limits_and_non_finite():
    x = np.array([[0.5, 1.5, 2.5, 254.5, 255.5, -0.5, np.nan, np.inf]], np.float32)
    got, stats = encode_ref(x, np.uint8)
    assert got.dtype == np.uint8 and got.tolist() == [[0, 2, 2, 254, 255, 0, 0, 0]]
    assert stats.tolist() == [[-0.5, 255.5, 1.0, 1.0, 2.0]]
    # -inf is non-finite too, not low; float16 saturates and counts; float32 keeps y and counts nothing
    x = np.array([[-np.inf, 70000.0, -70000.0, 65504.0, 65519.0, 1e-8, 0.1]], np.float32)
    got, stats = encode_ref(x, np.float16)
    assert got.view(np.uint16).tolist() == [[0, 0x7bff, 0xfbff, 0x7bff, 0x7bff, 0, np.float16(0.1).view(np.uint16)]]
    assert stats.tolist() == [[-70000.0, 70000.0, 1.0, 2.0, 1.0]]
    got, stats = encode_ref(x, np.float32)
    assert got[0, 1:].tolist() == x[0, 1:].tolist() and got[0, 0] == 0 and stats[0, 2:].tolist() == [0.0, 0.0, 1.0]
    # span and lo are two rounded operations
    x = np.array([[0.1, 0.7]], np.float32)
    got, _ = encode_ref(x, np.float32, lo=3.0, span=197.0)
    want = (x * np.float32(197.0)).astype(np.float32) + np.float32(3.0)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    # nothing finite: +inf / -inf
    assert encode_ref(np.full((1, 3), np.nan, np.float32), np.uint16)[1].tolist() == [[np.inf, -np.inf, 0.0, 0.0, 3.0]]


def test_product_numpy_rule_is_the_restatement():
    from opticalflowscivis_amd.data.series import encode_numpy
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 4096)) * 300).astype(np.float32)
    x[0, :8] = [0.5, 1.5, 2.5, np.nan, np.inf, -np.inf, 70000.0, -70000.0]
    for dt in (np.uint8, np.uint16, np.float16, np.float32):
        for lo, span in ((0.0, 1.0), (3.0, 197.0)):
            want = encode_ref(x, dt, lo, span)[0]
            got = encode_numpy(x, dt, lo, span)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (dt, lo, span)


def _product_round_trip(stored, first, stop, lo, inv, span):
    """The product's own host path: data.series.gather_numpy decodes whole frames, data.series.encode_numpy encodes."""
    from opticalflowscivis_amd import ops
    from opticalflowscivis_amd.data.series import encode_numpy, gather_numpy
    n = stop - first
    frame = (1, n)
    arr = np.concatenate([stored[first:stop]] * 3).reshape((3,) + frame)  # one ready-made triplet of three equal frames
    rec = np.zeros(1, ops.TRIPLET_JOB)
    rec["off"] = np.arange(3) * n
    rec["lo"], rec["inv"] = lo, inv
    x = gather_numpy(arr, rec[0], frame, frame)[0].reshape(-1)
    return encode_numpy(x, stored.dtype, lo, span)


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
def test_decode_then_encode_returns_every_integer_code(dtype):
    from opticalflowscivis_amd.reconstruct import normalisation
    mx = int(np.iinfo(dtype).max)
    for a, b in ((0, mx), (3, 200), (17, mx - 5), (0, 1), (100, 101), (1, mx)):
        codes = np.arange(a, b + 1).astype(dtype)
        lo, inv, span = lo_inv_span(a, b)
        back, stats = encode_ref(decode_ref(codes, lo, inv)[None], dtype, lo, span)
        assert np.array_equal(back[0], codes), (dtype, a, b)
        assert stats[0, 2:].tolist() == [0.0, 0.0, 0.0]
        # the same property of the product's rule, with the (lo, inv, span) the driver derives from the range
        plo, pinv, pspan = normalisation("global", (a, b))
        assert np.array_equal(_product_round_trip(codes, 0, len(codes), plo, pinv, pspan), codes), (dtype, a, b)


def test_decode_then_encode_float16_is_exact_from_zero():
    from opticalflowscivis_amd.reconstruct import normalisation
    codes = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16)  # every finite non-negative half
    for a, b in ((0.0, 1.0), (0.0, 65504.0)):
        v = codes[(codes >= a) & (codes <= b)]
        lo, inv, span = lo_inv_span(a, b)
        back, _ = encode_ref(decode_ref(v, lo, inv)[None], np.float16, lo, span)
        assert np.array_equal(back[0].view(np.uint16), v.view(np.uint16)), (a, b)
        plo, pinv, pspan = normalisation("global", (a, b))
        got = _product_round_trip(v, 0, len(v), plo, pinv, pspan)
        assert np.array_equal(got.view(np.uint16), v.view(np.uint16)), (a, b)


def test_keyframe_conversion():
    from opticalflowscivis_amd.data.series import encode_numpy
    v = np.array([0, 7, 300, 65535], np.uint16)
    assert keyframe_ref(v, np.uint16) is v
    assert keyframe_ref(v, np.uint8).tolist() == [0, 7, 255, 255]
    assert keyframe_ref(v, np.float32).tolist() == [0.0, 7.0, 300.0, 65535.0]
    f = np.array([np.nan, 2.5, 3.5, -np.inf, 1e9], np.float32)
    assert keyframe_ref(f, np.uint8).tolist() == [0, 2, 4, 0, 255]
    for src, dt in ((v, np.uint8), (v, np.float32), (v, np.float16), (f, np.uint8), (f, np.uint16), (f, np.float16)):
        got = encode_numpy(src.astype(np.float32), dt)  # what the writer does for a keyframe of another type
        assert got.dtype == np.dtype(dt) and got.tobytes() == keyframe_ref(src, dt).tobytes()


def test_rule_on_halves_through_the_product_rule():
    from opticalflowscivis_amd.data.series import encode_numpy
    x = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.5, np.nan, np.inf], np.float32)
    assert encode_numpy(x, np.uint8).tolist() == [0, 2, 2, 254, 255, 0, 0, 0]


def test_report_holds_no_token_json_lacks():
    import json
    from opticalflowscivis_amd.reconstruct import json_safe
    doc = {"totals": {"min": float("inf"), "max": float("-inf"), "n_low": 3}, "stats": [{"min": float("nan"), "max": 2.5}],
           "flow_parents": [(0, 2)], "range": None}
    text = json.dumps(json_safe(doc), allow_nan=False)
    assert json.loads(text) == {"totals": {"min": None, "max": None, "n_low": 3}, "stats": [{"min": None, "max": 2.5}],
                                "flow_parents": [[0, 2]], "range": None}


# ------------------------------------------------------------------------------------------- driver arithmetic
@pytest.mark.parametrize("chunk", (1, 2, 4))
def test_chunks_produce_every_in_between_frame_once(chunk):
    from opticalflowscivis_amd.reconstruct import plan_chunks
    K, exp = 5, 2
    factor = 2 ** exp
    chunks = plan_chunks(K, exp, chunk)
    assert [c["keys"] for c in chunks] == [(k, min(k + chunk, K - 1)) for k in range(0, K - 1, chunk)]
    frames = [t for c in chunks for t in c["frames"]]
    assert frames == [t for t in range((K - 1) * factor + 1) if t % factor]  # each once, in output order
    # the parents are the bisection's: replay interpolate_sequence's level loop on every chunk's sub-series
    want = {}
    for c in chunks:
        k0, k1 = c["keys"]
        T, step = (k1 - k0) * factor + 1, factor
        while step > 1:
            for left in range(0, T - 1, step):
                want[k0 * factor + left + step // 2] = (k0 * factor + left, k0 * factor + left + step)
            step //= 2
    got = {t: p for c in chunks for t, p in zip(c["frames"], c["parents"])}
    assert got == want
    assert got[1] == (0, 2) and got[2] == (0, 4) and got[3] == (2, 4) and got[13] == (12, 14)


def test_chunk_plan_refusals_and_uneven_tail():
    from opticalflowscivis_amd.reconstruct import plan_chunks
    assert [c["keys"] for c in plan_chunks(6, 1, 2)] == [(0, 2), (2, 4), (4, 5)]
    assert plan_chunks(6, 1, 2)[-1]["frames"] == [9] and plan_chunks(6, 1, 2)[-1]["parents"] == [(8, 10)]
    for bad in ((1, 1, 1), (5, 0, 1), (5, 1, 0)):
        with pytest.raises(ValueError):
            plan_chunks(*bad)


def test_normalisation_matches_the_training_plan():
    from opticalflowscivis_amd.data.series import TripletPlan
    from opticalflowscivis_amd.reconstruct import normalisation
    for lo, hi in ((3.0, 200.0), (0.0, 65535.0), (-1.25, 7.5), (5.0, 5.0), (0.1, 0.7)):
        plan = TripletPlan((9, 32, 32, 32), 3, normalize="global")
        plan.set_stats(np.zeros((9, 3)), norm_range=(lo, hi))
        rec = plan.records()[0]
        got = normalisation("global", (lo, hi))
        assert got[0] == rec["lo"] and got[1] == rec["inv"]
        want = lo_inv_span(lo, hi)
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want]
    assert [float(v) for v in normalisation("none", None)] == [0.0, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------- plumbing
def test_series_writer(tmp_path):
    from opticalflowscivis_amd.data.series import SeriesWriter, load_series
    src = str(tmp_path / "in.npy")
    np.save(src, np.zeros((2, 3, 4), np.uint16))
    out = str(tmp_path / "sub" / "out.npy")
    with SeriesWriter(out, (3, 1, 3, 4), np.uint16, source=src) as w:
        assert w.shape == (3, 1, 3, 4) and w.dtype == np.uint16
        for t in (2, 0, 1):
            w.write(t, np.full((3, 4), 1000 * t + 5, np.uint16))
        with pytest.raises(IndexError):
            w.write(3, np.zeros((3, 4), np.uint16))
        with pytest.raises(ValueError):
            w.write(0, np.zeros((3, 4), np.float32))
    got = np.load(out)
    assert got.dtype == np.uint16 and got.shape == (3, 1, 3, 4) and got[:, 0, 0, 0].tolist() == [5, 1005, 2005]
    assert load_series(out, nd=2).shape == (3, 1, 3, 4)
    with pytest.raises(ValueError, match="input itself"):
        SeriesWriter(src, (3, 3, 4), np.uint16, overwrite=True, source=src)
    link = str(tmp_path / "alias.npy")
    os.symlink(src, link)
    with pytest.raises(ValueError, match="input itself"):
        SeriesWriter(link, (3, 3, 4), np.uint16, overwrite=True, source=src)
    with pytest.raises(FileExistsError):
        SeriesWriter(out, (3, 1, 3, 4), np.uint16)
    SeriesWriter(out, (2, 3, 4), np.float16, overwrite=True).close()
    assert np.load(out).shape == (2, 3, 4)
    with pytest.raises(ValueError):
        SeriesWriter(str(tmp_path / "out.npz"), (2, 3, 4), np.uint8)
    with pytest.raises(ValueError):
        SeriesWriter(str(tmp_path / "o2.npy"), (2, 3, 4), np.int32)


def test_parser_and_driver_refusals():
    from opticalflowscivis_amd.reconstruct import build_parser, reconstruct_series
    ap = build_parser(3)
    args = ap.parse_args(["--series", "a.npy", "--out", "b.npy"])
    assert (args.exp, args.dtype, args.normalize, args.flow_dtype, args.batch, args.chunk) == (
        1, "stored", "global", "float32", 1, 1)
    with pytest.raises(SystemExit):
        ap.parse_args(["--series", "a.npy", "--out", "b.npy", "--normalize", "frame"])
    with pytest.raises(ValueError, match="per-frame"):
        reconstruct_series(None, np.zeros((3, 4, 4, 4), np.uint8), 1, None, normalize="frame", nd=3)
    with pytest.raises(ValueError, match="triplets"):
        reconstruct_series(None, np.zeros((4, 3, 4, 4, 4), np.uint8), 1, None, nd=3)
    with pytest.raises(ValueError):
        reconstruct_series(None, np.zeros((3, 4, 4, 4), np.int32), 1, None, nd=3)
    helptext = " ".join(build_parser(2).format_help().split())
    assert "powers of two" in helptext and "UPFlow" in helptext and "frame" in helptext
