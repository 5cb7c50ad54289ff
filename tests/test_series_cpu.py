"""CPU: training triplets from stored arrays (data/series.py) against the reference's load_data -- restated in
tests/series_ref.py and pinned by a fixture the reference's own code produced -- plus plan determinism, file formats,
refusals and the C entry points' argument validation."""
import os
import pickle

import numpy as np
import pytest
import torch

from opticalflowscivis_amd import ops
from opticalflowscivis_amd.data.series import FileTriplets, TripletPlan, gather_numpy, load_series, series_layout

from series_ref import ref_triplets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "series_rectangle3d.npz")
DTYPES = (np.uint8, np.uint16, np.float16, np.float32)


def _random(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.integer):
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    return (rng.standard_normal(shape) * 3).astype(dtype)


def _all(ds):
    return np.stack([ds[i].numpy() for i in range(len(ds))])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("five_d", (False, True))
def test_series_matches_reference_restatement(dtype, five_d):
    T, n_train = 30, 21  # a multiple of 3 training frames, as the reference's 750
    data = _random((T, 3, 5, 6), dtype, 1)
    stored = data[:, None] if five_d else data
    train = FileTriplets(stored, TripletPlan(stored.shape, 3, stop=n_train, augment="ref", multiple=1))
    val = FileTriplets(stored, TripletPlan(stored.shape, 3, first=n_train, train=False, multiple=1))
    rt, rv = ref_triplets(data, n_train)
    got_t, got_v = _all(train), _all(val)
    assert got_t.dtype == np.float32 and got_t.shape == rt.shape == (4 * n_train // 3, 3, 3, 5, 6)
    assert np.array_equal(got_t.view(np.uint32), rt.view(np.uint32))
    assert np.array_equal(got_v.view(np.uint32), rv.view(np.uint32)) and len(val) == 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_ready_made_triplets_match_reference_restatement(dtype):
    data = _random((10, 3, 4, 5, 3), dtype, 2)
    train = FileTriplets(data, TripletPlan(data.shape, 3, stop=7, augment="ref", multiple=1))
    val = FileTriplets(data, TripletPlan(data.shape, 3, first=7, train=False, multiple=1))
    rt, rv = ref_triplets(data, 7, cut=False)
    assert len(train) == 28 and np.array_equal(_all(train).view(np.uint32), rt.view(np.uint32))
    assert np.array_equal(_all(val).view(np.uint32), rv.view(np.uint32))


def test_restatement_and_plan_match_the_references_own_output():
    """series_rectangle3d.npz was written by the reference's load_data (tests/golden/make_series_golden.py)."""
    g = np.load(GOLDEN)
    data = g["data"]
    assert data.shape == (900, 4, 4, 4) and data.dtype == np.uint8
    rt, rv = ref_triplets(data, 750, 900)
    assert len(rt) == int(g["n_train"]) == 1000 and len(rv) == int(g["n_val"]) == 50
    assert np.array_equal(rt[g["train_idx"]], g["train"]) and np.array_equal(rv[g["val_idx"]], g["val"])
    train = FileTriplets(data, TripletPlan(data.shape, 3, stop=750, augment="ref", multiple=1))
    val = FileTriplets(data, TripletPlan(data.shape, 3, first=750, train=False, multiple=1))
    assert len(train) == 1000 and len(val) == 50
    for k, i in enumerate(g["train_idx"]):
        assert np.array_equal(train[int(i)].numpy(), g["train"][k]), i
    for k, i in enumerate(g["val_idx"]):
        assert np.array_equal(val[int(i)].numpy(), g["val"][k]), i


def test_plan_is_a_function_of_seed_and_epoch():
    shape = (40, 64, 96, 64)
    mk = lambda seed: TripletPlan(shape, 3, stop=30, augment="full", crop=(32, 32, 32), seed=seed)
    a, b = mk(5).records(3), mk(5).records(3)
    assert a.tobytes() == b.tobytes()
    c = mk(5).records(4)
    assert any((a[k] != c[k]).any() for k in ("z0", "y0", "x0"))
    assert mk(6).records(3).tobytes() != a.tobytes()
    assert (a["z0"] >= 0).all() and (a["z0"] <= 32).all() and (a["y0"] <= 64).all() and a["y0"].max() > 32
    assert set(np.unique(a["flip"])) <= set(range(8)) and (a["flip"] & 1).any()
    ops.check_triplet_jobs(a, int(np.prod(shape)), shape[1:], (32, 32, 32))
    # validation: no augmentation, centre crop, the same in every epoch
    v = TripletPlan(shape, 3, first=30, train=False, augment="full", crop=(32, 32, 32))
    r = v.records(0)
    assert len(v) == 3 and (r["flip"] == 0).all() and (r["z0"] == 16).all() and (r["y0"] == 32).all()
    assert r.tobytes() == v.records(7).tobytes()
    # gap and stride
    p = TripletPlan(shape, 3, gap=2, stride=1, augment="none")
    assert len(p) == 36 and (p.base[1] == (1, 5, 3)).all()


def test_two_d_series_and_normalisation():
    data = _random((9, 32, 64), np.uint16, 3)
    assert series_layout(data.shape, 2) == ("series", 9, (32, 64))
    ds = FileTriplets(data, TripletPlan(data.shape, 2, augment="none", normalize="global"))
    lo, hi = np.float32(data.min()), np.float32(data.max())
    want = (np.float32(data[[0, 2, 1]]) - lo) * (np.float32(1) / (hi - lo))
    assert np.array_equal(ds[0].numpy(), want) and ds[0].shape == (3, 32, 64)
    fr = FileTriplets(data, TripletPlan(data.shape, 2, augment="none", normalize="frame"))
    sub = data[3:6]
    lo, hi = np.float32(sub.min()), np.float32(sub.max())
    assert np.array_equal(fr[1].numpy(), (np.float32(data[[3, 5, 4]]) - lo) * (np.float32(1) / (hi - lo)))
    # non-finite stored values read as 0 and do not enter the range
    f = _random((3, 32, 32), np.float32, 4)
    f[0, 0, 0], f[1, 1, 1], f[2, 2, 2] = np.nan, np.inf, -np.inf
    g = FileTriplets(f, TripletPlan(f.shape, 2, augment="none", normalize="global"))[0].numpy()
    fin = f[np.isfinite(f)]
    lo, inv = fin.min(), np.float32(1) / (fin.max() - fin.min())
    assert g[0, 0, 0] == g[2, 1, 1] == g[1, 2, 2] == (np.float32(0) - lo) * inv and np.isfinite(g).all()


def test_file_formats_round_trip(tmp_path):
    data = _random((7, 2, 3, 4), np.float16, 5)
    np.save(tmp_path / "a.npy", data)
    np.savez(tmp_path / "a.npz", frames=data, other=np.zeros(3))
    with open(tmp_path / "a.pkl", "wb") as f:
        pickle.dump(data, f)
    a = load_series(str(tmp_path / "a.npy"))
    assert isinstance(a, np.memmap) and a.dtype == np.float16 and np.array_equal(a, data)
    assert np.array_equal(load_series(str(tmp_path / "a.npz"), key="frames"), data)
    assert np.array_equal(load_series(str(tmp_path / "a.pkl"), allow_pickle=True), data)
    np.save(tmp_path / "d.npy", data.astype(np.float64))
    d = load_series(str(tmp_path / "d.npy"))
    assert d.dtype == np.float32 and np.array_equal(d, data.astype(np.float32))


def test_refusals(tmp_path):
    data = _random((7, 2, 3, 4), np.float32, 6)
    with open(tmp_path / "a.pkl", "wb") as f:
        pickle.dump(data, f)
    with pytest.raises(ValueError, match="allow_pickle"):
        load_series(str(tmp_path / "a.pkl"))
    with open(tmp_path / "b.pkl", "wb") as f:
        pickle.dump({"x": 1}, f)
    with pytest.raises(ValueError, match="one numpy array"):
        load_series(str(tmp_path / "b.pkl"), allow_pickle=True)
    np.savez(tmp_path / "a.npz", x=data, y=data)
    with pytest.raises(ValueError, match="series_key"):
        load_series(str(tmp_path / "a.npz"))
    np.save(tmp_path / "six.npy", np.zeros((2, 1, 1, 2, 2, 2), np.float32))
    with pytest.raises(ValueError, match="shape"):
        load_series(str(tmp_path / "six.npy"))
    np.save(tmp_path / "i32.npy", np.zeros((4, 2, 2, 2), np.int32))
    with pytest.raises(ValueError, match="int32"):
        load_series(str(tmp_path / "i32.npy"))
    with pytest.raises(ValueError, match="spans 5 frames"):
        TripletPlan((4, 32, 32, 32), 3, gap=2)
    with pytest.raises(ValueError, match="larger than"):
        TripletPlan((9, 32, 32, 32), 3, crop=(64, 32, 32))
    with pytest.raises(ValueError, match="multiples of 32"):
        TripletPlan((9, 64, 64, 64), 3, crop=(48, 48, 48))
    with pytest.raises(ValueError, match="multiples of 32"):
        TripletPlan((9, 40, 40, 40), 3)
    with pytest.raises(ValueError):
        series_layout((9, 2, 8, 8, 8), 3)
    with pytest.raises(ValueError, match="set_stats"):
        TripletPlan((9, 32, 32, 32), 3, normalize="global").records()
    # a plan that leaves the array is refused on the host
    rec = TripletPlan((9, 32, 32, 32), 3, augment="none").records()
    bad = rec.copy()
    bad["off"][1, 2] = 9 * 32 ** 3 - 5
    with pytest.raises(ValueError, match="job 1"):
        ops.check_triplet_jobs(bad, 9 * 32 ** 3, (32, 32, 32), (32, 32, 32))
    bad = rec.copy()
    bad["x0"][2] = 1
    with pytest.raises(ValueError, match="job 2"):
        ops.check_triplet_jobs(bad, 9 * 32 ** 3, (32, 32, 32), (32, 32, 32))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.triplet_gather(torch.zeros(9, 32, 32, 32), rec[:1], (1, 3, 32, 32, 32))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.series_stats(torch.zeros(9, 32, dtype=torch.uint8))


def test_entry_points_validate_without_gpu():
    """Argument validation happens before any launch (null pointers 1, bad extents 2, unknown type 3)."""
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    ok = (0x1000, 3, 1 << 20, 8, 8, 8, 0x2000, 2, 8, 8, 8, 0x4000, None)
    sub = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for i in (0, 6, 11):
        assert L.fs_triplet_gather(*sub(i, None)) == 1
    for i, v in ((7, 0), (3, 0), (8, 9), (10, 16), (2, 100), (4, -1)):
        assert L.fs_triplet_gather(*sub(i, v)) == 2, (i, v)
    assert L.fs_triplet_gather(*sub(1, 4)) == 3 and L.fs_triplet_gather(*sub(1, -1)) == 3
    assert L.fs_triplet_gather(*sub(0, 0x1002)) == 3          # base not aligned to a float
    assert L.fs_series_stats(None, 0, 4, 64, 0x1000, 0x2000, None) == 1
    assert L.fs_series_stats(0x1000, 0, 4, 64, None, 0x2000, None) == 1
    assert L.fs_series_stats(0x1000, 0, 0, 64, 0x1000, 0x2000, None) == 2
    assert L.fs_series_stats(0x1000, 0, 4, 0, 0x1000, 0x2000, None) == 2
    assert L.fs_series_stats(0x1000, 7, 4, 64, 0x1000, 0x2000, None) == 3
    assert L.fs_series_stats_ws_bytes(0, 64) == -2 and L.fs_series_stats_ws_bytes(4, 1 << 24) > 0
    assert ops.TRIPLET_JOB.itemsize == 64 and ops.triplet_gather_cost(2, (256, 256, 256), 1) == (3 * 2 * 256 ** 3 * 5, 3 * 2 * 256 ** 3 * 2)
