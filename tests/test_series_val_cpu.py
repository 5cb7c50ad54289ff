"""CPU: a validation set scaled by the training file's range keeps that range; training crops start on multiples of 4
along W; `evaluate --seq` refuses what is not a series."""
import numpy as np
import pytest

from opticalflowscivis_amd import evaluate
from opticalflowscivis_amd.data.series import FileTriplets, TripletPlan


def test_validation_set_keeps_a_foreign_range():
    rng = np.random.default_rng(1)
    val = rng.integers(10, 100, size=(6, 32, 32), dtype=np.uint8)
    plan = TripletPlan(val.shape, 2, train=False, normalize="global")
    plan.norm_range = (0.0, 255.0)                 # as trainer.run assigns it, before any statistics exist
    ds = FileTriplets(val, plan)
    item = ds[0].numpy()
    assert plan.norm_range == (0.0, 255.0)
    want = (np.float32(val[[0, 2, 1]]) - np.float32(0)) * (np.float32(1) / np.float32(255))
    assert np.array_equal(item, want) and item.max() < 0.5
    plan.set_stats(plan.stats)                      # statistics again: the range stays
    assert plan.global_range() == (0.0, 255.0)
    plan.set_stats(plan.stats, norm_range=(1.0, 2.0))
    assert plan.global_range() == (1.0, 2.0)
    own = FileTriplets(val, TripletPlan(val.shape, 2, train=False, normalize="global"))[0].numpy()
    assert own.max() == 1.0                         # without a foreign range: the file's own


def test_training_crops_start_on_multiples_of_four_along_w():
    p = TripletPlan((40, 64, 96, 100), 3, augment="none", crop=(32, 32, 32), stride=1)
    r = np.concatenate([p.records(e) for e in range(4)])
    assert (r["x0"] % 4 == 0).all() and 0 <= r["x0"].min() and r["x0"].max() <= 68 and len(np.unique(r["x0"])) > 8
    assert (r["y0"] % 4 != 0).any()


def test_evaluate_seq_refuses_triplets_and_wrong_rank(tmp_path):
    np.save(tmp_path / "t.npy", np.zeros((4, 3, 8, 8), np.float32))
    with pytest.raises(ValueError, match="triplets"):
        evaluate._load_seq(str(tmp_path / "t.npy"), 2)
    np.save(tmp_path / "r.npy", np.zeros((4, 2, 8, 8, 8), np.float32))
    with pytest.raises(ValueError):
        evaluate._load_seq(str(tmp_path / "r.npy"), 3)
    a = np.random.default_rng(0).random((4, 8, 8)).astype(np.float32)
    a[0, 0, 0] = np.nan
    np.save(tmp_path / "s.npy", a)
    got = evaluate._load_seq(str(tmp_path / "s.npy"), 2).numpy()
    assert np.isnan(got[0, 0, 0]) and np.array_equal(got[1:], a[1:])      # 'none' passes the values through
    assert np.isfinite(evaluate._load_seq(str(tmp_path / "s.npy"), 2, "global").numpy()).all()
