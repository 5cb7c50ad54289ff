"""-m gpu: `--val_series` scales the validation file by the training file's range on the host and the device path
alike; the trainer redraws crops per epoch; `--host_cache` refuses what it cannot redraw."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from opticalflowscivis_amd import trainer
from opticalflowscivis_amd.data.series import DeviceSeriesLoader, gather_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(tmp_path, extra=()):
    import argparse
    rng = np.random.default_rng(4)
    tr, va = str(tmp_path / "train.npy"), str(tmp_path / "val.npy")
    np.save(tr, rng.integers(0, 256, size=(9, 32, 32, 32), dtype=np.uint8))
    np.save(va, rng.integers(40, 90, size=(6, 32, 32, 32), dtype=np.uint8))
    return trainer.add_common_args(argparse.ArgumentParser(), 3).parse_args(
        ["--series", tr, "--val_series", va] + list(extra)), tr, va


def test_validation_file_is_scaled_like_the_training_file_on_both_paths(tmp_path):
    args, tr, va = _args(tmp_path)
    lo, hi = np.float32(np.load(tr).min()), np.float32(np.load(tr).max())
    want = (np.float32(np.load(va)[[0, 2, 1]]) - lo) * (np.float32(1) / (hi - lo))
    batches = {}
    for path in ("host", "device"):
        train_set, val_set = trainer.series_sets(args, 3, 1234)
        if path == "device":
            DeviceSeriesLoader(train_set, 2, "cuda")
            val_data = DeviceSeriesLoader(val_set, 2, "cuda")
        trainer.share_norm_range(train_set, val_set, args)
        if path == "host":
            val_data = DataLoader(val_set, batch_size=2)
        batches[path] = torch.cat([b.cpu() for b in val_data])
        assert np.array_equal(batches[path][0].numpy(), want), path
    assert torch.equal(batches["host"], batches["device"]) and batches["host"].max() < 0.4


_CHILD = """
import json, runpy, sys, torch
from opticalflowscivis_amd.flow3d.model.RIFE import Model
sums, _update = [], Model.update
def update(self, imgs, gt, *a, **k):
    if k.get("training", True):
        sums.append([float(imgs.double().sum()), float(gt.double().sum())])
    return _update(self, imgs, gt, *a, **k)
Model.update = update
sys.argv = ["train"] + %(argv)r
try:
    runpy.run_module("opticalflowscivis_amd.flow3d.train", run_name="__main__")
finally:
    json.dump(sums, open(%(out)r, "w"))
"""


def test_trainer_redraws_crops_every_epoch(tmp_path):
    import argparse
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, size=(12, 64, 64, 64), dtype=np.uint8)
    path, out = str(tmp_path / "frames.npy"), str(tmp_path / "sums.json")
    np.save(path, data)
    argv = ["--series", path, "--mode", "train", "--epoch", "2", "--batch_size", "1", "--eager", "--crop", "32",
            "--augment", "none", "--normalize", "none", "--val_from", "9", "--log_path", str(tmp_path)]
    r = subprocess.run([sys.executable, "-c", _CHILD % {"argv": argv, "out": out}], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, (r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    got = json.load(open(out))
    args = trainer.add_common_args(argparse.ArgumentParser(), 3).parse_args(argv)
    train_set, _ = trainer.series_sets(args, 3, 1234)
    assert len(train_set) == 3 and len(got) == 6
    gen = torch.Generator().manual_seed(1234)
    want, origins = [], []
    for epoch in range(2):
        train_set.set_epoch(epoch)
        origins.append(train_set.records()[["z0", "y0", "x0"]].tolist())
        for i in torch.randperm(3, generator=gen).tolist():
            item = gather_numpy(data, train_set.records()[i], (64, 64, 64), (32, 32, 32)).astype(np.float64)
            want.append([item[:2].sum(), item[2:].sum()])
    assert origins[0] != origins[1]
    assert got == want


def test_host_cache_refuses_what_it_cannot_redraw(tmp_path):
    from opticalflowscivis_amd.flow3d.model.RIFE import Model
    for extra in (["--augment", "full"], []):
        args, tr, _ = _args(tmp_path, ["--host_data", "--host_cache", "--log_path", str(tmp_path)] + extra)
        if not extra:
            np.save(tr, np.zeros((9, 64, 64, 64), np.uint8))
            args.crop = [32]
        with pytest.raises(ValueError, match="host_cache"):
            trainer.run(args, Model, 3)
