"""-m gpu: fs_triplet_gather / fs_series_stats against numpy (bit for bit), the guard against records that leave the
array, DeviceSeriesLoader against DataLoader(FileTriplets), and `train --series` / `evaluate --seq` end to end."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from opticalflowscivis_amd import _lib, ops
from opticalflowscivis_amd.data import synthetic
from opticalflowscivis_amd.data.series import (DeviceSeriesLoader, FileTriplets, TripletPlan, frame_stats_numpy,
                                               gather_numpy)

from series_ref import ref_triplets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.uint8, np.uint16, np.float16, np.float32)


def _random(shape, dtype, seed, special=False):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.integer):
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    a = (rng.standard_normal(shape) * 3).astype(dtype)
    if special:
        f = a.reshape(-1)
        idx = rng.choice(f.size, size=max(3, f.size // 50), replace=False)
        f[idx[0::3]], f[idx[1::3]], f[idx[2::3]] = np.nan, np.inf, -np.inf
    return a


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _expect(flat, n_elems, rec, frame, crop):
    """The entry point's contract in numpy, records of any kind: a source coordinate outside the frame or an element
    index outside [0, n_elems) reads as 0; non-finite -> 0; (v - lo) * inv in fp32."""
    Ds, Hs, Ws = frame
    Do, Ho, Wo = crop
    z, y, x = np.meshgrid(np.arange(Do), np.arange(Ho), np.arange(Wo), indexing="ij")
    fl = int(rec["flip"])
    zs = int(rec["z0"]) + (Do - 1 - z if fl & 4 else z)
    ys = int(rec["y0"]) + (Ho - 1 - y if fl & 2 else y)
    xs = int(rec["x0"]) + (Wo - 1 - x if fl & 1 else x)
    inside = (zs >= 0) & (zs < Ds) & (ys >= 0) & (ys < Hs) & (xs >= 0) & (xs < Ws)
    out = np.empty((3, Do, Ho, Wo), np.float32)
    for c in range(3):
        e = int(rec["off"][c]) + (zs * Hs + ys) * Ws + xs
        ok = inside & (e >= 0) & (e < n_elems)
        v = np.where(ok, flat[np.clip(e, 0, n_elems - 1)].astype(np.float32), np.float32(0))
        v = np.where(np.isfinite(v), v, np.float32(0)).astype(np.float32)
        out[c] = (v - np.float32(rec["lo"])) * np.float32(rec["inv"])
    return out


def _records(rng, B, frames_or_items, layout, frame, crop, aligned, flip, norm):
    F = int(np.prod(frame))
    rec = np.zeros(B, ops.TRIPLET_JOB)
    for b in range(B):
        if layout == "series":
            rec["off"][b] = rng.choice(frames_or_items, 3, replace=False) * F
        else:
            rec["off"][b] = (3 * rng.integers(frames_or_items) + np.arange(3)) * F
        for k, name in enumerate(("z0", "y0", "x0")):
            r = frame[k] - crop[k]
            o = int(rng.integers(r + 1))
            rec[name][b] = o // 4 * 4 if (aligned and name == "x0") else o
        if not aligned and frame[2] > crop[2]:
            rec["x0"][b] = min(frame[2] - crop[2], rec["x0"][b] | 1)
        rec["flip"][b] = flip
        rec["lo"][b], rec["inv"][b] = (rng.standard_normal(), 1 / (0.5 + rng.random())) if norm else (0, 1)
    return rec


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Ws", (64, 57))
def test_gather_matches_numpy_bit_for_bit(dtype, Ws):
    rng = np.random.default_rng(Ws + np.dtype(dtype).itemsize)
    cases = [  # (frame, crop): 3-D with a partial last tile of the grid, Ds = 1 (the 2-D models), full frame
        ((6, 20, Ws), (5, 12, 40)), ((1, 40, Ws), (1, 32, 44)), ((4, 8, Ws), (4, 8, Ws)), ((5, 9, Ws), (3, 7, 37))]
    for frame, crop in cases:
        for layout, shape in (("series", (9,) + frame), ("triplets", (4, 3) + frame)):
            src = _random(shape, dtype, int(rng.integers(1 << 30)), special=True)
            stored, flat = _dev(src), src.reshape(-1)
            for flip in range(8):
                for aligned in (True, False):
                    for norm in (False, True):
                        rec = _records(rng, 3, shape[0], layout, frame, crop, aligned, flip, norm)
                        got = ops.triplet_gather(stored, rec, (3, 3) + crop).cpu().numpy()
                        for b in range(3):
                            want = _expect(flat, flat.size, rec[b], frame, crop)
                            assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), \
                                (dtype, frame, crop, layout, flip, aligned, norm, b)
                            if not norm:  # ... and the host loaders' numpy gather is the same function
                                assert np.array_equal(gather_numpy(src, rec[b], frame, crop).view(np.uint32),
                                                      want.view(np.uint32))
    # the 2-D form of the op: [T,H,W] stored, [B,3,H,W] out
    src = _random((5, 40, Ws), dtype, 7)
    rec = _records(rng, 2, 5, "series", (1, 40, Ws), (1, 32, 32), False, 3, True)
    got = ops.triplet_gather(_dev(src), rec, (2, 3, 32, 32)).cpu().numpy()
    for b in range(2):
        assert np.array_equal(got[b], _expect(src.reshape(-1), src.size, rec[b], (1, 40, Ws), (1, 32, 32))[:, 0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_records_that_leave_the_array_read_zero(dtype):
    """Past ops' validation, straight to the C entry point.  The array handed over is a WINDOW inside a larger
    allocation of this test, filled with a sentinel, and no bad record points further than that padding: a kernel
    without the guard returns the sentinel (and fails the comparison), it never touches unmapped memory."""
    frame, crop, T = (4, 8, 16), (3, 6, 12), 5
    F = int(np.prod(frame))
    n, pad = T * F, 2 * F
    sentinel = 77
    big = np.full(pad + n + pad, sentinel, dtype)
    src = _random((n,), dtype, 11)
    src[src == sentinel] = 1
    big[pad:pad + n] = src
    whole = _dev(big)
    window = whole[pad:pad + n]
    rec = np.zeros(6, ops.TRIPLET_JOB)
    rec["inv"] = 1
    rec["off"][:] = (0, F, 2 * F)
    rec["off"][0] = (-F // 2, F, 2 * F)             # starts before the array
    rec["off"][1] = (0, n - F // 3, 4 * F)          # runs past its end
    rec["off"][2] = (n + 5, -F - 7, 0)              # wholly outside, both sides
    rec["z0"][3], rec["y0"][3], rec["x0"][3] = 2, 4, 8   # origin + extent beyond the frame
    rec["x0"][4], rec["flip"][4] = -3, 5            # a negative origin, mirrored
    rec["off"][5] = (1, F + 2, 2 * F + 3)           # in range but odd: the element path
    jobs = torch.from_numpy(rec.view("<i8").reshape(-1, 8)).cuda()
    out = torch.full((6, 3) + crop, -1.0, device="cuda")
    rc = _lib.lib().fs_triplet_gather(window.data_ptr(), ops.SERIES_DTYPES[window.dtype], n, *frame, jobs.data_ptr(),
                                      6, *crop, out.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    zeros = 0
    for b in range(6):
        want = _expect(src, n, rec[b], frame, crop)
        assert np.array_equal(got[b], want), b
        zeros += int((want == 0).sum())
    assert zeros > 500 and not (got == sentinel).any()
    assert (whole[:pad] == sentinel).all() and (whole[pad + n:] == sentinel).all()
    with pytest.raises(ValueError, match="leaves the stored array"):
        ops.triplet_gather(window.view((T,) + frame), rec, (6, 3) + crop)


@pytest.mark.parametrize("dtype", DTYPES)
def test_series_stats_exact(dtype):
    for shape in ((5, 3, 7, 11), (3, 1 << 24), (4, 64, 64)):
        src = _random(shape, dtype, 13, special=True)
        got = ops.series_stats(_dev(src)).cpu().numpy()
        want = frame_stats_numpy(src, shape[0])
        assert np.array_equal(got, want), (dtype, shape, got[:2], want[:2])
    if dtype == np.float32:
        src = np.full((2, 64), np.nan, np.float32)
        src[1, 5] = 2.5
        got = ops.series_stats(_dev(src)).cpu().numpy()
        assert got[0].tolist() == [np.inf, -np.inf, 64] and got[1].tolist() == [2.5, 2.5, 63]


def test_device_loader_yields_the_dataloaders_batches():
    src = _random((30, 64, 32, 64), np.uint16, 17)
    plan = TripletPlan(src.shape, 3, stop=24, augment="full", crop=(32, 32, 32), normalize="global", seed=3)
    ds = FileTriplets(src, plan)
    for sampler in (None, "dist"):
        samp = DistributedSampler(ds, num_replicas=2, rank=1, shuffle=True) if sampler else None
        dev = DeviceSeriesLoader(ds, 3, "cuda", sampler=samp, drop_last=True)
        for epoch in range(2):
            ds.set_epoch(epoch)
            if samp is not None:
                samp.set_epoch(epoch)
            host = list(DataLoader(ds, batch_size=3, sampler=samp, drop_last=True))
            got = [b.cpu() for b in dev]
            assert len(got) == len(host) == len(dev) > 2
            for a, b in zip(got, host):
                assert a.shape == (3, 3, 32, 32, 32) and torch.equal(a, b)
    ds.set_epoch(0)
    dev = DeviceSeriesLoader(ds, 5, "cuda")   # a partial last batch, sequential order
    got = [b.cpu() for b in dev]
    assert [len(b) for b in got] == [5] * (len(ds) // 5) + [len(ds) % 5]
    assert torch.equal(torch.cat(got), torch.stack([ds[i] for i in range(len(ds))]))
    # between the epoch's first and last batch: no copy, no synchronisation
    it = iter(dev)
    batches = [next(it)]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in it:
            batches.append(b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(torch.cat(batches).cpu(), torch.cat(got))


_CHILD = """
import json, runpy, sys, torch
torch.use_deterministic_algorithms(True)
from opticalflowscivis_amd.flow%(nd)dd.model.RIFE import Model
losses, _update = [], Model.update
def update(self, *a, **k):
    r = _update(self, *a, **k)
    if k.get("training", True):
        losses.append(float(r[1]["loss_G"]).hex())
    return r
Model.update = update
sys.argv = ["train"] + %(argv)r
try:
    runpy.run_module("opticalflowscivis_amd.flow%(nd)dd.train", run_name="__main__")
finally:
    json.dump(losses, open(%(out)r, "w"))
"""


@pytest.mark.parametrize("nd", (3, 2))
def test_train_on_a_series_file(tmp_path, nd):
    from opticalflowscivis_amd import trainer
    if nd == 3:
        seq = synthetic.droplet3d_sequence(24, 32, seed=5, radius=(6, 12))
    else:
        seq = synthetic.droplet2d_sequence(24, 64, 96, seed=5, radius=(8, 16))
    data = np.round(seq.numpy() * 255).astype(np.uint8)
    path = str(tmp_path / "frames.npy")
    np.save(path, data)
    argv = ["--series", path, "--mode", "train", "--epoch", "1", "--batch_size", "2", "--eager", "--log_every", "1",
            "--log_path", str(tmp_path)] + (["--crop", "32"] if nd == 3 else [])
    out_json = str(tmp_path / "losses.json")
    r = subprocess.run([sys.executable, "-c", _CHILD % {"nd": nd, "argv": argv, "out": out_json}], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0, (out[-1500:], r.stderr.decode()[-3000:])
    m = re.search(r"eval epoch 0: loss_G ([-+0-9.e]+)\s+PSNR ([-+0-9.]+) dB", out)
    assert m and np.isfinite(float(m.group(2))) and "device-resident series" in out
    assert os.path.exists(os.path.join(str(tmp_path), "flownet.pkl"))
    child = [float.fromhex(h) for h in json.load(open(out_json))]
    # by hand: the restatement's batches (load_datasets.py:138-183), the trainer's order, seeds and learning rates
    rt, _ = ref_triplets(data if nd == 3 else data[:, None, None], 18)
    if nd == 2:
        rt = rt[:, :, 0]
    lo, hi = np.float32(data.min()), np.float32(data.max())
    rt = (rt - lo) * (np.float32(1) / (hi - lo))
    assert len(rt) == 24 and len(child) == 12
    Model = __import__("opticalflowscivis_amd.flow%dd.model.RIFE" % nd, fromlist=["Model"]).Model
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        np.random.seed(1234)
        torch.manual_seed(1234)
        model = Model(-1, device=torch.device("cuda", 0))
        order = torch.randperm(24, generator=torch.Generator().manual_seed(1234)).tolist()
        for step in range(3):
            batch = torch.from_numpy(rt[order[2 * step:2 * step + 2]]).cuda()
            lr = trainer.get_learning_rate(step, 2001) / 4
            args = (batch[:, :2], batch[:, 2:3]) + (("series",) if nd == 2 else ()) + (lr,)
            _, info = model.update(*args, training=True)
            assert float(info["loss_G"]) == child[step], (step, float(info["loss_G"]), child[step])
    finally:
        torch.use_deterministic_algorithms(was)


def test_evaluate_seq_numbers_unchanged(tmp_path):
    """--seq on a .npy in [0,1] goes through load_series now: the same numbers as the array handed over directly.
    On the Flow-3D model, whose forward kernels are bitwise reproducible (the 2-D model's MIOpen convolutions differ in
    the last digits from one call to the next, so two evaluations of the same input are not equal there)."""
    from opticalflowscivis_amd import evaluate
    from opticalflowscivis_amd.flow3d.model.RIFE import Model
    seq = synthetic.droplet3d_sequence(9, 32, seed=2, radius=(6, 12))
    path = str(tmp_path / "seq.npy")
    np.save(path, seq.numpy())
    torch.manual_seed(7)
    doc = evaluate.main(Model, 3, ["--seq", path, "--exp", "1", "2", "--model", str(tmp_path)])
    torch.manual_seed(7)
    model = Model(-1, device=torch.device("cuda"))
    model.eval()
    before = evaluate.evaluate_sequence(model, torch.from_numpy(np.load(path).astype(np.float32)).cuda(), [1, 2], 1, False)
    strip = lambda rs: [{k: v for k, v in r.items() if not k.startswith("time")} for r in rs]
    assert json.dumps(strip(doc["results"])) == json.dumps(strip(before))
    # a uint8 file scored after --normalize global is the same sequence up to its quantisation
    np.save(path, np.round(seq.numpy() * 255).astype(np.uint8))
    assert evaluate._load_seq(path, 3, "global").max() == 1.0
    assert torch.equal(evaluate._load_seq(path, 3), torch.from_numpy(np.load(path).astype(np.float32)))
