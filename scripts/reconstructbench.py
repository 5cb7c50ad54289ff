"""Writing an up-sampled series: is the output hidden behind inference?  On jets3d at 128^3 and 256^3, K = 9 stored
frames (uint8), exp = 2, written as uint8 and as float32 (chunk = 1, batch = 1, Flow-3D with random-init weights), in
one process:

  * ops.series_encode alone on one chunk's frames [3,1,S,S,S]: HIP events around `iters` calls after `warmup` calls,
    each call on the next of a ring of operand pairs larger than three times the 256 MiB Infinity Cache; the
    algorithmic bytes of ops.series_encode_cost (4 + itemsize per element) against the 8 TB/s HBM peak (AMD's
    MI355X spec; ~6.3 TB/s is what a float4 copy reaches);
  * reconstruct.reconstruct_series file to file (second of two runs): wall time, device-to-host time per chunk (events
    on the copy stream), host time placing frames into the memory map, host time waiting on copy events;
  * evaluate.interpolate_sequence alone on the same decoded keyframes (second of two runs, wall time around a device
    synchronise): the inference the driver cannot do without.

The expectation it checks: driver wall - inference-only wall <= 2 x the output time of one chunk (encode + copy +
placement), i.e. only the first fill and the last drain are not overlapped.  Records, not thresholds.

    python scripts/reconstructbench.py [--sizes 128 256] [--out profiles/series_reconstruct.txt]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opticalflowscivis_amd import ops  # noqa: E402
from opticalflowscivis_amd.data import synthetic  # noqa: E402
from opticalflowscivis_amd.data.series import SeriesWriter, load_series  # noqa: E402
from opticalflowscivis_amd.evaluate import interpolate_sequence  # noqa: E402
from opticalflowscivis_amd.reconstruct import normalisation, reconstruct_series  # noqa: E402

HBM_BPS = 8.0e12
K, EXP = 9, 2


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


CACHE_BYTES = 256 << 20  # the Infinity Cache: a working set that fits is served from it, not from HBM


def encode_alone(S, dtype, warmup, iters):
    """ms per ops.series_encode call on [3,1,S,S,S] with and without stats, over a ring of operand pairs that together
    hold three times the cache, so that no call finds its source or destination lines left there by an earlier one."""
    tdt = getattr(torch, np.dtype(dtype).name)
    nbytes, _ = ops.series_encode_cost((3, 1, S, S, S), np.dtype(dtype).itemsize)
    ring = [(torch.rand(3, 1, S, S, S, device="cuda"), torch.empty((3, 1, S, S, S), dtype=tdt, device="cuda"))
            for _ in range(-(-3 * CACHE_BYTES // nbytes) + 1)]
    turn = [0]

    def call(stats):
        x, out = ring[turn[0] % len(ring)]
        turn[0] += 1
        ops.series_encode(x, dtype, (S, S, S), lo=3.0, span=250.0, out=out, stats=stats)

    ms = timed(lambda: call(True), warmup, iters)
    ms_plain = timed(lambda: call(False), warmup, iters)
    return ms, ms_plain, nbytes, len(ring)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "reconstructbench needs a GPU"
    from opticalflowscivis_amd.flow3d.model.RIFE import Model
    torch.manual_seed(3)
    model = Model(-1, device=torch.device("cuda"))
    model.eval()
    lines = ["device: %s; K = %d stored uint8 frames, exp = %d (%d frames written, %d rebuilt), chunk 1, batch 1" % (
        torch.cuda.get_device_name(0), K, EXP, (K - 1) * 2 ** EXP + 1, (K - 1) * (2 ** EXP - 1))]
    factor = 2 ** EXP
    with tempfile.TemporaryDirectory() as tmp:
        for S in args.sizes:
            seq = synthetic.jets3d_sequence(K, S, 1234, device="cuda")
            src = os.path.join(tmp, "jets_%d.npy" % S)
            np.save(src, torch.round(seq.clamp(0, 1) * 255).to(torch.uint8).cpu().numpy())
            del seq
            stored = load_series(src, nd=3)
            # inference alone, on the keyframes as the driver decodes them
            lo, inv, _ = normalisation("global", (float(stored.min()), float(stored.max())))
            frames = torch.zeros(((K - 1) * factor + 1, S, S, S), device="cuda")
            frames[::factor] = (torch.from_numpy(np.asarray(stored)).cuda().float() - float(lo)) * float(inv)
            t_inf = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = interpolate_sequence(model, frames, factor, 1)
                torch.cuda.synchronize()
                t_inf.append(time.perf_counter() - t0)
            del frames
            lines.append("")
            lines.append("jets3d %d^3: interpolate_sequence alone %.3f s (first run %.3f s)" % (S, t_inf[1], t_inf[0]))
            for dtype in ("uint8", "float32"):
                ms, ms_plain, nbytes, ring = encode_alone(S, dtype, args.warmup, args.iters)
                runs = []
                for i in range(2):
                    with SeriesWriter(os.path.join(tmp, "out_%d_%s.npy" % (S, dtype)), ((K - 1) * factor + 1, S, S, S),
                                      dtype, overwrite=True) as w:
                        runs.append(reconstruct_series(model, stored, EXP, w, batch=1, chunk=1))
                r = runs[1]
                n = len(r["time_d2h_chunk_s"])
                d2h = float(np.median(r["time_d2h_chunk_s"]))
                place = r["time_place_s"] / n
                out_chunk = ms * 1e-3 + d2h + place
                extra = r["time_total_s"] - t_inf[1]
                got = np.load(os.path.join(tmp, "out_%d_%s.npy" % (S, dtype)), mmap_mode="r")
                same = dtype != "float32" or bool(np.array_equal(
                    np.asarray(got[1]), (ref[1].cpu().numpy() * np.float32(r["span"])) + np.float32(r["lo"])))
                lines += [
                    "  -> %s" % dtype,
                    "     series_encode [3,1,%d^3]: %.3f ms with stats (%.2f TB/s, %.2f of the 8 TB/s roof by %d algorithmic "
                    "bytes), %.3f ms without (%.2f of the roof); ring of %d operand pairs" % (
                        S, ms, nbytes / ms / 1e9, nbytes / HBM_BPS * 1e3 / ms, nbytes, ms_plain,
                        nbytes / HBM_BPS * 1e3 / ms_plain, ring),
                    "     driver: wall %.3f s (first run %.3f s), of it %.3f s in front of the first chunk (buffers, range "
                    "pass); device: model %.3f s, select + encode + stats copy %.4f s; "
                    "device-to-host per chunk %.2f ms (median of %d; %.1f GB/s); host: placement %.2f ms per chunk, "
                    "waits on copy events %.3f s" % (r["time_total_s"], runs[0]["time_total_s"], r["time_setup_s"], r["time_model_s"],
                                                       r["time_encode_s"], d2h * 1e3, n,
                                                       3 * S ** 3 * np.dtype(dtype).itemsize / d2h / 1e9, place * 1e3,
                                                       r["time_wait_s"]),
                    "     driver wall - inference alone = %.3f s; output time of one chunk (encode + copy + placement) = "
                    "%.4f s; expectation (difference <= 2 x that): %s; first rebuilt frame equals interpolate_sequence's: %s"
                    % (extra, out_chunk, "holds" if extra <= 2 * out_chunk else "DOES NOT HOLD", same)]
                for ln in lines[-4:]:
                    print(ln, flush=True)
            del ref
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
