"""What transposition inside the window gather costs: (a) DeviceDataset.window with and without per-row shifts, joint row and one track,
device time between two HIP events; (b) wall-clock per step of driver.train_epoch on a DeviceDataset with and without
Transpose(6, fixed_tracks=(0,)), on synthetic songs of bench.py's density.

    python profiles/tools/bench_transpose_augment.py [--workload c2 tgt] [--songs 2048] [--pieces 4] [--epochs 10] [--repeat 2] [--precision fp16]

(a) 200 calls per form after 10 warm-up calls; the plain figure is mnn_window_gather's (the kernel this change leaves alone), measured in
the same process right beside the shifted one.  Shifts: uniform in -6..6 per row, every track but track 0 moving.
(b) as bench_device_dataset.py: every song has `pieces` windows of the workload's length, so every window is full-length and of one shape
and all but the first two steps replay one captured graph; time.perf_counter around train_epoch, ended by a device synchronise; plain and
augmented epochs alternate `repeat` times in one process, each time on a fresh generator and ONE dataset (uploaded once).  Prints one JSON
line per measurement; an f16 overflow that made the optimiser skip a step is reported there (overflow_warnings), not raised.  Figures: profiles/transpose_augment.md."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from bench import WORKLOADS, HN, UNITS                                       # noqa: E402
from multinn_amd import RnnNade, AdamOptimizer, DeviceDataset                # noqa: E402
from multinn_amd.data import Transpose                                       # noqa: E402
from multinn_amd.driver import train_epoch, LossAccumulator, TrainingStats  # noqa: E402
from bench_device_dataset import songs                                       # noqa: E402


def window_rate(ds, B, Tw, calls=200):
    """µs per DeviceDataset.window call (device events, and the host clock around the same loop) for the plain and the shifted gather."""
    M = ds.shape[3]
    ids = np.random.default_rng(0).permutation(len(ds))[:B]
    ids_dev = ds.upload_ids(ids)
    shifts_dev = torch.from_numpy(np.random.default_rng(1).integers(-6, 7, B).astype(np.int32)).to(ds.device)
    out = {}
    for form, track in (("joint", None), ("track", 2)):
        for kind, kw in (("plain", {}), ("shift", dict(shifts_dev=shifts_dev, moving=(1 << M) - 2)), ("plain_again", {})):
            for _ in range(10):
                x, _ = ds.window(ids, Tw, Tw, track=track, ids_dev=ids_dev, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(calls):
                ds.window(ids, Tw, Tw, track=track, ids_dev=ids_dev, **kw)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / calls
            out[f"{form}/{kind}"] = {"us_per_call_device": round(us, 2), "us_per_call_host": round((time.perf_counter() - t0) * 1e6 / calls, 2),
                                     "bytes_out": x.numel(), "GBps_read_plus_write": round(2 * x.numel() / us / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["c2", "tgt"], choices=["c2", "tgt", "tiny"])
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--pieces", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rho", type=float, default=0.03)
    a = ap.parse_args()
    for name in a.workload:
        w = WORKLOADS[name]
        B, T, P, M = w["B"], w["T"], w["P"], w["M"]
        X = songs(a.songs, a.pieces * T, P, M, a.rho)
        X[:, :, :8] = X[:, :, -8:] = 0                                       # room for the shifts: songs that fill the axis are never moved
        ds = DeviceDataset(X)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lo, hi = ds.extents(tuple(range(1, M)))
        print(json.dumps({"workload": name, "pitch_extent_s": round(time.perf_counter() - t0, 4), "lo_min": int(lo.min()), "hi_max": int(hi.max())}), flush=True)
        print(json.dumps({"workload": name, "window": [B, T, P, M], "window_gather": window_rate(ds, B, T)}), flush=True)
        for kind in ("plain", "transpose") * a.repeat:
            augment = Transpose(6, fixed_tracks=(0,)) if kind == "transpose" else None
            gen = RnnNade(P * M, HN, UNITS, keep_prob=0.9, precision=a.precision, seed=23)
            gen._materialize(P * M)
            opt, stats, ids, ms, losses, moved = AdamOptimizer(0.01), TrainingStats(), np.arange(a.songs), [], [], None
            for epoch in range(1, a.epochs + 1):
                stats.new_epoch()
                np.random.seed(epoch)
                np.random.shuffle(ids)
                acc = LossAccumulator()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if augment is None:
                    train_epoch(gen, ds, None, ids, B, T, opt, acc, stats, lr=0.01)
                else:
                    train_epoch(gen, ds, None, ids, B, T, opt, acc, stats, lr=0.01, augment=augment)
                torch.cuda.synchronize()
                n = acc.finite_n + acc.num_bad()
                ms.append((time.perf_counter() - t0) * 1e3 / n)
                losses.append(acc.loss())
            if augment is not None:
                moved = float((augment.shifts((lo, hi), 2, P) != 0).mean())
            with warnings.catch_warnings(record=True) as skipped:            # f16 overflows are the dynamic loss scale's business, as in driver.fit
                warnings.simplefilter("always")
                gen.check(tolerate_overflow=True)
            print(json.dumps({"workload": name, "window": [B, T, P, M], "input": kind, "songs": a.songs, "steps_per_epoch": n,
                              "songs_moved_epoch_2": moved, "ms_per_step_by_epoch": [round(v, 3) for v in ms], "ms_per_step": round(ms[1], 3),
                              "later_epochs_min_median_max": [round(v, 3) for v in (min(ms[1:]), float(np.median(ms[1:])), max(ms[1:]))],
                              "loss_by_epoch": [round(v, 4) for v in losses], "graphs": len(gen._step_graphs),
                              "overflow_warnings": [str(w.message) for w in skipped]}), flush=True)
            del gen, opt
            torch.cuda.empty_cache()
        del ds
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
