"""Wall-clock per step of driver.train_epoch fed from a NumPy array (the host path: fancy-index gather, pageable copy, a loss read per
step) and from a DeviceDataset (window_gather on the device, one loss read-back per epoch), on synthetic songs of bench.py's density.

    python profiles/tools/bench_device_dataset.py [--workload c2 tgt] [--songs 2048] [--pieces 4] [--epochs 10] [--repeat 2] [--precision fp16]

Every song has `pieces` windows of the workload's length, so all windows are full-length and of one shape: the first two steps of the first
epoch run eagerly (the second captures the step), everything after replays the graph.  Per epoch: time.perf_counter around train_epoch with a
final torch.cuda.synchronize(); the SECOND epoch is the figure, the later ones show its spread.  The two input types alternate `repeat` times
in one process, each time on a fresh generator.  Prints one JSON line per (workload, input type, repeat).  Figures: profiles/device_dataset.md."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from bench import WORKLOADS, HN, UNITS                                       # noqa: E402
from multinn_amd import RnnNade, AdamOptimizer, DeviceDataset                # noqa: E402
from multinn_amd.driver import train_epoch, LossAccumulator, TrainingStats  # noqa: E402


def songs(S, T, P, M, rho, seed=23, slab=64):
    rng = np.random.Generator(np.random.PCG64(seed))
    X = np.empty((S, T, P, M), np.uint8)
    for s in range(0, S, slab):
        X[s:s + slab] = rng.random((min(slab, S - s), T, P, M)) < rho
    return X


def window_rate(X, B, Tw, calls=200):
    """DeviceDataset.window alone at the workload's window: device time per call between two HIP events around `calls` gathers (joint row,
    then one track), and the bytes moved (read + written) over it."""
    ds = DeviceDataset(X)
    ids = np.random.default_rng(0).permutation(len(ds))[:B]
    ids_dev = ds.upload_ids(ids)
    out = {}
    for name, track in (("joint", None), ("track", 2)):
        for _ in range(10):
            x, _ = ds.window(ids, Tw, Tw, track=track, ids_dev=ids_dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(calls):
            ds.window(ids, Tw, Tw, track=track, ids_dev=ids_dev)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / calls
        out[name] = {"us_per_call_device": round(us, 2), "us_per_call_host": round((time.perf_counter() - t0) * 1e6 / calls, 2),
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
        for kind in ("numpy", "device") * a.repeat:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data = X if kind == "numpy" else DeviceDataset(X)
            torch.cuda.synchronize()
            upload = time.perf_counter() - t0
            gen = RnnNade(P * M, HN, UNITS, keep_prob=0.9, precision=a.precision, seed=23)
            gen._materialize(P * M)
            opt, stats, ids, ms, losses = AdamOptimizer(0.01), TrainingStats(), np.arange(a.songs), [], []
            for epoch in range(1, a.epochs + 1):
                np.random.seed(epoch)
                np.random.shuffle(ids)
                acc = LossAccumulator()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train_epoch(gen, data, None if kind == "device" else np.full(a.songs, X.shape[1]), ids, B, T, opt, acc, stats, lr=0.01)
                torch.cuda.synchronize()
                n = acc.finite_n + acc.num_bad()
                ms.append((time.perf_counter() - t0) * 1e3 / n)
                losses.append(acc.loss())
            gen.check()
            print(json.dumps({"workload": name, "window": [B, T, P, M], "input": kind, "songs": a.songs, "steps_per_epoch": n, "bytes": int(X.size),
                              "upload_s": round(upload, 3) if kind == "device" else None, "ms_per_step_by_epoch": [round(v, 3) for v in ms],
                              "ms_per_step": round(ms[1], 3), "later_epochs_min_median_max": [round(v, 3) for v in (min(ms[1:]), float(np.median(ms[1:])), max(ms[1:]))],
                              "loss_by_epoch": [round(v, 4) for v in losses], "graphs": len(gen._step_graphs)}), flush=True)
            del gen, data, opt
            torch.cuda.empty_cache()
        print(json.dumps({"workload": name, "window": [B, T, P, M], "window_gather": window_rate(X, B, T)}), flush=True)


if __name__ == "__main__":
    main()
