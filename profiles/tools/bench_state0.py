"""What the learned initial LSTM state (`learn_zero_state`) costs: the TGT-shaped captured train step [1024, 256, 88, 5] of the joint LSTM-NADE
with the flag off, with it on (cluster / CU-resident recurrences), and with it on but forced onto the launch-per-timestep kernels.
Device-synchronised medians over the replays.  `--variant off|on|on-steps` runs one of them alone (for a kernel trace of its own).

    python profiles/tools/bench_state0.py [--replays 20] [--variant all]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from multinn_amd import RnnNade, AdamOptimizer   # noqa: E402


def median_step_ms(variant, B, T, P, M, replays, rho=0.03):
    dev = "cuda:0"
    x = torch.from_numpy((np.random.default_rng(23).random((B, T, P, M)) < rho).astype(np.uint8)).to(dev)
    gen = RnnNade(P * M, 256, [512, 256], keep_prob=0.9, precision="fp16", seed=23, learn_zero_state=(variant != "off"))
    gen._materialize(P * M)
    if variant != "off":
        for l, u in enumerate([512, 256]):
            gen.store[f"rnn/cell_{l}/c0"].copy_(torch.linspace(-0.3, 0.3, u, device=dev).view(1, u))
    if variant == "on-steps":
        gen._stack.cluster = gen._stack.resident = False          # no resident / cluster form: the stateful stack steps launch by launch
    opt = AdamOptimizer(0.01)
    run = gen.graphed_train_step(x, opt, warmup=2)
    forms = dict(rowpar=bool(gen._ctx["lstm"][0].get("rowpar")), state=gen._ctx["lstm"][0].get("c0") is not None)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    gen.check()
    return dict(variant=variant, ms_per_step=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), replays=replays, loss=float(run()), **forms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="all", choices=["all", "off", "on", "on-steps"])
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--shape", default="1024,256,88,5")
    a = ap.parse_args()
    B, T, P, M = (int(v) for v in a.shape.split(","))
    for v in (["off", "on", "on-steps"] if a.variant == "all" else [a.variant]):
        print(json.dumps(median_step_ms(v, B, T, P, M, a.replays)), flush=True)


if __name__ == "__main__":
    main()
