"""Ragged prompts: what the sampling scan costs with and without per-row prompt lengths (profiles/ragged_prompts.md).

    python profiles/tools/bench_ragged_prompts.py [--root DIR] [--reps N] [--tag NAME]

The sampling shape of DESIGN.md section 6: 72 intros of 32 steps, D = 440, NADE 256, LSTM [512, 256], the bench model.  Every figure is a
host clock around generate() ending in a device synchronise (one hipGraph replay per call), the minimum and the median of N calls after
the capture and a warm-up; us_per_step is the slope between the scans of 128 and of 8 generated steps, intro_ms their common intercept
(intro pass + packing + the first Dense).  --root: the tree whose multinn_amd is imported (a checkout of the parent commit, to alternate
with this one); a tree without `lengths` reports the plain call alone.  One JSON line."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--tag", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))

import numpy as np      # noqa: E402
import torch            # noqa: E402
from multinn_amd import RnnNade   # noqa: E402

B, TI, D, LONG, SHORT = 72, 32, 440, 128, 8


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), statistics.median(ts)


def scan(gen, x, reps, **kw):
    """-> dict: the 128-step and 8-step calls (min, median, seconds), the slope per generated step and the intercept."""
    long_, short = timed(lambda: gen.generate(x, LONG, **kw), reps), timed(lambda: gen.generate(x, SHORT, **kw), reps)
    per_step = (long_[0] - short[0]) / (LONG - SHORT)
    return {"s128_min": long_[0], "s128_med": long_[1], "s8_min": short[0], "s8_med": short[1], "us_per_step": 1e6 * per_step,
            "intro_ms": 1e3 * (short[0] - SHORT * per_step)}


def main():
    assert torch.cuda.is_available(), "a measurement needs the device"
    R = np.random.default_rng(23)
    x = torch.from_numpy((R.random((B, TI, D)) < 0.03).astype(np.uint8)).to("cuda:0")
    gen = RnnNade(D, 256, [512, 256], keep_prob=0.9, precision="bf16", seed=23)
    out = {"tag": a.tag, "root": os.path.abspath(a.root), "rows": B, "intro": TI, "reps": a.reps, "plain": scan(gen, x, a.reps)}
    if "lengths" in inspect.signature(gen.generate).parameters:
        uniform = R.integers(TI // 2, TI + 1, B).tolist()
        out["uniform_half_to_full"] = scan(gen, x, a.reps, lengths=uniform)
        # the all-frozen-tile short cut: rows 64..71 are the third tile.  "frozen": they end after one step, so that tile only copies for
        # 31 of the 32 intro steps; "live": they run to the end.  Row 0 is one step short in both, so both run the ragged instantiation.
        base = [TI - 1] + [TI] * (B - 1)
        out["third_tile_live"] = scan(gen, x, a.reps, lengths=base)
        out["third_tile_frozen"] = scan(gen, x, a.reps, lengths=base[:64] + [1] * 8)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
