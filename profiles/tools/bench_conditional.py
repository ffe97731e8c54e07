"""Conditioned vs unconditioned sampling scan at bench.py's sampling shape: joint LSTM-NADE, P 88, M 5 (D 440, Hn 256, LSTM [512, 256]),
72 intros x 32 steps -> 128 generated steps, one hipGraph replay per call.  Conditioned: one whole track given (codes of
multinn_amd.common.given_codes, feature p M + m).  The two scans alternate in one process; prints one JSON line of us per generated step.
`--only given` runs the conditioned scan alone (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import math
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from multinn_amd import RnnNade                      # noqa: E402
from multinn_amd.common import given_codes           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=72)
    ap.add_argument("--intro", type=int, default=32)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--track", type=int, default=1, help="the given track")
    ap.add_argument("--only", choices=["both", "given"], default="both")
    a = ap.parse_args()
    P, M, Hn = 88, 5, 256
    D = P * M
    dev = "cuda:0"
    R = np.random.default_rng(23)
    x = torch.from_numpy((R.random((a.n, a.intro, D)) < 0.03).astype(np.uint8)).to(dev)
    g = RnnNade(D, Hn, [512, 256], keep_prob=0.9, precision="fp16", seed=23)
    g._materialize(D)
    g.store["dense/bias"][Hn:Hn + D] = math.log(0.03 / 0.97)          # piano-roll-like conditionals (bench.py's second weight state)
    given = torch.from_numpy((R.random((a.n, a.steps, P, M)) < 0.05).astype(np.uint8)).to(dev)
    mask = torch.zeros(M, dtype=torch.bool)
    mask[a.track] = True
    codes = given_codes(given, mask).reshape(a.n, a.steps, D)

    def timed(c):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = g.generate(x, a.steps, given=c)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    forms = [("given", codes)] if a.only == "given" else [("plain", None), ("given", codes)]
    for _, c in forms:
        timed(c)                                                        # capture
    best = {k: float("inf") for k, _ in forms}
    dens = {}
    for _ in range(a.reps):
        for k, c in forms:
            t, out = timed(c)
            best[k] = min(best[k], t)
            dens[k] = float(out.float().mean())
    res = {"n": a.n, "intro": a.intro, "steps": a.steps, "given_track": a.track, "reps": a.reps}
    for k, _ in forms:
        res[k] = {"us_per_step": round(1e6 * best[k] / a.steps, 2), "density": round(dens[k], 4)}
    if "plain" in res:
        res["given_over_plain"] = round(best["given"] / best["plain"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
