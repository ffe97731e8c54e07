"""Conditioned vs unconditioned sampling with RBM generators: jamming mode at the C3 widths (tests/test_gpu_realmodes.py) -- 5 tracks of
RnnRBM(88 visibles, 256 hidden, LSTM [512, 256], CD-10) -- n intros x `intro` steps -> `steps` generated steps, every generator's scan one
hipGraph replay per call.  Three cases, alternated in one process:
  plain  no given;
  track  one whole track given (jamming mode pastes it: the other four generators run their free chains);
  pitch  a [P, M] pitch-range mask, the lowest `--low` pitches of every track given (all five generators run the clamped chain).
Prints one JSON line of us per generated step (best of --reps).  `--only pitch` runs one case alone (for a `rocprofv3 --kernel-trace
--stats` run of its own)."""
import argparse
import json
import math
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from multinn_amd import MultINN                      # noqa: E402

P, M, HN, UNITS, K = 88, 5, 256, [512, 256], 10
TRACKS = ["Drums", "Piano", "Guitar", "Bass", "Strings"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=72)
    ap.add_argument("--intro", type=int, default=16)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--track", type=int, default=1, help="the given track of the `track` case")
    ap.add_argument("--low", type=int, default=44, help="given pitches per track of the `pitch` case")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--only", choices=["all", "plain", "track", "pitch"], default="all")
    a = ap.parse_args()
    dev = "cuda:0"
    config = {"model_name": "bench", "data": {"pitch_range": {"lowest": 0, "highest": P}, "instruments": TRACKS, "beat_resolution": 4},
              "training": {"num_pixels": 1, "random_seed": 23}}
    params = {"mode": "jamming", "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
              "generator": {"type": "RBM", "num_hidden": HN, "num_hidden_rnn": UNITS, "feedback": None}}
    m = MultINN(config, params, mode="jamming", precision=a.precision)
    assert all(g.k == K for g in m.generators)
    R = np.random.default_rng(23)
    x = torch.from_numpy((R.random((a.n, a.intro, P, M)) < 0.03).astype(np.uint8)).to(dev)
    m.build(x, lengths=None, is_train=False, mode="generate")
    for g in m.generators:
        g._rbm.bv.fill_(math.log(0.03 / 0.97))                      # piano-roll-like visible marginals
        g._packed_step = -1
    given = torch.from_numpy((R.random((a.n, a.steps, P, M)) < 0.05).astype(np.uint8)).to(dev)
    track = torch.zeros(M, dtype=torch.bool)
    track[a.track] = True
    pitch = torch.zeros(P, M, dtype=torch.bool)
    pitch[:a.low] = True
    cases = {"plain": None, "track": track, "pitch": pitch}
    if a.only != "all":
        cases = {a.only: cases[a.only]}

    def timed(mask):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(a.steps) if mask is None else m.generate(a.steps, given=given, given_mask=mask)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for mask in cases.values():
        timed(mask)                                                 # capture
    best = {k: float("inf") for k in cases}
    dens = {}
    for _ in range(a.reps):
        for k, mask in cases.items():
            t, out = timed(mask)
            best[k] = min(best[k], t)
            dens[k] = float(out.float().mean())
    res = {"n": a.n, "intro": a.intro, "steps": a.steps, "tracks": M, "P": P, "Hn": HN, "k": K, "precision": a.precision, "reps": a.reps,
           "given_track": a.track, "given_low_pitches": a.low}
    for k in cases:
        res[k] = {"us_per_step": round(1e6 * best[k] / a.steps, 2), "density": round(dens[k], 4)}
        if k != "plain" and "plain" in cases:
            res[k]["over_plain"] = round(best[k] / best["plain"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
