"""AIS log-likelihood estimation at the C3 widths: 5 tracks of RnnRBM(88 visibles, 256 hidden, LSTM [512, 256]) in jamming mode,
B x T = N rows per track, S chains, L ladder values.  Two measurements, one JSON line each:
  model   MultINN.estimate_nll on a [B, T, 88, 5] batch (eval build of the five generators + five AIS launches), best of --reps;
  kernel  one ops.rbm_ais launch on N random bias rows at (88, 256): time, chain-steps per second (N S (L - 1)) and the fraction of the
          f32 matrix-core rate, counting 4 D Hn FLOP per chain-step against --peak TFLOP/s (155: the measured v_mfma_f32_32x32x2_f32 rate).
  reverse one ops.rbm_raise launch (reverse AIS from random data rows) on the same rows, ladder and chains, timed in the same process in
          alternation with the forward launch (--reps rounds of forward, reverse), and the ratio of the two best times.  The reverse run has
          L hidden and L - 1 visible contractions against L - 1 and L - 2: parity is the expectation.
`--only kernel` runs the kernel legs alone (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from multinn_amd import MultINN, ops                 # noqa: E402

P, M, HN, UNITS = 88, 5, 256, [512, 256]
TRACKS = ["Drums", "Piano", "Guitar", "Bass", "Strings"]


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 1e3)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--betas", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--peak", type=float, default=155.0)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--only", choices=["all", "model", "kernel"], default="all")
    a = ap.parse_args()
    dev = "cuda:0"
    N, S, L = a.B * a.T, a.chains, a.betas
    R = np.random.default_rng(0)
    if a.only in ("all", "model"):
        config = {"model_name": "bench", "data": {"pitch_range": {"lowest": 0, "highest": P}, "instruments": TRACKS, "beat_resolution": 4},
                  "training": {"num_pixels": 1, "random_seed": 23}}
        params = {"mode": "jamming", "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
                  "generator": {"type": "RBM", "num_hidden": HN, "num_hidden_rnn": UNITS, "feedback": None}}
        m = MultINN(config, params, mode="jamming", precision=a.precision)
        x = torch.from_numpy((R.random((a.B, a.T, P, M)) < 0.05).astype(np.uint8)).to(dev)
        m.estimate_nll(x, num_chains=S, num_betas=L)                   # warm-up (materialise, pack)
        t, est = timed(lambda: m.estimate_nll(x, num_chains=S, num_betas=L), a.reps)
        print(json.dumps({"leg": "model", "tracks": M, "rows_per_track": N, "chains": S, "betas": L, "s": round(t, 4),
                          "s_per_track": round(t / M, 4), "mean_nll": round(est.mean, 3), "stderr": round(est.stderr, 4),
                          "min_ess": round(est.ess, 2)}), flush=True)
    if a.only in ("all", "kernel"):
        W = torch.from_numpy((R.standard_normal((P, HN)) * 0.05).astype(np.float32)).to(dev)
        bh = torch.from_numpy((R.standard_normal((N, HN)) * 0.3).astype(np.float32)).to(dev)
        bv = torch.from_numpy((R.standard_normal((N, P)) * 0.3 - 3.0).astype(np.float32)).to(dev)
        betas = (torch.arange(L, dtype=torch.float64) / (L - 1)).float().to(dev)
        log_z = torch.empty(N, device=dev)
        v = torch.from_numpy((R.random((N, P)) < 0.05).astype(np.uint8)).to(dev)
        ops.rbm_ais(W, bh, bv, betas, S, 1, log_z=log_z)                # warm-up
        ops.rbm_raise(W, bh, bv, v, betas, S, 1, log_z=log_z)
        torch.cuda.synchronize()
        t = t_rev = float("inf")
        for _ in range(a.reps):                                         # alternating: both legs see the same neighbours on a shared host
            t = min(t, timed(lambda: ops.rbm_ais(W, bh, bv, betas, S, 1, log_z=log_z), 1)[0])
            t_rev = min(t_rev, timed(lambda: ops.rbm_raise(W, bh, bv, v, betas, S, 1, log_z=log_z), 1)[0])
        steps = N * S * (L - 1)
        flop = 4.0 * P * HN * steps
        print(json.dumps({"leg": "kernel", "rows": N, "chains": S, "betas": L, "D": P, "Hn": HN, "s": round(t, 4),
                          "chain_steps_per_s": float(f"{steps / t:.4g}"), "tflops": round(flop / t / 1e12, 2),
                          "fraction_of_f32_matrix_peak": round(flop / t / 1e12 / a.peak, 3)}), flush=True)
        print(json.dumps({"leg": "reverse", "rows": N, "chains": S, "betas": L, "D": P, "Hn": HN, "s": round(t_rev, 4),
                          "chain_steps_per_s": float(f"{N * S * L / t_rev:.4g}"), "ratio_to_forward": round(t_rev / t, 4)}), flush=True)


if __name__ == "__main__":
    main()
