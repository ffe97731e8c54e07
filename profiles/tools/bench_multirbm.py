"""The three measurements of profiles/multirbm.md, all with HIP events on one device in one process:

  1. ops.rbm_gibbs_multi (one grouped launch) against a loop of M ops.rbm_gibbs launches, alternated, at the sampling shape
     (N = 72, D = 88, Hn = 256, k = 10, M = 5) and at the training shape (N = 32 768);
  2. us per generated step of the composer LSTM-RBM scan (RnnMultiRBM.generate, 72 intros) next to the jamming scan's (five RnnRBM.generate);
  3. ms per captured train step of the composer MultiRBM mode at [256, 128, 88, 5], k = 10, next to the jamming RBM mode (C3).

    python profiles/tools/bench_multirbm.py [out.json]
"""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from multinn_amd import ops, MultINN, AdamOptimizer, RnnRBM, RnnMultiRBM   # noqa: E402

DEV = "cuda:0"
TRACKS = ["Drums", "Piano", "Guitar", "Bass", "Strings"]


def timed(fn, reps, inner=1):
    """ms per call of fn: `reps` event-bracketed windows of `inner` calls each -> (median, min, max)."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def gibbs_case(N, D=88, Hn=256, k=10, M=5, reps=15, inner=20):
    R = np.random.default_rng(1)
    W = torch.from_numpy((R.standard_normal((M, D, Hn)) * .1).astype(np.float32)).to(DEV)
    ld = ops.round_up(M * (Hn + D), 64)
    out = torch.from_numpy((R.standard_normal((N, ld)) * .3).astype(np.float32)).to(DEV)
    v0 = torch.from_numpy((R.random((M, N, D)) < .05).astype(np.uint8)).to(DEV)
    p_v = torch.empty((M, N, D), device=DEV)
    v_s = torch.empty((M, N, D), device=DEV, dtype=torch.uint8)
    bh = [out[:, m * Hn:(m + 1) * Hn] for m in range(M)]
    bv = [out[:, M * Hn + m * D:M * Hn + (m + 1) * D] for m in range(M)]
    bh_c, bv_c = [b.contiguous() for b in bh], [b.contiguous() for b in bv]
    jobs = [dict(v0=v0[m], W=W[m], bh=bh[m], bv=bv[m], seed=3 + m, p_v=p_v[m], v_out=v_s[m]) for m in range(M)]

    def grouped():
        ops.rbm_gibbs_multi(jobs, k, 0, None, 0)

    def loop():
        for m in range(M):
            ops.rbm_gibbs(v0[m], W[m], bh_c[m], bv_c[m], k, 3 + m, 0, None, 0, p_v[m], v_s[m])

    grouped(); ref = v_s.clone(); loop()
    assert torch.equal(ref, v_s), "grouped and single launches must agree"
    res = {}
    for rnd in range(3):                      # alternated: three rounds of each, the spread is between rounds of the same code
        for name, fn in (("grouped", grouped), ("loop", loop)):
            fn(); torch.cuda.synchronize()
            res.setdefault(name, []).append(timed(fn, reps, inner)[0])
    return {"N": N, "D": D, "Hn": Hn, "k": k, "M": M,
            "grouped_ms": res["grouped"], "loop_ms": res["loop"],
            "grouped_median_ms": float(np.median(res["grouped"])), "loop_median_ms": float(np.median(res["loop"]))}


def generate_case(n=72, Ti=8, steps=64, P=88, M=5, reps=5):
    R = np.random.default_rng(23)
    x = torch.from_numpy((R.random((n, Ti, P, M)) < 0.03).astype(np.uint8)).to(DEV)
    comp = RnnMultiRBM(P, 256, [512, 256], tracks=TRACKS, k=10, precision="fp16", seed=23)
    jam = [RnnRBM(P, 256, [512, 256], k=10, precision="fp16", seed=23 + m) for m in range(M)]
    xs = x.reshape(n, Ti, P * M)
    xm = [x[..., m].contiguous() for m in range(M)]
    f_comp = lambda: comp.generate(xs, steps)
    f_jam = lambda: [g.generate(xm[m], steps) for m, g in enumerate(jam)]
    out = {}
    for rnd in range(2):
        for name, fn in (("composer_multirbm", f_comp), ("jamming_rbm", f_jam)):
            fn(); torch.cuda.synchronize()
            out.setdefault(name, []).append(1e3 * timed(fn, reps)[0] / steps)
    return {"intros": n, "steps": steps, "us_per_step": {k_: float(np.median(v)) for k_, v in out.items()}, "rounds": out}


def cfg(P):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 0, "highest": P}, "instruments": TRACKS, "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def prm(mode, gen):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
            "generator": {"type": gen, "num_hidden": 256, "num_hidden_rnn": [512, 256], "feedback": None}}


def train_case(B=256, T=128, P=88, M=5, reps=10):
    x = torch.from_numpy((np.random.default_rng(5).random((B, T, P, M)) < 0.03).astype(np.uint8)).to(DEV)
    runs = {}
    for name, mode, gen in (("composer_multirbm", "composer", "MultiRBM"), ("jamming_rbm_c3", "jamming", "RBM")):
        m = MultINN(cfg(P), prm(mode, gen), mode=mode, precision="fp16")
        runs[name] = (m, m.graphed_train_step(x, AdamOptimizer(0.01), 0.01, warmup=2))
    out = {}
    for rnd in range(2):
        for name, (m, run) in runs.items():
            run(); torch.cuda.synchronize()
            out.setdefault(name, []).append(timed(run, reps)[0])
    for m, _ in runs.values():
        m.check(tolerate_overflow=True)
    return {"shape": [B, T, P, M], "k": 10, "ms_per_step": {k_: float(np.median(v)) for k_, v in out.items()}, "rounds": out}


def main():
    assert torch.cuda.is_available(), "this measurement needs a ROCm device"
    res = {"gibbs_sampling_shape": gibbs_case(72), "gibbs_training_shape": gibbs_case(32768, reps=7, inner=3),
           "generate": generate_case(), "train_step": train_case()}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text)


if __name__ == "__main__":
    main()
