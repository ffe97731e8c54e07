"""The cap by rejection (`redraws=`): timings and acceptance counts (profiles/redraws.md).
    python profiles/tools/bench_redraws.py generate joint|multi REDRAWS [reps]
        72 intros of 32 steps, generate(128) of the captured scan under max_notes = (1, None, 4, 4, 4): the joint LSTM-NADE over 440 visibles
        (caps by visible index) or the LSTM-MultiNADE of 5 x 88.  The Dense bias of the b_dec blocks is set to logit(13 / 440): about 13 ones
        per step, a piano-roll's density (the untrained model's 219 would send every row to the fallback).  REDRAWS = 0 passes no argument:
        the line also runs on a tree without the feature.
    python profiles/tools/bench_redraws.py restart G REDRAWS [reps]
        the sample launch alone (72 rows G = 16, or 300 rows G = 8; 440 visibles, Hn 256) on a row that violates at visible 0 on every
        attempt (cap 0 on its counter, p = 1 - 5e-5): REDRAWS restarts, each a ring drain, a re-prime and chunk 0's first pass, in front of
        the truncating scan.  (time(REDRAWS) - time(0)) / REDRAWS is the cost of one restart."""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
CAPS = (1, None, 4, 4, 4)


def generate(kind, redraws, reps=8):
    from multinn_amd import RnnNade, RnnMultiNADE
    dev, n, Ti, steps = "cuda:0", 72, 32, 128
    R = np.random.default_rng(23)
    x = torch.from_numpy((R.random((n, Ti, 440)) < 0.03).astype(np.uint8)).to(dev)
    if kind == "joint":
        g, tracks, Hn = RnnNade(440, 256, [512, 256], keep_prob=0.9, precision="bf16", seed=23), 1, 256
    else:
        g, tracks, Hn = RnnMultiNADE(88, 256, [512, 256], tracks=list("abcde"), keep_prob=0.9, precision="bf16", seed=23), 5, 256
    g._materialize(440)
    g.store["dense/bias"][tracks * Hn:] = float(np.log(13 / 427))
    g._packed_step = -1
    kw = dict(max_notes=CAPS, **({"redraws": redraws} if redraws else {}))
    out = g.generate(x, 4, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = g.generate(x, steps, **kw)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = min(ts)
    counts = g.redraw_counts() if redraws else (0, 0)
    print(json.dumps({"kind": kind, "redraws": redraws, "us_per_step": 1e6 * t / steps, "all_us_per_step": [round(1e6 * v / steps, 2) for v in ts],
                      "ones_per_step": float(out.float().sum(2).mean()), "scans": n * steps * tracks, "redrawn": counts[0], "fallback": counts[1]}))


def restart(G, redraws, reps=200):
    from multinn_amd import ops
    dev, D, Hn = "cuda:0", 440, 256
    N = 72 if G == 16 else 300
    g = torch.Generator(device=dev).manual_seed(1)
    bias = torch.zeros((N, Hn + D), device=dev)
    bias[:, Hn:] = float(np.log(13 / 427))
    bias[:, Hn] = 10.0                                              # visible 0: a 1 on every attempt, past its cap of 0
    we = torch.randn((1, D, Hn), device=dev, generator=g) * 0.02
    wd = torch.randn((1, D, Hn), device=dev, generator=g) * 0.02
    out = torch.zeros((N, D), device=dev, dtype=torch.uint8)
    stats = torch.zeros(2, device=dev, dtype=torch.int32)
    kw = dict(by_visible=True, max_notes=(0, None, None, None, None), **({"redraws": redraws, "redraw_stats": stats} if redraws else {}))
    run = lambda: ops.nade_sample(bias, we, wd, 1, D, Hn, 1.0, 5, 0, 0, out, **kw)
    for _ in range(10):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        best.append(1e3 * e0.elapsed_time(e1) / reps)
    print(json.dumps({"G": G, "rows": N, "redraws": redraws, "us_per_launch": min(best), "all": [round(b, 2) for b in best],
                      "fallback_per_launch": int(stats[1]) / (reps * 5 + 10) if redraws else 0}))


if __name__ == "__main__":
    if sys.argv[1] == "generate":
        generate(sys.argv[2], int(sys.argv[3]), *[int(a) for a in sys.argv[4:5]])
    else:
        restart(int(sys.argv[2]), int(sys.argv[3]), *[int(a) for a in sys.argv[4:5]])
