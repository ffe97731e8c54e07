"""The NADE importance estimator at the joint shape: N = B x T rows of one NADE over D = 440 visibles (88 pitches x 5 tracks, ordered p M + m),
Hn = 256, the cells of ONE track of five given (every fifth visible), C particles per row.  One JSON line per leg:
  lower / upper   one ops.nade_given_is launch (scan kernel + reduction) without / with data, best of --reps, timed in alternation with
  route           the only way to the same weights without the kernel: every bias row replicated C times (torch), ops.nade_sample(given=) on
                  the N C rows, ops.nade_logprob_fwd for the conditionals of the sampled vectors, and the weights, their logsumexp, ESS and
                  standard error formed in torch.  `route_sample_only` is the nade_sample launch of that route on its own.
  ratio           route / lower and route / upper (above 1: the new launch is faster).
The two routes draw from different uniforms (the replicated rows have row ids of their own), so their estimates agree statistically, not bit
for bit: `mean_log_pg` of both is printed.  `--only kernel` runs the new launches alone (for a `rocprofv3 --kernel-trace --stats` run)."""
import argparse
import json
import math
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from multinn_amd import ops                          # noqa: E402

P, M, HN = 88, 5, 256
D = P * M


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=72)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["all", "kernel"], default="all")
    a = ap.parse_args()
    dev = "cuda:0"
    N, C = a.B * a.T, a.particles
    R = np.random.default_rng(0)
    t = lambda x: torch.from_numpy(x).to(dev)
    bias = (R.standard_normal((N, HN + D)) * 0.3).astype(np.float32)
    bias[:, HN:] -= 3.0                                                     # piano-roll-like: a few percent of the cells on
    bias, we, wd = t(bias), t((R.standard_normal((1, D, HN)) * 0.05).astype(np.float32)), t((R.standard_normal((1, D, HN)) * 0.05).astype(np.float32))
    x = (R.random((1, N, D)) < 0.05).astype(np.uint8)
    given = np.arange(D) % M == 0                                           # track 0 of five
    codes, x = t(np.where(given[None, None, :], x, 255).astype(np.uint8)), t(x)
    g_dev = torch.from_numpy(given).to(dev)
    log_pg, stats = torch.empty((1, N), device=dev), torch.empty((1, N, 2), device=dev)

    def new(data):
        return ops.nade_given_is(bias, we, wd, 1, D, HN, codes, C, 1, data=data, log_pg=log_pg, stats=stats)

    def route(sample_only=False):
        rep = bias.repeat_interleave(C, dim=0)
        crep = codes[0].repeat_interleave(C, dim=0)
        smp = torch.empty((N * C, D), device=dev, dtype=torch.uint8)
        ops.nade_sample(rep, we, wd, 1, D, HN, 1.0, 1, 0, 0, smp, given=crep)
        if sample_only:
            return smp
        cp = torch.empty((1, N * C, D), device=dev)
        ops.nade_logprob_fwd(smp.view(1, N * C, D), rep, we, wd, 1, D, HN, cond_p=cp)
        q = torch.where(smp > 0, cp[0], 1.0 - cp[0])
        lw = (torch.log(1e-6 + q) * g_dev).sum(1).view(N, C).double()
        m = lw.max(1, keepdim=True).values
        e = torch.exp(lw - m)
        s1, s2 = e.sum(1), (e * e).sum(1)
        ess = s1 * s1 / s2
        return (m[:, 0] + torch.log(s1) - math.log(C)).float(), ess, torch.sqrt((C / ess - 1.0).clamp_min(0) / max(C - 1, 1))

    new(None), new(x)                                                       # warm-up of every timed shape
    if a.only == "all":
        route(), route(True)
    torch.cuda.synchronize()
    best = {"lower": math.inf, "upper": math.inf, "route": math.inf, "route_sample_only": math.inf}
    mean = {}
    for _ in range(a.reps):                                                 # alternating: every leg sees the same neighbours on a shared host
        for leg, fn in (("lower", lambda: new(None)), ("upper", lambda: new(x)), ("route", route), ("route_sample_only", lambda: route(True))):
            if a.only == "kernel" and leg.startswith("route"):
                continue
            s, out = timed(fn)
            best[leg] = min(best[leg], s)
            if leg in ("lower", "upper"):
                mean[leg] = float(out.double().mean())
            elif leg == "route":
                mean[leg] = float(out[0].double().mean())
    scans = N * C
    for leg, s in best.items():
        if math.isfinite(s):
            print(json.dumps({"leg": leg, "rows": N, "particles": C, "D": D, "Hn": HN, "given": int(given.sum()), "s": round(s, 5),
                              "scans_per_s": float(f"{scans / s:.4g}"), "mean_log_pg": None if leg not in mean else round(mean[leg], 4)}), flush=True)
    if a.only == "all":
        print(json.dumps({"leg": "ratio", "route_over_lower": round(best["route"] / best["lower"], 3),
                          "route_over_upper": round(best["route"] / best["upper"], 3),
                          "route_sample_only_over_lower": round(best["route_sample_only"] / best["lower"], 3)}), flush=True)


if __name__ == "__main__":
    main()
