"""NADE importance resampling at the joint shape: B rows of one NADE over D = 440 visibles (88 pitches x 5 tracks, ordered p M + m), Hn = 256,
the cells of ONE track of five given (every fifth visible), C particles per scan.  One JSON line per leg:
  sir       one ops.nade_sample_sir step (the scan kernel + the pick launch), best of --reps, timed in alternation with
  plain     the step of the call without particles: ops.nade_sample(given=) on the B rows
  route     the same resampling built from the ops the project had before: every bias row replicated C times (torch), ops.nade_sample(given=)
            on the B C rows, ops.nade_logprob_fwd for the conditionals of the sampled vectors, and the weights, the pick (cumulative sum
            against one uniform per row) and the gather of the picked vectors in torch.
  ratio     route / sir and sir / plain.
  generate  (--generate) RnnNade.generate of --steps steps with the given track, with and without particles, per generated step: one replay
            of the captured scan, best of --reps.
The route draws from other uniforms (the replicated rows have row ids of their own): the legs agree statistically, `mean_on` (the mean of
the emitted free cells) is printed for both."""
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
    ap.add_argument("--particles", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generate", action="store_true")
    ap.add_argument("--steps", type=int, default=32)
    a = ap.parse_args()
    dev = "cuda:0"
    N = a.B
    R = np.random.default_rng(0)
    t = lambda x: torch.from_numpy(x).to(dev)
    bias = (R.standard_normal((N, HN + D)) * 0.3).astype(np.float32)
    bias[:, HN:] -= 3.0                                                     # piano-roll-like: a few percent of the cells on
    bias, we, wd = t(bias), t((R.standard_normal((1, D, HN)) * 0.05).astype(np.float32)), t((R.standard_normal((1, D, HN)) * 0.05).astype(np.float32))
    x = (R.random((N, D)) < 0.05).astype(np.uint8)
    given = np.arange(D) % M == 0                                           # track 0 of five
    codes = t(np.where(given[None, :], x, 255).astype(np.uint8))
    g_dev = torch.from_numpy(given).to(dev)
    out = torch.empty((N, D), device=dev, dtype=torch.uint8)
    ess, pick = torch.empty((1, N), device=dev), torch.empty((1, N), device=dev, dtype=torch.int32)

    def plain():
        ops.nade_sample(bias, we, wd, 1, D, HN, 1.0, 1, 0, 0, out, given=codes)
        return out

    for C in a.particles:
        def sir():
            ops.nade_sample_sir(bias, we, wd, 1, D, HN, 1.0, 1, 0, 0, out, codes, C, ess=ess, pick=pick)
            return out

        def route():
            rep = bias.repeat_interleave(C, dim=0)
            crep = codes.repeat_interleave(C, dim=0)
            smp = torch.empty((N * C, D), device=dev, dtype=torch.uint8)
            ops.nade_sample(rep, we, wd, 1, D, HN, 1.0, 1, 0, 0, smp, given=crep)
            cp = torch.empty((1, N * C, D), device=dev)
            ops.nade_logprob_fwd(smp.view(1, N * C, D), rep, we, wd, 1, D, HN, cond_p=cp)
            q = torch.where(smp > 0, cp[0], 1.0 - cp[0])
            lw = (torch.log(1e-6 + q) * g_dev).sum(1).view(N, C).double()
            run = torch.exp(lw - lw.max(1, keepdim=True).values).cumsum(1)
            u = torch.rand((N, 1), device=dev, dtype=torch.float64)
            p = (run <= u * run[:, -1:]).sum(1).clamp_max(C - 1)
            return smp.view(N, C, D)[torch.arange(N, device=dev), p]

        sir(), plain(), route()                                             # warm-up of every timed shape
        torch.cuda.synchronize()
        best = {"sir": math.inf, "plain": math.inf, "route": math.inf}
        mean = {}
        for _ in range(a.reps):                                             # alternating: every leg sees the same neighbours on a shared host
            for leg, fn in (("sir", sir), ("plain", plain), ("route", route)):
                s, o = timed(fn)
                best[leg] = min(best[leg], s)
                mean[leg] = float(o[:, ~g_dev].double().mean())
        for leg, s in best.items():
            print(json.dumps({"leg": leg, "rows": N, "particles": C, "D": D, "Hn": HN, "given": int(given.sum()), "us": round(s * 1e6, 1),
                              "mean_on": round(mean[leg], 5)}), flush=True)
        print(json.dumps({"leg": "ratio", "particles": C, "route_over_sir": round(best["route"] / best["sir"], 3),
                          "sir_over_plain": round(best["sir"] / best["plain"], 3), "mean_ess": round(float(ess.mean()), 2)}), flush=True)

    if a.generate:
        from multinn_amd import RnnNade
        gen = RnnNade(D, HN, [512, 512], precision="bf16", seed=5)
        gen._materialize(D)
        intro = t((R.random((N, 8, D)) < 0.05).astype(np.uint8))
        block = (R.random((N, a.steps, D)) < 0.05).astype(np.uint8)
        gcodes = t(np.where(given[None, None, :], block, 255).astype(np.uint8))
        legs = [("generate_plain", {})] + [(f"generate_particles_{C}", dict(particles=C)) for C in a.particles]
        for _, kw in legs:
            gen.generate(intro, a.steps, given=gcodes, **kw)                 # capture
        torch.cuda.synchronize()
        best = {leg: math.inf for leg, _ in legs}
        for _ in range(a.reps):
            for leg, kw in legs:
                s, _ = timed(lambda: gen.generate(intro, a.steps, given=gcodes, **kw))
                best[leg] = min(best[leg], s)
        for leg, s in best.items():
            print(json.dumps({"leg": leg, "rows": N, "steps": a.steps, "us_per_step": round(s * 1e6 / a.steps, 1)}), flush=True)


if __name__ == "__main__":
    main()
