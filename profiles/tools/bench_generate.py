"""Sampling-scan timing (A10/A11): intro pass + num_steps x {NADE sample, LSTM step, Dense}.
    python profiles/tools/bench_generate.py [n [Ti [steps [reps [max_notes]]]]]
max_notes (optional, a Python literal): generate's polyphony cap -- 4, or "(1, 4, None, 4, 1)" for one entry per track of the 440 visibles."""
import ast, sys, time, json
import numpy as np, torch
sys.path.insert(0, ".")
from multinn_amd import RnnNade

def main(n=72, Ti=32, steps=128, reps=3, max_notes=None):
    dev = "cuda:0"
    R = np.random.default_rng(23)
    x = torch.from_numpy((R.random((n, Ti, 440)) < 0.03).astype(np.uint8)).to(dev)
    g = RnnNade(440, 256, [512, 256], keep_prob=0.9, precision="bf16", seed=23)
    kw = {} if max_notes is None else dict(max_notes=max_notes)
    out = g.generate(x, 4, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = g.generate(x, steps, **kw)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = min(ts)
    print(json.dumps({"n": n, "intro": Ti, "steps": steps, "s": t, "us_per_step": 1e6 * t / steps, "generated_timesteps_per_s": n * steps / t,
                      "density": float(out.float().mean()), **({} if max_notes is None else {"max_notes": max_notes})}))

if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:5]], *[ast.literal_eval(a) for a in sys.argv[5:6]])
