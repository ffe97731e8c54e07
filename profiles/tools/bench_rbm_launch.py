"""The chain timings of profiles/rbm_launch.md for ONE library, with HIP events: sections 1 of bench_multirbm.py (a grouped launch against a
loop of single launches at N = 72 and N = 32 768) and a single ops.rbm_gibbs at N = 72, k = 10.  Two libraries are compared by running this
once per library and round, alternated, each in a process of its own (MULTINN_HIP_LIB selects the library):

    MULTINN_HIP_LIB=/path/to/libmultinn_hip.so python profiles/tools/bench_rbm_launch.py out.json
"""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "profiles/tools")
from bench_multirbm import DEV, gibbs_case, timed   # noqa: E402
from multinn_amd import ops   # noqa: E402


def single_case(N=72, D=88, Hn=256, k=10, reps=15, inner=20):
    R = np.random.default_rng(2)
    W = torch.from_numpy((R.standard_normal((D, Hn)) * .1).astype(np.float32)).to(DEV)
    bh = torch.from_numpy((R.standard_normal((N, Hn)) * .3).astype(np.float32)).to(DEV)
    bv = torch.from_numpy((R.standard_normal((N, D)) * .3).astype(np.float32)).to(DEV)
    v0 = torch.from_numpy((R.random((N, D)) < .05).astype(np.uint8)).to(DEV)
    p_v, v_s = torch.empty((N, D), device=DEV), torch.empty((N, D), device=DEV, dtype=torch.uint8)
    fn = lambda: ops.rbm_gibbs(v0, W, bh, bv, k, 3, 0, None, 0, p_v, v_s)
    fn(); torch.cuda.synchronize()
    return {"N": N, "k": k, "ms": [timed(fn, reps, inner)[0] for _ in range(3)]}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs a ROCm device"
    res = {"sampling": gibbs_case(72), "training": gibbs_case(32768, reps=7, inner=3), "single": single_case()}
    text = json.dumps(res)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text)
