"""Clamped AIS beside AIS at the C3 widths (D 88, Hn 256: the matrix-core form): one launch each of mnn_rbm_ais, mnn_rbm_raise and -- where
the library has them -- mnn_rbm_ais_given / mnn_rbm_raise_given on the same N random bias rows, ladder and chains, alternated in one
process over --reps rounds, best time of each; one JSON line per leg.  Clamped legs: every code free (the GIVEN kernels with nothing to
clamp), half of the cells clamped at random, and every fifth cell clamped (one track of five in the joint order p M + m).
The library is loaded with ctypes from --lib (default: the package's), so the parent commit's build -- which lacks the two new symbols --
runs the free legs through the same script: `--lib scratch/lib_parent.so`."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
P, HN = 88, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(HERE, "..", "..", "multinn_amd", "libmultinn_hip.so"))
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--betas", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    lib = C.CDLL(os.path.abspath(a.lib))
    lib.mnn_rbm_ais_workspace_bytes.restype = C.c_size_t
    dev = "cuda:0"
    N, S, L = a.rows, a.chains, a.betas
    R = np.random.default_rng(0)
    t_ = lambda x: torch.from_numpy(x).to(dev)
    W = t_((R.standard_normal((P, HN)) * 0.05).astype(np.float32))
    bh = t_((R.standard_normal((N, HN)) * 0.3).astype(np.float32))
    bv = t_((R.standard_normal((N, P)) * 0.3 - 3.0).astype(np.float32))
    v = t_((R.random((N, P)) < 0.05).astype(np.uint8))
    betas = (torch.arange(L, dtype=torch.float64) / (L - 1)).float().to(dev)
    vals = (R.random((N, P)) < 0.05).astype(np.uint8)
    codes = {"all_free": np.full((N, P), 255, np.uint8), "half": np.where(R.random((N, P)) < 0.5, vals, 255).astype(np.uint8),
             "one_track_of_five": np.where((np.arange(P) % 5 == 0)[None, :], vals, 255).astype(np.uint8)}
    codes = {k: t_(c) for k, c in codes.items()}
    log_z = torch.empty(N, device=dev)
    ws = torch.empty(lib.mnn_rbm_ais_workspace_bytes(N, P, HN, S, L), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (st, N, P, HN, S, L, p(betas), p(W), p(bh), HN, p(bv), P)
    tail = (C.c_uint64(1), C.c_uint32(0), None, p(log_z), None, None, None, p(ws))
    legs = {"ais": lambda: lib.mnn_rbm_ais(*head, *tail), "raise": lambda: lib.mnn_rbm_raise(*head, p(v), *tail)}
    if hasattr(lib, "mnn_rbm_ais_given"):
        for k, c in codes.items():
            legs["ais_given/" + k] = lambda c=c: lib.mnn_rbm_ais_given(*head, *tail, p(c), P)
            legs["raise_given/" + k] = lambda c=c: lib.mnn_rbm_raise_given(*head, p(v), *tail, p(c), P)
    best = {k: float("inf") for k in legs}
    for k, f in legs.items():                                            # warm-up
        assert f() == 0, k
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert f() == 0, k
            e1.record()
            torch.cuda.synchronize()
            best[k] = min(best[k], e0.elapsed_time(e1) / 1e3)
    for k, t in best.items():
        print(json.dumps({"lib": os.path.basename(a.lib), "leg": k, "rows": N, "chains": S, "betas": L, "D": P, "Hn": HN, "s": round(t, 4),
                          "ratio_to_free": round(t / best[k.split("_given")[0]], 4)}), flush=True)


if __name__ == "__main__":
    main()
