"""Eager vs captured (two-graph) wall time per step of the jamming model (bench.py's C3: 5 x LSTM-RBM CD-10) at [256,128,88,5] PER RANK, over
gloo ranks that share one GPU -- profiles/dp_modes.md.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 profiles/tools/bench_dp_modes.py
    MULTINN_DP_REHEARSAL=1 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 profiles/tools/bench_dp_modes.py

gloo moves the gradient through the host: this shows the host-bound eager step against the replay, not xGMI scaling.

CAUTION, the 2-rank form: both ranks' persistent recurrences share the one device, and a replay can stall for SECONDS (one of 20 took
10.7 s when this was recorded; cause only supposed, profiles/dp_modes.md section 2).  Run it under an outer time limit
(`timeout -k 10 300 ...`), once; do not loop it or repeat it to reproduce the stall on a GPU that others share."""
import json
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    import bench
    from multinn_amd import MultINN, AdamOptimizer
    w = bench.WORKLOADS["c3"]
    B, T, P, M = w["B"], w["T"], w["P"], w["M"]
    config, params = bench.mode_params(w)
    model = MultINN(config, params, mode="jamming", precision="fp16", seed=23, device="cuda:0")
    model.row0 = rank * B
    x = torch.from_numpy(bench.synth(B, T, P, M, 23 + rank, 0.03)).to("cuda:0")
    opt = AdamOptimizer(0.01)

    def timed(fn, n):
        out = []
        for _ in range(n):
            dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    for _ in range(3):
        model.train_step(x, None, opt)
    eager = timed(lambda: model.train_step(x, None, opt), 20)
    run = model.graphed_train_step(x, opt, None, warmup=0)
    for _ in range(3):
        run(x)
    captured = timed(lambda: run(x), 20)
    model.check(tolerate_overflow=True)
    if rank == 0:
        q = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
        print(json.dumps({"what": "jamming c3, %d gloo rank(s) on one GPU, ms per step (rank 0 wall, barrier before each step)" % world, "eager": q(eager),
                          "captured": q(captured), "two_graphs": run.opt_graph is not None, "grad_words": int(model._grad_arena.flat.numel())}))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
