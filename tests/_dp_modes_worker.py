"""Worker of tests/test_gpu_dp_modes.py: one data-parallel rank of the MODE classes' train step (run under torch.distributed.run, gloo, every
rank on the one GPU), and the model / batch / trajectory helpers the test shares with it.

    _dp_modes_worker.py eager OUT      every case x precision: 3 eager steps on this rank's half of the batch
    _dp_modes_worker.py captured OUT   the capturable cases: 1 eager step, graphed_train_step(warmup=0), 3 replays
    _dp_modes_worker.py rehearsal OUT  world size 1 with MULTINN_DP_REHEARSAL=1: driver.train_epoch on the jamming model, and the ragged refusals
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
B, T, P, M = 8, 6, 8, 2
TRACKS = ["Drums", "Piano"]
CASES = {"joint-nade": ("joint", "NADE"), "jamming-nade": ("jamming", "NADE"), "jamming-rbm": ("jamming", "RBM"),
         "composer-multinade": ("composer", "NADE"), "feedback-nade": ("feedback", "NADE")}
CAPTURED = ["joint-nade", "jamming-nade", "jamming-rbm", "composer-multinade"]
PRECISIONS = ["fp32", "bf16"]
EAGER_STEPS, REPLAYS = 3, 3
SONGS, WINDOWS, EPOCH_BATCH = 6, 3, 2


def batch():
    return (np.random.default_rng(3).random((B, T, P, M)) < 0.25).astype(np.uint8)


def songs():
    return (np.random.default_rng(8).random((SONGS, WINDOWS * T, P, M)) < 0.2).astype(np.uint8)


def make_model(case, precision):
    from multinn_amd import MultINN, AdamOptimizer
    mode, gen = CASES[case]
    config = {"model_name": "t", "data": {"pitch_range": {"lowest": 0, "highest": P}, "instruments": list(TRACKS), "beat_resolution": 4},
              "training": {"num_pixels": 1, "random_seed": 23}}
    params = {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
              "generator": {"type": gen, "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": [24] if mode == "feedback" else None}}
    m = MultINN(config, params, mode=mode, precision=precision, seed=23)
    if gen == "RBM":
        for g in m.generators:
            g._k = 2                                   # CD-2
    return m, AdamOptimizer(0.01)


def snapshot(m):
    stores = m._all_stores()
    return dict(theta=[st.theta.cpu() for st in stores], step=[st.step for st in stores], step_dev=[int(st.step_dev) for st in stores])


def full_batch_trajectory(case, precision, steps):
    """The single-process eager steps on the whole batch: losses, and a snapshot after every step."""
    m, opt = make_model(case, precision)
    x = torch.from_numpy(batch()).to(DEV)
    losses, snaps = [], []
    for _ in range(steps):
        losses.append(float(m.train_step(x, None, opt)))
        snaps.append(snapshot(m))
    m.check()
    return losses, snaps


class Counted:
    """training.allreduce_flat behind a call counter."""

    def __init__(self):
        from multinn_amd import training
        self.calls, self._training, self._orig = 0, training, training.allreduce_flat
        training.allreduce_flat = self

    def __call__(self, grad):
        self.calls += 1
        return self._orig(grad)


def global_loss(loss):
    import torch.distributed as dist
    lt = loss.detach().clone().reshape(1).float()
    dist.all_reduce(lt)                                 # the logged loss: sum of the ranks' weighted partial sums
    return float(lt)


def run_eager(rank, world, counter):
    per = B // world
    x = torch.from_numpy(batch()[rank * per:(rank + 1) * per]).to(DEV)
    out = {}
    for case in CASES:
        for precision in PRECISIONS:
            m, opt = make_model(case, precision)
            m.row0 = rank * per
            losses, calls = [], []
            for _ in range(EAGER_STEPS):
                c0 = counter.calls
                loss = m.train_step(x, None, opt)
                calls.append(counter.calls - c0)
                losses.append(global_loss(loss))
            m.check()
            out[(case, precision)] = dict(losses=losses, calls=calls, stores=len(m._all_stores()), **snapshot(m))
    return out


def run_captured(rank, world, counter):
    per = B // world
    x = torch.from_numpy(batch()[rank * per:(rank + 1) * per]).to(DEV)
    out = {}
    for case in CAPTURED:
        for precision in PRECISIONS:
            m, opt = make_model(case, precision)
            m.row0 = rank * per
            losses, calls = [global_loss(m.train_step(x, None, opt))], []
            run = m.graphed_train_step(x, opt, None, warmup=0)
            for _ in range(REPLAYS):
                c0 = counter.calls
                loss = run(x)
                calls.append(counter.calls - c0)
                losses.append(global_loss(loss))
            m.check()
            out[(case, precision)] = dict(losses=losses, calls=calls, two_graphs=run.opt_graph is not None, ragged=run.ragged, **snapshot(m))
    return out


def run_rehearsal(counter):
    from multinn_amd.driver import train_epoch, LossAccumulator, TrainingStats
    from multinn_amd.training import dp_active
    assert dp_active()
    X = songs()
    lengths, ids = np.full(SONGS, WINDOWS * T), np.arange(SONGS)
    out = {}
    for graph in (True, False):
        os.environ["MULTINN_TRAIN_GRAPH"] = "1" if graph else "0"
        m, opt = make_model("jamming-nade", "bf16")
        acc, c0 = LossAccumulator(), counter.calls
        train_epoch(m, X, lengths, ids, EPOCH_BATCH, T, opt, acc, TrainingStats(), lr=0.01, device=DEV)
        m.check()
        graphs = m.__dict__.get("_step_graphs", {})
        out["graph" if graph else "eager"] = dict(loss=acc.loss(), calls=counter.calls - c0, keys=[k[-1] for k in graphs],
                                                  two_graphs=[r.opt_graph is not None for r in graphs.values()], **snapshot(m))
    os.environ["MULTINN_TRAIN_GRAPH"] = "1"
    # ragged windows stay eager under data parallelism
    m, opt = make_model("jamming-nade", "bf16")
    x = torch.from_numpy(batch()).to(DEV)
    lens = torch.tensor([6, 3, 5, 6, 2, 6, 4, 1], dtype=torch.int32, device=DEV)
    m.train_step(x, lens, opt)
    shape = tuple(x.shape)
    out["capturable_full"], out["capturable_ragged"] = m.capturable(shape, False), m.capturable(shape, True)
    try:
        m.graphed_train_step(x, opt, None, warmup=0, lengths=lens)
        out["ragged_refusal"] = None
    except NotImplementedError as e:
        out["ragged_refusal"] = str(e)
    # the feedback modes' captured step is refused under data parallelism (their eager step is what the two-rank test checks)
    m, opt = make_model("feedback-nade", "bf16")
    m.train_step(x, None, opt)
    try:
        m.graphed_train_step(x, opt, None, warmup=0)
        out["feedback_refusal"] = None
    except NotImplementedError as e:
        out["feedback_refusal"] = str(e)
    return out


def main():
    import torch.distributed as dist
    kind, out_path = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)                            # every rank on the one GPU of the box: gloo moves the gradient
    dist.init_process_group("gloo")
    counter = Counted()
    if kind == "eager":
        out = run_eager(rank, world, counter)
    elif kind == "captured":
        out = run_captured(rank, world, counter)
    else:
        out = run_rehearsal(counter)
    if rank == 0:
        torch.save(out, out_path)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
