"""The data-parallel train step of the MODE classes (joint, jamming, composer, feedback) with world size 2 on the one GPU of the box -- two
processes, each a rank with half of the batch and `model.row0` set, the gradients of ALL the mode's stores exchanged by ONE
`training.allreduce_flat` per step (gloo here; the call site is the product's) -- against the single-process step on the whole batch:
eagerly, and as replays of the two-graph captured step (forward + backward + arena pack | all-reduce | unpack + clip + Adam).  Then the
driver's epoch on one rehearsal rank (MULTINN_DP_REHEARSAL=1), and the ragged windows that stay eager there.

One worker launch per kind (tests/_dp_modes_worker.py loops over the cases), shared by the cases' tests; bounds: tests/test_gpu_dp.py's for
the single generator, and for bf16 replays test_two_graph_data_parallel_step_matches_eager's."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _dp_modes_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_RTOL = {"fp32": 2e-5, "bf16": 2e-2}               # two ranks against the full batch, eager (test_gpu_dp.py)
THETA_ATOL = {"fp32": 2e-4, "bf16": 4e-3}
CAPTURED_LOSS_RTOL = {"fp32": 2e-5, "bf16": 2e-3}      # bf16: captured against eager (test_two_graph_data_parallel_step_matches_eager)
CAPTURED_THETA_ATOL = {"fp32": 2e-4, "bf16": 3e-3}


def launch(world, kind, out, extra_env=None):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(extra_env or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_dp_modes_worker.py"), kind, out]
    # (two ranks replaying persistent kernels on ONE device: at large shapes such a replay was seen to stall for seconds,
    # profiles/dp_modes.md section 2 -- if this ever times out, look there first)
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def eager(tmp_path_factory):
    return launch(2, "eager", str(tmp_path_factory.mktemp("dp_modes") / "eager.pt"), {"MULTINN_TRAIN_GRAPH": "0"})


@pytest.fixture(scope="module")
def captured(tmp_path_factory):
    return launch(2, "captured", str(tmp_path_factory.mktemp("dp_modes") / "captured.pt"))


@pytest.fixture(scope="module")
def rehearsal(tmp_path_factory):
    return launch(1, "rehearsal", str(tmp_path_factory.mktemp("dp_modes") / "rehearsal.pt"), {"MULTINN_DP_REHEARSAL": "1"})


@functools.lru_cache(maxsize=None)
def reference(case, precision):
    """The single-process trajectory on the whole batch, computed once per case: the eager test reads its first 3 steps, the captured one all 4."""
    return W.full_batch_trajectory(case, precision, 1 + W.REPLAYS)


def max_delta(got, want):
    return [float((a - b).abs().max()) for a, b in zip(got, want)]


@pytest.mark.parametrize("precision", W.PRECISIONS)
@pytest.mark.parametrize("case", list(W.CASES))
def test_two_ranks_equal_the_full_batch_step(case, precision, eager):
    got = eager[(case, precision)]
    losses, snaps = reference(case, precision)
    want = snaps[W.EAGER_STEPS - 1]
    deltas = max_delta(got["theta"], want["theta"])
    print(case, precision, "losses", got["losses"], losses[:W.EAGER_STEPS], "max |d theta| per store", deltas, "all-reduces per step", got["calls"])
    assert got["stores"] == len(want["theta"]) == (W.M + 1 if case.startswith("feedback") else W.M if case.startswith("jamming") else 1)
    assert got["calls"] == [1] * W.EAGER_STEPS                      # ONE exchange per step, however many stores
    assert np.allclose(got["losses"], losses[:W.EAGER_STEPS], rtol=LOSS_RTOL[precision]), (got["losses"], losses)
    assert max(deltas) < THETA_ATOL[precision], deltas
    assert got["step"] == got["step_dev"] == [W.EAGER_STEPS] * got["stores"]


@pytest.mark.parametrize("precision", W.PRECISIONS)
@pytest.mark.parametrize("case", W.CAPTURED)
def test_two_ranks_captured_step_follows_the_eager_trajectory(case, precision, captured):
    got = captured[(case, precision)]
    losses, snaps = reference(case, precision)
    deltas = max_delta(got["theta"], snaps[-1]["theta"])
    print(case, precision, "losses", got["losses"], losses, "max |d theta| per store", deltas, "all-reduces per replay", got["calls"])
    assert got["two_graphs"] and not got["ragged"]
    assert got["calls"] == [1] * W.REPLAYS
    assert np.allclose(got["losses"], losses, rtol=CAPTURED_LOSS_RTOL[precision]), (got["losses"], losses)
    assert max(deltas) < CAPTURED_THETA_ATOL[precision], deltas
    assert got["step"] == got["step_dev"] == [1 + W.REPLAYS] * len(got["theta"])


def test_driver_epoch_replays_the_two_graph_step(rehearsal):
    g, e = rehearsal["graph"], rehearsal["eager"]
    steps = (W.SONGS // W.EPOCH_BATCH) * W.WINDOWS
    print("epoch loss captured", g["loss"], "eager", e["loss"], "graphs", g["keys"], "all-reduces", g["calls"], e["calls"])
    assert g["keys"] == ["full"] and g["two_graphs"] == [True]      # captured at the shape's second occurrence, replayed from then on
    assert e["keys"] == []
    assert g["calls"] == e["calls"] == steps                        # one exchange per step, eager or replayed
    assert g["step"] == g["step_dev"] == e["step"] == e["step_dev"] == [steps] * W.M
    assert abs(g["loss"] - e["loss"]) <= 2e-3 * abs(e["loss"]), (g["loss"], e["loss"])


def test_ragged_windows_stay_eager_under_data_parallelism(rehearsal):
    assert rehearsal["capturable_full"] is True and rehearsal["capturable_ragged"] is False
    assert rehearsal["ragged_refusal"] is not None and "valid-row total" in rehearsal["ragged_refusal"]
    assert rehearsal["feedback_refusal"] is not None and "feedback" in rehearsal["feedback_refusal"]
    # without a process group: as before
    m, opt = W.make_model("jamming-nade", "bf16")
    x = torch.from_numpy(W.batch()).to(W.DEV)
    lens = torch.tensor([6, 3, 5, 6, 2, 6, 4, 1], dtype=torch.int32, device=W.DEV)
    m.train_step(x, lens, opt)
    assert m.capturable(tuple(x.shape), True) and m.capturable(tuple(x.shape), False)
    run = m.graphed_train_step(x, opt, None, warmup=0, lengths=lens)
    assert run.ragged and run.opt_graph is None
    run(x, lens)
    m.check()
