"""Host side of the modes' data-parallel step, without a GPU: the layout of training.GradArena (the copy kernels are not called on CPU
tensors) and the `reduce=` hook of common.capture_train_step."""
import contextlib
import types

import pytest
import torch


def fake_stores(sizes):
    return [types.SimpleNamespace(grad=torch.arange(n, dtype=torch.float32) + 1, step=0) for n in sizes]


def test_grad_arena_layout():
    from multinn_amd.training import GradArena
    sizes = [1, 5, 1025, 4, 8]
    a = GradArena(fake_stores(sizes))
    assert a.offsets == [0, 4, 12, 1040, 1044] and a.sizes == sizes
    assert all(o % 4 == 0 for o in a.offsets) and a.flat.numel() == 1052 and a.flat.dtype == torch.float32
    assert not a.single and float(a.flat.abs().sum()) == 0          # the gaps (and everything else, before the first pack) are zero
    for i, n in enumerate(sizes):
        seg = a.segment(i)
        assert seg.numel() == n and seg.data_ptr() == a.flat.data_ptr() + 4 * a.offsets[i]
    for i in range(len(sizes) - 1):                                  # segments do not overlap
        assert a.offsets[i] + sizes[i] <= a.offsets[i + 1]


def test_single_store_needs_no_arena():
    from multinn_amd.training import GradArena
    st = fake_stores([7])
    a = GradArena(st)
    assert a.single and a.flat is st[0].grad and a.offsets == [0]
    a.pack()                                                        # nothing to copy: no kernel is called (these are CPU tensors)
    a.unpack()
    with pytest.raises(ValueError):
        GradArena([])
    with pytest.raises(ValueError):
        GradArena([types.SimpleNamespace(grad=None)])


def test_arena_cache_follows_the_stores():
    from multinn_amd.training import GradArena
    owner = types.SimpleNamespace()
    stores = fake_stores([3, 9])
    a = GradArena.cached(owner, stores)
    assert GradArena.cached(owner, stores) is a and owner._grad_arena is a
    assert GradArena.cached(owner, list(reversed(stores))) is not a              # other order: another layout
    a = GradArena.cached(owner, stores)
    stores[1].grad = torch.zeros(9)                                              # re-materialised: same size, a new buffer
    b = GradArena.cached(owner, stores)
    assert b is not a and b.key != a.key and b.grads[1] is stores[1].grad
    stores[0].grad = torch.zeros(11)
    assert GradArena.cached(owner, stores).sizes == [11, 9]


def test_several_stores_need_their_arena_under_data_parallelism(monkeypatch):
    """compute_gradients_multi makes no arena of its own: the caller keeps one (GradArena.cached); refused before any device work."""
    from multinn_amd import training
    monkeypatch.setattr(training, "dp_active", lambda: True)
    monkeypatch.setattr(training, "allreduce_flat", lambda grad: pytest.fail("nothing may be exchanged"))
    stores, other = fake_stores([3, 9]), fake_stores([3, 9])
    opt = training.AdamOptimizer(0.01)
    with pytest.raises(ValueError, match="GradArena.cached"):
        training.compute_gradients_multi(opt, stores)
    with pytest.raises(ValueError, match="GradArena.cached"):
        training.compute_gradients_multi(opt, stores, arena=training.GradArena(other))        # laid out for other buffers
    with pytest.raises(ValueError, match="GradArena.cached"):
        training.compute_gradients_multi(opt, stores, arena=training.GradArena(stores[:1]))


class FakeGraph:
    replays = []

    def __init__(self):
        self.name = len(FakeGraph.replays)

    def pool(self):
        return None

    def replay(self):
        FakeGraph.replays.append(self)


@pytest.fixture
def host_capture(monkeypatch):
    """common.capture_train_step with the device taken out: fake graphs, no warm-up stream, a recording allreduce_flat."""
    from multinn_amd import common, training
    calls = []
    monkeypatch.setattr(common, "_warm_up", lambda fn, n=1: None)
    monkeypatch.setattr(common, "graph_capture", lambda g, **kw: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
    monkeypatch.setattr(training, "allreduce_flat", lambda grad: calls.append(grad))
    FakeGraph.replays = []
    return calls


def test_capture_train_step_reduces_every_store_by_default(host_capture):
    from multinn_amd.common import capture_train_step
    stores = fake_stores([3, 9])
    ran = []
    run = capture_train_step(lambda: ran.append("feed"), lambda: None, 0, [], lambda: stores, split=True, fwd_bwd=lambda: "loss",
                             opt=lambda: ran.append("opt"))
    assert ran == ["opt"] and [st.step for st in stores] == [-1, -1]            # the capture executed nothing
    assert run() == "loss"
    assert [g is st.grad for g, st in zip(host_capture, stores)] == [True, True]   # today's loop: one all-reduce per store
    assert FakeGraph.replays == [run.graph, run.opt_graph] and [st.step for st in stores] == [0, 0]


def test_capture_train_step_reduce_hook_replaces_the_loop(host_capture):
    from multinn_amd.common import capture_train_step
    stores = fake_stores([3, 9])
    order = []
    run = capture_train_step(lambda: order.append("feed"), lambda: None, 0, [], lambda: stores, split=True, fwd_bwd=lambda: "loss",
                             opt=lambda: None, reduce=lambda: order.append(("reduce", len(FakeGraph.replays))))
    run()
    assert host_capture == []                                                    # no per-store exchange
    assert order == ["feed", ("reduce", 1)]                                      # between the two replays
    assert len(FakeGraph.replays) == 2
    single = capture_train_step(lambda: None, lambda: "loss", 0, [], lambda: stores, reduce=lambda: order.append("never"))
    single()
    assert single.opt_graph is None and "never" not in order                    # one rank, one graph: nothing to reduce
