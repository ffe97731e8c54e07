"""The host side of the generation path without a GPU: the one step loop (RnnEstimator._scan_steps) and the draw position it hands on
(common.DrawAt), the one `given` check, the mode hooks that map codes to the generators and samples back, and the absence of the hidden
attributes the position used to travel through."""
import ctypes as C

import pytest
import torch

from test_modes_cpu import config, params

CPU = torch.device("cpu")
TRACKS = ("Drums", "Piano", "Guitar")


# ------------------------------------------------------------------------------------------------
# 1. the step loop
def _stub(n_out=4):
    """An estimator whose sample_single / single_step only record: the state is a step count, a sampled row holds the step it was drawn at."""
    from multinn_amd import generators

    class Stub(generators.RnnEstimator):
        def __init__(self):
            self.samples, self.steps_taken = [], []

        def sample_single(self, inputs, state, *, given=None, temperature=1.0, at=None):
            self.samples.append((inputs.clone(), state, None if given is None else given.clone(), temperature, at))
            return torch.full((2, n_out), at.step, dtype=torch.uint8), None

        def single_step(self, inputs, initial_state, x2=None):
            self.steps_taken.append((inputs.clone(), initial_state))
            return initial_state + 1
    Stub.__abstractmethods__ = frozenset()
    return Stub()


@pytest.mark.parametrize("base", [None, "cell"])
def test_one_call_and_chunks_record_the_same_steps(base):
    from multinn_amd.common import DrawAt
    n_out, temperature = 4, (0.5, 2.0)
    base = torch.zeros(1, dtype=torch.int32) if base == "cell" else None
    given = torch.arange(2 * 6 * n_out, dtype=torch.uint8).reshape(2, 6, n_out)
    first = torch.full((2, n_out), 99, dtype=torch.uint8)

    whole = _stub(n_out)
    out, state, last = whole._scan_steps(0, first, 6, DrawAt(7, 3, 0, base), given, temperature)
    assert out.shape == (2, 6, n_out) and state == 6 and torch.equal(last, out[:, -1])
    assert [int(out[0, j, 0]) for j in range(6)] == list(range(6))

    parts = _stub(n_out)
    outs, state, last, s = [], 0, first, 0
    for n in (1, 2, 3):                                          # at0.step = 0, 1, 3
        o, state, last = parts._scan_steps(state, last, n, DrawAt(7, 3, s, base), given[:, s:s + n], temperature)
        outs.append(o)
        s += n
    assert state == 6 and torch.equal(torch.cat(outs, 1), out)

    for rec in (whole, parts):
        ats = [c[4] for c in rec.samples]
        assert [(a.seed, a.row0, a.step) for a in ats] == [(7, 3, j) for j in range(6)]
        assert all(a.base is base for a in ats)                  # passed through untouched
        assert [c[1] for c in rec.samples] == list(range(6)) and [c[1] for c in rec.steps_taken] == list(range(6))
        assert all(c[3] == temperature for c in rec.samples)
        for j, c in enumerate(rec.samples):
            assert torch.equal(c[2], given[:, j])                # the step's slice of the codes
            assert torch.equal(c[0], first if j == 0 else out[:, j - 1])      # the row before it
            assert torch.equal(rec.steps_taken[j][0], out[:, j])              # its own row goes into the LSTM step


def test_without_given_the_steps_get_none_and_the_default_temperature():
    from multinn_amd.common import DrawAt
    g = _stub()
    g._scan_steps(0, torch.zeros((2, 4), dtype=torch.uint8), 2, DrawAt(1, 0, 5))
    assert [(c[2], c[3], c[4]) for c in g.samples] == [(None, 1.0, DrawAt(1, 0, 5, None)), (None, 1.0, DrawAt(1, 0, 6, None))]


def test_draw_position_is_an_immutable_value():
    from multinn_amd.common import DrawAt
    at = DrawAt(7, 3, 5)
    assert at == (7, 3, 5, None) and at.base is None and at._replace(step=6) == DrawAt(7, 3, 6)
    with pytest.raises(AttributeError):
        at.step = 6


def test_sample_single_takes_its_position_from_the_argument_alone(monkeypatch):
    """ops.call recorded with the device taken away (as test_session_cpu does): seed, row0, sub-counter and the trailing cell pointer of the
    sampling launch are those of `at` -- step for a NADE, step * max(k, 1) for an RBM's chain -- whatever the generator's own seed and row0."""
    from multinn_amd import ops, RnnNade, RnnRBM
    from multinn_amd.common import DrawAt
    from multinn_amd.generators import RnnEstimatorStateTuple
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    monkeypatch.setattr(ops, "rbm_workspace", lambda D, Hn, device: torch.zeros(1, dtype=torch.uint8))
    N, D, Hn = 3, 12, 8
    cell = torch.zeros(1, dtype=torch.int32)
    nade = RnnNade(D, Hn, [32], device=CPU, seed=100)
    rbm = RnnRBM(D, Hn, [32], k=4, device=CPU, seed=100)
    for g in (nade, rbm):
        g._materialize(D)
        g.row0 = 50
    dense = torch.zeros((N, nade.ldo))
    st = RnnEstimatorStateTuple(dense[:, :Hn], dense[:, Hn:Hn + D], ())
    st.dense = dense
    nade.sample_single(None, st, at=DrawAt(7, 3, 5))
    nade.sample_single(None, st, at=DrawAt(7, 3, 5, cell))
    nade.sample_single(None, st)
    assert [c[0] for c in calls] == ["mnn_nade_sample", "mnn_nade_sample_temps_at", "mnn_nade_sample"]
    assert [c[1][10:13] for c in calls] == [(7, 3, 5), (7, 3, 5), (100, 50, 0)]
    assert calls[1][1][-1].value == cell.data_ptr()
    calls.clear()
    v0 = torch.zeros((N, D), dtype=torch.uint8)
    st = RnnEstimatorStateTuple(torch.zeros((N, Hn)), torch.zeros((N, D)), ())
    rbm.sample_single(v0, st, at=DrawAt(7, 3, 5))
    rbm.sample_single(v0, st, at=DrawAt(7, 3, 5, cell))
    rbm.sample_single(v0, st)
    assert [c[0] for c in calls] == ["mnn_rbm_gibbs", "mnn_rbm_gibbs_at", "mnn_rbm_gibbs"]
    assert [(c[1][11], c[1][12], c[1][14]) for c in calls] == [(7, 3, 20), (7, 3, 20), (100, 50, 0)]      # k = 4 sub-counters per step
    assert calls[1][1][-1].value == cell.data_ptr()
    for g in (nade, rbm):
        assert (g.seed, g.row0) == (100, 50)


def test_given_and_temperature_are_keyword_only_in_one_order():
    import inspect
    from multinn_amd import RnnNade, RnnRBM, RnnMultiRBM
    for cls in (RnnNade, RnnRBM, RnnMultiRBM):
        ps = inspect.signature(cls.sample_single).parameters
        assert list(ps) == ["self", "inputs", "state", "given", "temperature", "at"]
        assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("given", "temperature", "at"))
        assert ps["given"].default is None and ps["temperature"].default == 1.0 and ps["at"].default is None


# ------------------------------------------------------------------------------------------------
# 2. the `given` check
def test_one_given_check_one_text():
    from multinn_amd import RnnNade
    from multinn_amd.common import check_given
    from multinn_amd.session import _chunk_arguments
    codes = torch.full((2, 3, 12), 255, dtype=torch.uint8)
    check_given(codes, 2, 3, 12)
    check_given(codes.reshape(2, 3, 4, 3), 2, 3, 4, 3)                       # the feedback scan's [B, n, P, M]: the same check, another tail
    gen = RnnNade(12, 8, [32], device=CPU)
    x = torch.zeros((2, 4, 12), dtype=torch.uint8)
    for bad, got in ((codes.float(), "torch.float32 (2, 3, 12)"), (codes.reshape(2, 36), "torch.uint8 (2, 36)"), (codes[:, :2], "torch.uint8 (2, 2, 12)")):
        text = f"given must be u8 [2, 3, 12], got {got}"
        for raises in (lambda: check_given(bad, 2, 3, 12), lambda: gen.generate(x, 3, given=bad), lambda: _chunk_arguments(gen, 2, 0, 3, bad)):
            with pytest.raises(ValueError) as e:
                raises()
            assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        check_given(codes, 2, 3, 4, 3)
    assert str(e.value) == "given must be u8 [2, 3, 4, 3], got torch.uint8 (2, 3, 12)"
    with pytest.raises(ValueError, match=r"given must be u8 \[2, 3, 12\], got list"):
        check_given([[0]], 2, 3, 12)
    assert gen.store.theta is None                                           # refused before anything was materialised


# ------------------------------------------------------------------------------------------------
# 3. the mode hooks
@pytest.mark.parametrize("mode,gen", [("joint", "NADE"), ("jamming", "NADE"), ("composer", "NADE"), ("composer", "MultiRBM")])
def test_mode_hooks_round_trip_a_code_block(mode, gen):
    """Generators that return their `given`: codes -> per-generator given -> "samples" -> [B, n, P, M] is the identity."""
    from multinn_amd import modes
    B, n, P, M = 2, 5, 4, 3
    m = modes.MultINN(config(P, TRACKS), params(mode, gen=gen), mode=mode, device=CPU)
    codes = torch.randint(0, 2, (B, n, P, M), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    ran = []

    def scan(i):
        def run(num_steps, given=None, temperature=1.0):
            ran.append((i, temperature))
            assert num_steps == n and given.is_contiguous() and given.shape[:2] == (B, n)
            return given
        return run
    G = len(m.generators)
    assert G == (M if mode == "jamming" else 1)
    cond = (codes, [False] * M, [True] * M)
    for session in (False, True):
        givens = m._generator_given(cond, session)
        assert len(givens) == G and all(run for _, run in givens)
        assert [tuple(gv.shape) for gv, _ in givens] == ([(B, n, P)] * M if mode == "jamming" else [(B, n, P * M)])
        assert torch.equal(m._decode_samples([gv for gv, _ in givens], n), codes)
        ran.clear()
        out = m._sample_generators([scan(i) for i in range(G)], n, cond, (0.5, 1.0, 2.0), session=session)
        assert torch.equal(out, codes) and out.dtype == torch.uint8
        # M generators take one temperature each, one generator the whole sequence
        assert ran == ([(0, 0.5), (1, 1.0), (2, 2.0)] if mode == "jamming" else [(0, (0.5, 1.0, 2.0))])
    if mode == "jamming":
        # a wholly given track: generate does not sample it, a session still runs its clamped chunk; a free track gets no codes
        cond = (codes, [True, False, False], [True, False, True])
        assert [(gv is None, run) for gv, run in m._generator_given(cond, False)] == [(False, False), (True, True), (False, True)]
        assert [(gv is None, run) for gv, run in m._generator_given(cond, True)] == [(False, True), (True, True), (False, True)]
        ran.clear()
        free = torch.zeros((B, n, P), dtype=torch.uint8)
        scans = [scan(0), lambda num_steps, given=None, temperature=1.0: free, scan(2)]
        out = m._sample_generators(scans, n, cond, 1.0)
        assert ran == [(2, 1.0)] and torch.equal(out[..., 0], codes[..., 0]) and torch.equal(out[..., 2], codes[..., 2]) and not out[..., 1].any()


# ------------------------------------------------------------------------------------------------
# 4. no hidden position on a generator
def test_generators_carry_no_hidden_draw_position():
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM, RnnMultiRBM, generators
    gens = (RnnNade(12, 8, [32], device=CPU), RnnMultiNADE(4, 8, [32], tracks=list("abc"), device=CPU),
            RnnRBM(12, 8, [32], k=4, device=CPU), RnnMultiRBM(4, 8, [32], tracks=list("abc"), k=0, device=CPU))
    for g in gens + (generators.RnnEstimator, generators.RnnNade, generators.RnnMultiNADE, generators.RnnRBM, generators.RnnMultiRBM):
        assert not hasattr(g, "_gen_step") and not hasattr(g, "_gen_base") and not hasattr(g, "_last_dense")
