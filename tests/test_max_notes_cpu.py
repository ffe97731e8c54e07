"""The polyphony cap without a GPU: the one normalisation helper (common.sampling_max_notes) and every ValueError it owes; the refusals of RBM
generators, DBN encoders and host models -- all before any device work (the models live on the host: anything that reached a kernel would
raise a plain MnnError or ValueError from the ops layer) --; the scan-graph key; the C-ABI additions; the ops wrappers' choice of entry point."""
import os
import re
import subprocess

import pytest
import torch

from test_modes_cpu import config, params

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mnn_nade_sample_caps_at", "mnn_nade_sample_multi_caps", "mnn_generate_scan_caps", "mnn_generate_scan_chunk_caps")
TRACKS = ("Drums", "Piano", "Guitar")


# ------------------------------------------------------------------------------------------------
# 1. the helper
def test_normalisation():
    from multinn_amd.common import sampling_max_notes as mn, max_notes_key
    assert mn(None) is None and mn(None, 3) is None
    assert mn(2, 3) == 2 and isinstance(mn(2, 3), int) and mn(0, 3) == 0
    assert mn((1, None, 0), 3) == (1, None, 0) and isinstance(mn([1, None, 0], 3), tuple)
    assert mn(torch.tensor([1, 2, 0]), 3) == (1, 2, 0)
    # the three normalisations to None / to the scalar
    assert mn((2, 2, 2), 3) == 2 and isinstance(mn((2, 2, 2), 3), int)          # equal entries are the scalar
    assert mn((None, None, None), 3) is None                                    # all-None is None
    assert mn(12, 3, 12) is None and mn(50, 3, 12) is None and mn(11, 3, 12) == 11     # a cap >= D is None
    assert mn((12, 40, None), 3, 12) is None and mn((12, 3, None), 3, 12) == (None, 3, None)
    # inside ONE NADE a sequence counts by visible index and an integer counts the whole of it: equal entries stay a sequence there
    assert mn((2, 2, 2), 3, 4, collapse=False) == (2, 2, 2) and mn((None,) * 3, 3, 4, collapse=False) is None
    # the scan-graph key gains nothing at None
    assert max_notes_key(None) == () and max_notes_key(mn((None, None), 2)) == () and max_notes_key(mn(99, 3, 12)) == ()
    assert max_notes_key(1) != () and max_notes_key(1) != max_notes_key(2) and max_notes_key((1, None, 0)) != max_notes_key((1, None, 1))


@pytest.mark.parametrize("bad", [-1, 1.0, 2.5, True, False, "two", (1, -1, 0), (1, 2.0, 0), (1, True, 0), (1, "x", 0), float("nan")])
def test_entries_that_are_not_integers_from_zero(bad):
    from multinn_amd.common import sampling_max_notes as mn
    with pytest.raises(ValueError):
        mn(bad, 3)


def test_sequence_lengths():
    from multinn_amd.common import sampling_max_notes as mn
    for bad, M in (((1, 2), 3), ((1, 2, 3, 4), 3), ((), 3), ((1, 2), None), ((1,) * 9, 9), ((None,) * 9, 9)):
        with pytest.raises(ValueError):
            mn(bad, M)
    assert mn((1,) * 8, 8) == 1


# ------------------------------------------------------------------------------------------------
# 2. generators and mode classes: ValueError and the refusals before any device work
def _mode(mode, gen, enc="Pass"):
    from multinn_amd import modes
    fb = [32, 16] if mode.startswith("feedback") else None
    p = params(mode, enc=enc, enc_hidden=None if enc == "Pass" else [6, 4], gen=gen, feedback=fb)
    return modes.MultINN(config(8, TRACKS), p, mode=mode, device=CPU)


BAD_ANYWHERE = [-1, 1.5, True, (1, 2), (1, 2, 3, 4), (1, -1, 0), (1,) * 9]
MODES = [("joint", "NADE"), ("jamming", "NADE"), ("composer", "NADE"), ("feedback", "NADE"), ("feedback-rnn", "NADE")]


@pytest.mark.parametrize("mode,gen", MODES + [("joint", "RBM"), ("jamming", "RBM"), ("composer", "MultiRBM"), ("feedback", "RBM")])
def test_modes_refuse_bad_caps(mode, gen):
    m = _mode(mode, gen)
    for bad in BAD_ANYWHERE:
        with pytest.raises(ValueError):
            m.generate(4, max_notes=bad)
        with pytest.raises(ValueError):
            m.sampler(1, max_notes=bad)
    assert m._max_notes(None) is None


@pytest.mark.parametrize("mode,gen", [("joint", "RBM"), ("jamming", "RBM"), ("composer", "MultiRBM"), ("feedback", "RBM"), ("feedback-rnn", "RBM")])
def test_rbm_generators_are_refused(mode, gen):
    from multinn_amd._lib import MnnUnsupported
    m = _mode(mode, gen)
    for cap in (1, 0, (1, None, 0), 100):
        with pytest.raises(MnnUnsupported, match="NADE generators only"):
            m.generate(4, max_notes=cap)
        with pytest.raises(MnnUnsupported, match="NADE generators only"):
            m.sampler(1, max_notes=cap)


@pytest.mark.parametrize("mode,gen", MODES)
def test_host_models_are_refused(mode, gen):
    from multinn_amd._lib import MnnUnsupported
    m = _mode(mode, gen)
    for cap in (1, (1, None, 0)):
        with pytest.raises(MnnUnsupported, match="not a ROCm device"):
            m.generate(4, max_notes=cap)


@pytest.mark.parametrize("mode", ["joint", "jamming", "composer", "feedback"])
def test_dbn_encoders_are_refused(mode):
    from multinn_amd._lib import MnnUnsupported
    m = _mode(mode, "NADE", enc="DBN")
    with pytest.raises(MnnUnsupported, match="DBN"):
        m.generate(4, max_notes=1)
    with pytest.raises(ValueError):
        m.generate(4, max_notes=-1)


def test_generators_validate_and_refuse():
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM, RnnMultiRBM
    from multinn_amd._lib import MnnUnsupported
    x = torch.zeros((2, 3, 12), dtype=torch.uint8)
    nade = RnnNade(12, 8, [32], device=CPU)
    multi = RnnMultiNADE(4, 8, [32], tracks=list("abc"), device=CPU)
    rbm = RnnRBM(12, 8, [32], device=CPU)
    mrbm = RnnMultiRBM(4, 8, [32], tracks=list("abc"), device=CPU)
    for g in (nade, multi):
        for bad in (-1, 1.5, True, (1,) * 9, (1, -2, 0)):
            with pytest.raises(ValueError):
                g.generate(x, 2, max_notes=bad)
        with pytest.raises(MnnUnsupported, match="not a ROCm device"):      # the host model's refusal, after the validation
            g.generate(x, 2, max_notes=1)
    for g in (rbm, mrbm):
        with pytest.raises(MnnUnsupported, match="NADE generators only"):
            g.generate(x, 2, max_notes=1)
    assert multi._max_notes((1, None, 0)) == (1, None, 0) and multi._max_notes((2, 2, 2)) == 2 and multi._max_notes(4) is None
    with pytest.raises(ValueError):
        multi.generate(x, 2, max_notes=(1, 2))
    # one NADE: an integer caps the whole vector; a sequence of n entries (n dividing the visibles) counts visible i in entry i % n
    assert nade._max_notes(3) == 3 and nade._max_notes(12) is None
    assert nade._max_notes((1, None, 0)) == (1, None, 0) and nade._max_notes((2, 2, 2)) == (2, 2, 2) and nade._max_notes((4, None, 9)) is None
    with pytest.raises(ValueError):
        nade.generate(x, 2, max_notes=(1, 2, 3, 4, 5))


def test_the_modes_hand_each_generator_its_cap():
    joint, jam, comp = _mode("joint", "NADE"), _mode("jamming", "NADE"), _mode("composer", "NADE")
    assert joint._generator_max_notes(2) == [(2, 2, 2)] and joint._generator_max_notes((1, None, 0)) == [(1, None, 0)]
    assert jam._generator_max_notes(2) == [2, 2, 2] and jam._generator_max_notes((1, None, 0)) == [1, None, 0]
    assert comp._generator_max_notes((1, None, 0)) == [(1, None, 0)] and comp._generator_max_notes(2) == [2]


# ------------------------------------------------------------------------------------------------
# 3. the scan-graph key
def test_the_cap_is_part_of_the_graph_key_and_none_leaves_it_alone(monkeypatch):
    from multinn_amd.common import ScanGraphs
    keys, calls = [], []
    monkeypatch.setattr(ScanGraphs, "enabled", staticmethod(lambda x: True))

    def run(self, key, x, scan, warm, after_capture, extra=None):
        keys.append(key)
        return scan(x)
    monkeypatch.setattr(ScanGraphs, "run", run)

    class Owner:
        pass

    def scan(*a):
        calls.append(a)
        return a[0]
    x = torch.zeros(1)
    base = ("k", 3)
    ScanGraphs.generate(Owner(), base, x, 3, None, 1.0, scan, lambda: None)
    ScanGraphs.generate(Owner(), base, x, 3, None, 1.0, scan, lambda: None, None)
    assert keys == [base, base] and all(len(c) == 4 for c in calls)              # the key and the call of before
    ScanGraphs.generate(Owner(), base, x, 3, None, 1.0, scan, lambda: None, 2)
    ScanGraphs.generate(Owner(), base, x, 3, None, 0.5, scan, lambda: None, (1, None, 0))
    assert keys[2] == base + (("max_notes", 2),) and keys[3] == base + (("temperature", 0.5), ("max_notes", (1, None, 0)))
    assert calls[2][4] == 2 and calls[3][4] == (1, None, 0)


def test_scan_steps_takes_the_capped_step_only_when_there_is_a_cap():
    from multinn_amd.common import DrawAt
    from multinn_amd.generators import RnnEstimator
    plain, capped = [], []

    class G(RnnEstimator):
        def __init__(self):
            pass

        def sample_single(self, inputs, state, **kw):
            plain.append(kw)
            return inputs, None

        def sample_single_capped(self, inputs, state, **kw):
            capped.append(kw)
            return inputs, None

        def single_step(self, inputs, initial_state, x2=None):
            return initial_state
    G.__abstractmethods__ = frozenset()
    g = G()
    row = torch.zeros((2, 4), dtype=torch.uint8)
    g._scan_steps(0, row, 2, DrawAt(1, 0, 0))
    assert len(plain) == 2 and not capped and all("max_notes" not in kw for kw in plain)      # the step loop of before
    plain.clear()
    g._scan_steps(0, row, 2, DrawAt(1, 0, 0), None, 1.0, (1, None))
    assert not plain and [kw["max_notes"] for kw in capped] == [(1, None)] * 2 and [kw["at"].step for kw in capped] == [0, 1]


def test_sample_single_keeps_its_signature_and_the_capped_step_adds_the_cap():
    import inspect
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM
    for cls in (RnnNade, RnnMultiNADE):
        assert list(inspect.signature(cls.sample_single).parameters) == ["self", "inputs", "state", "given", "temperature", "at"]
        ps = inspect.signature(cls.sample_single_capped).parameters
        assert list(ps) == ["self", "inputs", "state", "given", "temperature", "at", "max_notes"]
        assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("given", "temperature", "at", "max_notes"))
        assert ps["max_notes"].default is None
    assert not hasattr(RnnRBM, "sample_single_capped")
    for name in ("generate", "sampler"):
        from multinn_amd.modes import MultINNCore
        assert inspect.signature(getattr(MultINNCore, name)).parameters["max_notes"].default is None
    assert inspect.signature(RnnNade.generate).parameters["max_notes"].default is None


def test_sample_single_capped_picks_the_entry_point(monkeypatch):
    """ops.call recorded with the device taken away: without a cap the capped step is sample_single's launch, with one the caps entry point."""
    import ctypes as C
    from multinn_amd import ops, _lib, RnnNade
    from multinn_amd.common import DrawAt
    from multinn_amd.generators import RnnEstimatorStateTuple
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    N, D, Hn = 3, 12, 8
    nade = RnnNade(D, Hn, [32], device=CPU, seed=100)
    nade._materialize(D)
    dense = torch.zeros((N, nade.ldo))
    st = RnnEstimatorStateTuple(dense[:, :Hn], dense[:, Hn:Hn + D], ())
    st.dense = dense
    nade.sample_single(None, st, at=DrawAt(7, 3, 5))
    nade.sample_single_capped(None, st, at=DrawAt(7, 3, 5))
    nade.sample_single_capped(None, st, at=DrawAt(7, 3, 5), max_notes=2)
    nade.sample_single_capped(None, st, at=DrawAt(7, 3, 5), max_notes=(1, None, 0))
    assert [c[0] for c in calls] == ["mnn_nade_sample", "mnn_nade_sample", "mnn_nade_sample_caps_at", "mnn_nade_sample_caps_at"]
    assert len(calls[0][1]) == len(calls[1][1]) == 19 and calls[0][1][9:13] == calls[1][1][9:13] and len(calls[2][1]) == 21
    assert [c[1][11:14] for c in calls[2:]] == [(7, 3, 5)] * 2
    cap = C.cast(calls[3][1][10], C.POINTER(_lib.Caps)).contents
    assert (cap.n, cap.by_visible, tuple(cap.cap[i] for i in range(3))) == (3, 1, (1, -1, 0))


def test_sessions_carry_the_cap_as_a_checked_property():
    """The setter's checks without a session on a device: the property objects applied to stand-ins that hold what the setters read."""
    import inspect
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd.session import GeneratorSession, ModeSession
    assert list(inspect.signature(GeneratorSession.generate).parameters) == ["self", "num_steps", "given", "temperature"]
    assert list(inspect.signature(ModeSession.generate).parameters) == ["self", "num_steps", "given", "given_mask", "temperature"]
    assert isinstance(GeneratorSession.max_notes, property) and isinstance(ModeSession.max_notes, property)

    def stand_in(cls, **attrs):
        s = cls.__new__(cls)
        s._max_notes = None
        for k, v in attrs.items():
            setattr(s, k, v)
        return s
    s = stand_in(GeneratorSession, _gen=RnnMultiNADE(4, 8, [32], tracks=list("abc"), device=CPU))
    assert s.max_notes is None
    s.max_notes = (1, None, 0)
    assert s.max_notes == (1, None, 0)
    s.max_notes = (2, 2, 2)
    assert s.max_notes == 2
    s.max_notes = 4                                             # a cap >= the visibles of a track
    assert s.max_notes is None
    for bad in (-1, 1.5, True, (1, 2)):
        with pytest.raises(ValueError):
            s.max_notes = bad
    assert s.max_notes is None
    r = stand_in(GeneratorSession, _gen=RnnRBM(12, 8, [32], device=CPU))
    with pytest.raises(MnnUnsupported, match="NADE generators only"):
        r.max_notes = 1
    r.max_notes = None
    # a mode's session: the mode's own checks (here: a model on the host), before any of its generators' sessions is touched
    m = stand_in(ModeSession, _model=_mode("jamming", "NADE")._model, _subs=[])
    with pytest.raises(ValueError):
        m.max_notes = (1, 2)
    with pytest.raises(MnnUnsupported, match="not a ROCm device"):
        m.max_notes = (1, None, 0)
    m.max_notes = None
    assert m.max_notes is None


# ------------------------------------------------------------------------------------------------
# 4. the C ABI: additions only, no version bump
def _header_decl(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
    return None if m is None else re.sub(r"\s+", " ", m.group(1))


def test_new_symbols_in_header_loader_and_library():
    import ctypes as C
    from multinn_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    S = _lib.SIGNATURES
    for new, old in zip(NEW_SYMBOLS, ("mnn_nade_sample_temps_at", "mnn_nade_sample_multi_temps", "mnn_generate_scan_temps", "mnn_generate_scan_chunk")):
        a, b = _header_decl(header, old), _header_decl(header, new)
        assert b is not None and a.replace("const mnn_temps* temps,", "const mnn_temps* temps, const mnn_caps* caps,") == b, new
        assert len(S[new][1]) == len(S[old][1]) + 1
    assert re.search(r"#define\s+MNN_ABI_VERSION\s+124\b", header) and _lib.ABI_VERSION == 124
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\bT (mnn_[a-z0-9_]+)", out))
    assert re.search(r"typedef struct \{\s*int n;\s*int by_visible;\s*int32_t cap\[MNN_TEMPS_MAX\];\s*\} mnn_caps;", header)
    assert C.sizeof(_lib.Caps) == 40 and _lib.Caps.cap.offset == 8 and _lib.Caps.by_visible.offset == 4


def test_library_validates_caps_on_the_host(lib):
    """Null device pointers throughout: the checks of the table answer before anything else could."""
    import ctypes as C
    from multinn_amd import _lib
    t, c = _lib.Temps(), _lib.Caps()
    t.n, t.t[0] = 1, 1.0
    one = C.c_void_p(16)
    c.n = 9
    rc = lib.mnn_nade_sample_caps_at(None, 1, 4, 8, 16, one, 32, one, one, C.byref(t), C.byref(c), 1, 0, 0, one, 8, 8, 1, None, None, None)
    assert rc == -1 and b"caps" in lib.mnn_last_error()
    c.n = 2                                                     # two caps per track, three tracks
    rc = lib.mnn_nade_sample_caps_at(None, 3, 4, 8, 16, one, 96, one, one, C.byref(t), C.byref(c), 1, 0, 0, one, 8, 24, 1, None, None, None)
    assert rc == -1 and b"caps" in lib.mnn_last_error()
    jobs = (_lib.NadeSampleJob * 3)()
    rc = lib.mnn_nade_sample_multi_caps(None, 3, jobs, 4, 8, 16, C.byref(t), C.byref(c), 0, 0, 8, 1)
    assert rc == -1 and b"caps" in lib.mnn_last_error()


# ------------------------------------------------------------------------------------------------
# 5. the ops wrappers
def test_ops_wrappers_refuse_bad_caps_before_any_device_work():
    """Host tensors throughout: a wrapper that reached the device would raise MnnError (no CPU path), not ValueError."""
    from multinn_amd import ops
    N, D, Hn = 4, 6, 8
    bias = torch.zeros((N, 2 * (Hn + D)))
    w = torch.zeros((2, D, Hn))
    out = torch.zeros((N, 2 * D), dtype=torch.uint8)
    for bad in ((1, 2, 3), (1, -1), (1,) * 9, (), (1, 1.5), -1, True):
        with pytest.raises(ValueError):
            ops.nade_sample(bias, w, w, 2, D, Hn, 1.0, 1, 0, 0, out, max_notes=bad)


def test_ops_wrappers_pick_the_entry_point_by_the_cap(monkeypatch):
    """The wrappers' argument building with the device taken away: None -- and a table of Nones -- goes to the entry point of before, a cap
    to the one that takes both tables."""
    import ctypes as C
    from multinn_amd import ops, _lib
    calls = []
    monkeypatch.setattr(ops, "_ptr", lambda t: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "call", lambda name, *args: calls.append((name, args)))

    def caps(arg):
        c = C.cast(arg, C.POINTER(_lib.Caps)).contents
        return c.n, c.by_visible, tuple(c.cap[i] for i in range(c.n))

    def temps(arg):
        t = C.cast(arg, C.POINTER(_lib.Temps)).contents
        return t.n, t.by_visible, tuple(round(t.t[i], 6) for i in range(t.n))

    B, Ti, tracks, D, Hn, u, steps = 2, 3, 3, 4, 8, 32, 5
    intro = torch.zeros((B, Ti, tracks * D), dtype=torch.uint8)
    layers = [(torch.zeros((tracks * D + u, 4 * u)), torch.zeros(4 * u))]
    w = torch.zeros((tracks, D, Hn))
    scan = lambda t, **kw: ops.generate_scan(intro, steps, layers, torch.zeros((u, tracks * (Hn + D))), None, tracks, D, Hn, w, w, t, 1, 0, **kw)
    for kw in ({}, {"max_notes": None}, {"max_notes": (None, None, None)}):
        calls.clear()
        scan(1.0, **kw)
        assert calls[0][0] == "mnn_generate_scan" and len(calls[0][1]) == 23
    calls.clear()
    assert tuple(scan(None, max_notes=(1, None, 0)).shape) == (B, steps, tracks * D)
    assert calls[0][0] == "mnn_generate_scan_caps" and len(calls[0][1]) == 26
    assert temps(calls[0][1][16]) == (0, 0, ()) and caps(calls[0][1][17]) == (3, 0, (1, -1, 0))
    calls.clear()
    scan(0.7, max_notes=2)
    assert temps(calls[0][1][16]) == (1, 0, (0.7,)) and caps(calls[0][1][17]) == (1, 0, (2,))
    state = [(torch.zeros((B, u)), torch.zeros((B, u)))]
    chunk = lambda **kw: ops.generate_scan_chunk(None, steps, layers, torch.zeros((u, tracks * (Hn + D))), None, tracks, D, Hn, w, w, 1.0, 1, 0,
                                                 state, state, **kw)
    calls.clear()
    chunk()
    assert calls[0][0] == "mnn_generate_scan_chunk" and len(calls[0][1]) == 29
    calls.clear()
    chunk(max_notes=(1, None, 0))
    assert calls[0][0] == "mnn_generate_scan_chunk_caps" and len(calls[0][1]) == 30 and caps(calls[0][1][17]) == (3, 0, (1, -1, 0))
    # the single sampling step: one NADE by visible index, a MultiNADE per track
    bias = torch.zeros((B, tracks * (Hn + D)))
    out = torch.zeros((B, tracks * D), dtype=torch.uint8)
    for kw, name, n in (({}, "mnn_nade_sample", 19), ({"max_notes": None}, "mnn_nade_sample", 19), ({"max_notes": 1}, "mnn_nade_sample_caps_at", 21),
                        ({"max_notes": (1, None, 0)}, "mnn_nade_sample_caps_at", 21)):
        calls.clear()
        ops.nade_sample(bias, w, w, tracks, D, Hn, 1.0, 1, 0, 0, out, **kw)
        assert calls[0][0] == name and len(calls[0][1]) == n
    assert caps(calls[0][1][10]) == (3, 0, (1, -1, 0))
    calls.clear()
    w1 = torch.zeros((1, 12, Hn))
    ops.nade_sample(torch.zeros((B, Hn + 12)), w1, w1, 1, 12, Hn, 1.0, 1, 0, 0, torch.zeros((B, 12), dtype=torch.uint8), by_visible=True,
                    max_notes=(1, None, 2, 0))
    assert caps(calls[0][1][10]) == (4, 1, (1, -1, 2, 0))
    jobs = [dict(bias=torch.zeros((B, Hn + D)), w_enc=w[0], w_dec=w[0], seed=i, samples=torch.zeros((B, D), dtype=torch.uint8)) for i in range(3)]
    for kw, name, n in (({}, "mnn_nade_sample_multi", 11), ({"max_notes": (1, None, 0)}, "mnn_nade_sample_multi_caps", 12)):
        calls.clear()
        ops.nade_sample_multi(jobs, D, Hn, 1.0, 0, 0, **kw)
        assert calls[0][0] == name and len(calls[0][1]) == n
    assert caps(calls[0][1][7]) == (3, 0, (1, -1, 0))
