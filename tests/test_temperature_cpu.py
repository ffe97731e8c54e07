"""Sampling temperature without a GPU: the one normalisation helper (common.sampling_temperature) and every ValueError it owes, through the
helper, the generators and the mode classes -- all before any device work (the models live on the host: anything that reached a kernel
would raise MnnError) --, the scan-graph key, the C-ABI additions in header / loader / library, and the ops wrappers' host checks."""
import math
import os
import re
import subprocess

import pytest
import torch

from test_modes_cpu import config, params

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mnn_nade_sample_temps", "mnn_nade_sample_multi_temps", "mnn_generate_scan_temps", "mnn_rbm_gibbs_temp", "mnn_rbm_gibbs_multi_temps")
TRACKS = ("Drums", "Piano", "Guitar")


# ------------------------------------------------------------------------------------------------
# 1. the helper
def test_normalisation():
    from multinn_amd.common import sampling_temperature as st, temperature_key
    assert st(1.0) == 1.0 and isinstance(st(1), float) and st(0.8, 3) == 0.8
    assert st(None) is None and st(None, 3) is None
    assert st((0.5, 1.0, 2.0), 3) == (0.5, 1.0, 2.0) and isinstance(st([0.5, 1, 2], 3), tuple)
    assert st(torch.tensor([0.5, 1.0, 2.0]), 3) == (0.5, 1.0, 2.0)
    # a sequence of equal values is the scalar; all ones is 1.0
    assert st((0.7, 0.7, 0.7), 3) == 0.7 and isinstance(st((0.7, 0.7, 0.7), 3), float)
    assert st([1.0, 1, 1.0], 3) == 1.0
    assert st((2.0,) * 8, 8) == 2.0
    # the scan-graph key gains nothing at 1.0
    assert temperature_key(1.0) == () and temperature_key(st([1, 1, 1], 3)) == ()
    assert temperature_key(0.8) != () and temperature_key((0.5, 1.0, 2.0)) != temperature_key((0.5, 1.0, 4.0)) and temperature_key(None) != ()


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, math.inf, -math.inf, math.nan, "hot", True, (0.5, 0.0, 1.0), (1.0, math.nan, 1.0), (1.0, math.inf, 2.0),
                                 (1.0, -2.0, 1.0), (0.5, "x", 1.0)])
def test_values_that_are_not_positive_and_finite(bad):
    from multinn_amd.common import sampling_temperature as st
    with pytest.raises(ValueError):
        st(bad, 3)


def test_sequence_lengths_and_modes_of_the_helper():
    from multinn_amd.common import sampling_temperature as st, MAX_TEMPERATURE_TRACKS
    assert MAX_TEMPERATURE_TRACKS == 8
    for bad, M in (((0.5, 1.0), 3), ((0.5, 1.0, 2.0, 1.0), 3), ((), 3), ((0.5, 2.0), None), ((1.0,) * 9, 9), ((0.5,) * 9, 9)):
        with pytest.raises(ValueError):
            st(bad, M)
    with pytest.raises(ValueError, match="RBM"):
        st(None, 3, allow_none=False)
    with pytest.raises(ValueError):
        st((0.5, 1.0, 2.0), 3, allow_sequence=False)
    with pytest.raises(ValueError):
        st((1.0, 1.0, 1.0), 3, allow_sequence=False)           # no per-track temperature here, whatever the values
    assert st(2.0, 3, allow_none=False, allow_sequence=False) == 2.0


# ------------------------------------------------------------------------------------------------
# 2. generators and mode classes: ValueError before any device work
def _mode(mode, gen):
    from multinn_amd import modes
    fb = [32, 16] if mode.startswith("feedback") else None
    return modes.MultINN(config(8, TRACKS), params(mode, gen=gen, feedback=fb), mode=mode, device=CPU)


BAD_ANYWHERE = [0.0, -0.5, math.nan, math.inf, (0.5, 1.0), (0.5, 1.0, 2.0, 4.0), (0.5, 0.0, 1.0), (1.0,) * 9]


@pytest.mark.parametrize("mode,gen", [("joint", "NADE"), ("joint", "RBM"), ("jamming", "NADE"), ("jamming", "RBM"), ("composer", "NADE"),
                                      ("composer", "MultiRBM"), ("feedback", "NADE"), ("feedback-rnn", "NADE"), ("feedback", "RBM")])
def test_modes_refuse_bad_temperatures(mode, gen):
    m = _mode(mode, gen)
    for bad in BAD_ANYWHERE:
        with pytest.raises(ValueError):
            m.generate(4, temperature=bad)
        with pytest.raises(ValueError):
            m.sampler(1, temperature=bad)
    rbm = gen in ("RBM", "MultiRBM")
    if rbm:                                                     # an RBM has no threshold mode
        with pytest.raises(ValueError, match="RBM"):
            m.generate(4, temperature=None)
    else:
        assert m._temperature(None) is None
    if mode == "joint" and rbm:                                 # hidden units belong to no track
        with pytest.raises(ValueError):
            m.generate(4, temperature=(0.5, 1.0, 2.0))
        assert m._temperature(2.0) == 2.0
    else:
        assert m._temperature((0.5, 1.0, 2.0)) == (0.5, 1.0, 2.0)
    assert m._temperature((1.0, 1.0, 1.0)) == 1.0 if not (mode == "joint" and rbm) else True
    assert m._temperature(1) == 1.0


def test_generators_refuse_bad_temperatures():
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM, RnnMultiRBM
    x = torch.zeros((2, 3, 12), dtype=torch.uint8)
    nade = RnnNade(12, 8, [32], device=CPU)
    multi = RnnMultiNADE(4, 8, [32], tracks=list("abc"), device=CPU)
    rbm = RnnRBM(12, 8, [32], device=CPU)
    mrbm = RnnMultiRBM(4, 8, [32], tracks=list("abc"), device=CPU)
    for g in (nade, multi, rbm, mrbm):
        for bad in (0.0, -1.0, math.nan, math.inf, (1.0,) * 9, (0.5, 0.0, 2.0)):
            with pytest.raises(ValueError):
                g.generate(x, 2, temperature=bad)
    for g in (multi, mrbm):
        assert g._temperature((0.5, 1.0, 2.0)) == (0.5, 1.0, 2.0) and g._temperature((2.0, 2.0, 2.0)) == 2.0
        with pytest.raises(ValueError):
            g.generate(x, 2, temperature=(0.5, 1.0))
    for g in (rbm, mrbm):
        with pytest.raises(ValueError, match="RBM"):
            g.generate(x, 2, temperature=None)
    with pytest.raises(ValueError):
        rbm.generate(x, 2, temperature=(0.5, 1.0, 2.0))       # one RBM: its hidden units belong to no track
    # one NADE: visible i at temperature[i % n], n dividing the visibles
    assert nade._temperature((0.5, 1.0, 2.0)) == (0.5, 1.0, 2.0) and nade._temperature(None) is None and multi._temperature(None) is None
    with pytest.raises(ValueError):
        nade.generate(x, 2, temperature=(0.5, 1.0, 2.0, 1.0, 3.0))


# ------------------------------------------------------------------------------------------------
# 3. the C ABI: additions only, no version bump
def _header_decl(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
    return None if m is None else re.sub(r"\s+", " ", m.group(1))


def test_new_symbols_in_header_loader_and_library():
    from multinn_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert _header_decl(header, s) is not None, s
        assert s in _lib.SIGNATURES, s
    assert re.search(r"#define\s+MNN_ABI_VERSION\s+124\b", header) and _lib.ABI_VERSION == 124
    lib = _lib.load()
    assert lib.mnn_version() == 124
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    exported = set(re.findall(r"\bT (mnn_[a-z0-9_]+)", out))
    assert set(NEW_SYMBOLS) <= exported
    # the struct: declared, and bound with the same layout
    assert re.search(r"typedef struct \{\s*int n;\s*int by_visible;\s*float t\[MNN_TEMPS_MAX\];\s*\} mnn_temps;", header)
    assert re.search(r"#define\s+MNN_TEMPS_MAX\s+8\b", header) and _lib.TEMPS_MAX == 8
    import ctypes as C
    assert C.sizeof(_lib.Temps) == 40 and _lib.Temps.t.offset == 8 and _lib.Temps.by_visible.offset == 4


def test_existing_signatures_are_unchanged_and_the_new_ones_differ_only_in_the_temperature():
    from multinn_amd import _lib
    header = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    S = _lib.SIGNATURES
    for old, new, was, now in (("mnn_nade_sample", "mnn_nade_sample_temps", "float temperature", "const mnn_temps* temps"),
                               ("mnn_nade_sample_multi", "mnn_nade_sample_multi_temps", "float temperature", "const mnn_temps* temps"),
                               ("mnn_generate_scan_state", "mnn_generate_scan_temps", "float temperature", "const mnn_temps* temps")):
        a, b = _header_decl(header, old), _header_decl(header, new)
        assert was in a and a.replace(was, now) == b, (old, new)
        assert len(S[old][1]) == len(S[new][1])
    a, b = _header_decl(header, "mnn_rbm_gibbs"), _header_decl(header, "mnn_rbm_gibbs_temp")
    assert b == a + ", float temperature" and len(S["mnn_rbm_gibbs_temp"][1]) == len(S["mnn_rbm_gibbs"][1]) + 1
    a, b = _header_decl(header, "mnn_rbm_gibbs_multi"), _header_decl(header, "mnn_rbm_gibbs_multi_temps")
    assert b == a + ", const float* temps" and len(S["mnn_rbm_gibbs_multi_temps"][1]) == len(S["mnn_rbm_gibbs_multi"][1]) + 1
    # the entry points the existing tests call keep the argument lists they bind
    assert len(S["mnn_nade_sample"][1]) == 19 and len(S["mnn_nade_sample_multi"][1]) == 11 and len(S["mnn_generate_scan"][1]) == 23
    assert len(S["mnn_generate_scan_state"][1]) == 25 and len(S["mnn_rbm_gibbs"][1]) == 20 and len(S["mnn_rbm_gibbs_multi"][1]) == 17


def test_library_validates_temperatures_on_the_host(lib):
    """Null device pointers throughout: the temperature checks of the new entry points answer before anything else could."""
    import ctypes as C
    from multinn_amd import _lib
    t = _lib.Temps()
    t.n, t.by_visible = 9, 0
    one = C.c_void_p(16)
    rc = lib.mnn_nade_sample_temps(None, 1, 4, 8, 16, one, 32, one, one, C.byref(t), 1, 0, 0, one, 8, 8, 1, None, None)
    assert rc == -1 and b"temps" in lib.mnn_last_error()
    t.n = 2
    t.t[0], t.t[1] = 1.0, -1.0
    rc = lib.mnn_nade_sample_temps(None, 2, 4, 8, 16, one, 64, one, one, C.byref(t), 1, 0, 0, one, 8, 16, 1, None, None)
    assert rc == -1 and b"temps" in lib.mnn_last_error()
    t.t[1] = 2.0                                                # two temperatures per track, three tracks
    rc = lib.mnn_nade_sample_temps(None, 3, 4, 8, 16, one, 96, one, one, C.byref(t), 1, 0, 0, one, 8, 24, 1, None, None)
    assert rc == -1 and b"temps" in lib.mnn_last_error()
    for bad in (0.0, -1.0, math.inf, math.nan):
        rc = lib.mnn_rbm_gibbs_temp(None, 4, 8, 16, 1, one, one, one, 0, one, 0, 1, 0, None, 0, None, None, one, None, 0, bad)
        assert rc == -1 and b"temperature" in lib.mnn_last_error(), bad


# ------------------------------------------------------------------------------------------------
# 4. the ops wrappers
def test_ops_wrappers_refuse_bad_temperatures_before_any_device_work():
    """Host tensors throughout: a wrapper that reached the device would raise MnnError (no CPU path), not ValueError."""
    from multinn_amd import ops
    N, D, Hn = 4, 6, 8
    bias = torch.zeros((N, 2 * (Hn + D)))
    w = torch.zeros((2, D, Hn))
    out = torch.zeros((N, 2 * D), dtype=torch.uint8)
    for bad in ((0.5, 1.0, 2.0), (0.5, -1.0), (1.0,) * 9, (), (0.5, math.nan)):
        with pytest.raises(ValueError):
            ops.nade_sample(bias, w, w, 2, D, Hn, bad, 1, 0, 0, out)
    job = dict(v0=torch.zeros((N, D), dtype=torch.uint8), W=torch.zeros((D, Hn)), bh=torch.zeros((N, Hn)), bv=torch.zeros((N, D)), seed=1,
               p_v=torch.zeros((N, D)), v_out=torch.zeros((N, D), dtype=torch.uint8))
    for bad in (0.0, -1.0, math.nan, math.inf, None, (0.5, 1.0, 2.0), (0.5, 0.0)):
        with pytest.raises(ValueError):
            ops.rbm_gibbs_multi([job, dict(job)], 2, temperature=bad)
    for bad in (0.0, -1.0, math.nan, math.inf, None, (0.5, 1.0)):
        with pytest.raises(ValueError):
            ops.rbm_gibbs(job["v0"], job["W"], job["bh"], job["bv"], 2, 1, temperature=bad)
    step = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="seed_step"):          # training's stepped chain stays untempered
        ops.rbm_gibbs(job["v0"], job["W"], job["bh"], job["bv"], 2, 1, seed_step=step, temperature=2.0)
    with pytest.raises(ValueError, match="seed_step"):
        ops.rbm_gibbs_multi([job, dict(job)], 2, seed_step=step, temperature=(1.0, 2.0))


def test_ops_wrappers_pick_the_entry_point_by_the_temperature(monkeypatch):
    """The wrappers' argument building with the device taken away (pointers, stream and the call itself replaced): a float or None goes to
    the entry point that always took it -- the T = 1 path is today's call --, a sequence to the one that takes the table."""
    import ctypes as C
    from multinn_amd import ops, _lib
    calls = []
    monkeypatch.setattr(ops, "_ptr", lambda t: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "call", lambda name, *args: calls.append((name, args)))

    def table(arg):
        t = C.cast(arg, C.POINTER(_lib.Temps)).contents
        return t.n, t.by_visible, tuple(round(t.t[i], 6) for i in range(t.n))

    B, Ti, tracks, D, Hn, u, steps = 2, 3, 3, 4, 8, 32, 5
    intro = torch.zeros((B, Ti, tracks * D), dtype=torch.uint8)
    layers = [(torch.zeros((tracks * D + u, 4 * u)), torch.zeros(4 * u))]
    w = torch.zeros((tracks, D, Hn))
    scan = lambda t, **kw: ops.generate_scan(intro, steps, layers, torch.zeros((u, tracks * (Hn + D))), None, tracks, D, Hn, w, w, t, 1, 0, **kw)
    state0 = [(torch.zeros((B, u)), torch.zeros((B, u)))]
    for t, name, want in ((1.0, "mnn_generate_scan", 1.0), (None, "mnn_generate_scan", -1.0), (0.8, "mnn_generate_scan", 0.8)):
        calls.clear()
        assert tuple(scan(t).shape) == (B, steps, tracks * D)
        assert calls[0][0] == name and len(calls[0][1]) == 23 and abs(calls[0][1][16] - want) < 1e-6
        calls.clear()
        scan(t, state0=state0)
        assert calls[0][0] == "mnn_generate_scan_state" and len(calls[0][1]) == 25
    for kw in ({}, {"state0": state0}):
        calls.clear()
        scan((0.5, 1.0, 2.0), **kw)
        assert calls[0][0] == "mnn_generate_scan_temps" and len(calls[0][1]) == 25
        assert table(calls[0][1][16]) == (3, 0, (0.5, 1.0, 2.0))
        assert (calls[0][1][23] is None) == (not kw)
    # one NADE, by visible index
    calls.clear()
    w1 = torch.zeros((1, 12, Hn))
    ops.generate_scan(torch.zeros((B, Ti, 12), dtype=torch.uint8), steps, [(torch.zeros((12 + u, 4 * u)), torch.zeros(4 * u))],
                      torch.zeros((u, Hn + 12)), None, 1, 12, Hn, w1, w1, (0.5, 2.0, 4.0), 1, 0, by_visible=True)
    assert calls[0][0] == "mnn_generate_scan_temps" and table(calls[0][1][16]) == (3, 1, (0.5, 2.0, 4.0))
    # the single sampling step
    bias = torch.zeros((B, tracks * (Hn + D)))
    out = torch.zeros((B, tracks * D), dtype=torch.uint8)
    for t, name in ((1.0, "mnn_nade_sample"), (None, "mnn_nade_sample"), (0.7, "mnn_nade_sample"), ((0.5, 1.0, 2.0), "mnn_nade_sample_temps")):
        calls.clear()
        ops.nade_sample(bias, w, w, tracks, D, Hn, t, 1, 0, 0, out)
        assert calls[0][0] == name and len(calls[0][1]) == 19
    jobs = [dict(bias=torch.zeros((B, Hn + D)), w_enc=w[0], w_dec=w[0], seed=i, samples=torch.zeros((B, D), dtype=torch.uint8)) for i in range(3)]
    for t, name in ((1.0, "mnn_nade_sample_multi"), (None, "mnn_nade_sample_multi"), ((0.5, 1.0, 2.0), "mnn_nade_sample_multi_temps")):
        calls.clear()
        ops.nade_sample_multi(jobs, D, Hn, t, 0, 0)
        assert calls[0][0] == name and len(calls[0][1]) == 11
    # the Gibbs chain
    monkeypatch.setattr(ops, "rbm_workspace", lambda D, Hn, device: None)
    v0, W, bh, bv = torch.zeros((B, D), dtype=torch.uint8), torch.zeros((D, Hn)), torch.zeros((B, Hn)), torch.zeros((B, D))
    for t, name, n in ((1.0, "mnn_rbm_gibbs", 20), (1, "mnn_rbm_gibbs", 20), (2.0, "mnn_rbm_gibbs_temp", 21)):
        calls.clear()
        ops.rbm_gibbs(v0, W, bh, bv, 2, 1, temperature=t)
        assert calls[0][0] == name and len(calls[0][1]) == n
    rj = [dict(v0=v0, W=W, bh=bh, bv=bv, seed=i) for i in range(3)]
    for t, name, n in ((1.0, "mnn_rbm_gibbs_multi", 17), ((1.0, 1.0, 1.0), "mnn_rbm_gibbs_multi", 17), (2.0, "mnn_rbm_gibbs_multi_temps", 18),
                       ((0.5, 1.0, 2.0), "mnn_rbm_gibbs_multi_temps", 18)):
        calls.clear()
        ops.rbm_gibbs_multi(rj, 2, temperature=t)
        assert calls[0][0] == name and len(calls[0][1]) == n
    assert list(calls[0][1][17]) == [0.5, 1.0, 2.0]
