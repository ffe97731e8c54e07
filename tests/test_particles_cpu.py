"""NADE importance resampling without a device: the normalisation (common.sampling_particles) and every refusal, all before any device
work; the C-ABI additions; the scan-graph key and the session property; and the algorithm itself on tests/nade_sir_reference.py -- the
statistical pin (the resampled frequency meets a bound that the clamped scan misses by far), the short cut, the nesting of particle sets, the
counters under chunking, and that the seeds of tests/test_gpu_particles.py leave no scan out of the pick comparison."""
import os
import re

import numpy as np
import pytest
import torch

import nade_sir_reference as REF
from test_max_notes_cpu import _mode

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE = REF.FREE
# what tests/test_gpu_particles.py runs: (N, D, Hn, tracks) x C, the Philox key and the counters (the sub-counter is SUB + the device cell)
SHAPES = [(3, 61, 30, 2),                # idle lanes, E4 = 124 != tracks D
          (4, 7, 256, 2),                # D under one Philox block
          (5, 333, 256, 3),              # element offsets off a block boundary
          (72, 440, 256, 1)]             # the joint shape
CS = [2, 5, 65]                          # 5: no multiple of a workgroup's four particles; 65: more than one pass of a 64-lane loop
NINE = (3, 13, 32, 9)                    # more tracks than a temperature table has entries: a scalar temperature is entry 0 for all of them
C_SHARED = 65                            # a larger C extends a smaller one's particles: the reference computes them once
SEED, ROW0, SUB, SUB_CELL = 77, 1000, 5, 3
TOY_SEED = 11
NEW_SYMBOLS = ("mnn_nade_sample_sir_workspace_bytes", "mnn_nade_sample_sir_at", "mnn_generate_scan_sir", "mnn_generate_scan_chunk_sir")


# ------------------------------------------------------------------------------------------------
# 1. the normalisation and the refusals
def test_normalisation():
    from multinn_amd.common import sampling_particles as sp, particles_key, MAX_PARTICLES
    from multinn_amd._lib import MnnUnsupported, PARTICLES_MAX
    assert MAX_PARTICLES == PARTICLES_MAX == 1024
    assert sp(None) == 0 and sp(0) == 0 and sp(1) == 0 and sp(2) == 2 and sp(np.int64(64)) == 64 and sp(1024) == 1024
    assert isinstance(sp(np.int64(64)), int)
    assert sp(8, given=None) == 0 and sp(8, given=False) == 0, "nothing given: the call without particles"
    assert sp(8, temperature=0.7) == 8 and sp(8, temperature=(0.5, 1.0)) == 8
    assert sp(1, temperature=None) == 0 and sp(0, max_notes=2) == 0, "without particles nothing is refused"
    for bad in (True, False, 1.0, 2.5, "3", -1, 1025, (2,)):
        with pytest.raises(ValueError):
            sp(bad)
    with pytest.raises(ValueError, match="temperature"):
        sp(2, temperature=None)
    with pytest.raises(MnnUnsupported, match="max_notes"):
        sp(2, max_notes=1)
    with pytest.raises(ValueError):                                  # the value is checked before what it is combined with
        sp(1025, max_notes=1)
    assert particles_key(0) == () and particles_key(16) == (("particles", 16),)


def test_generators_refuse_before_device_work():
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM
    from multinn_amd._lib import MnnUnsupported
    x = torch.zeros((2, 3, 12), dtype=torch.uint8)
    codes = torch.full((2, 2, 12), FREE, dtype=torch.uint8)
    for g in (RnnNade(12, 8, [32], device=CPU, seed=1), RnnMultiNADE(4, 8, [32], tracks=list("abc"), device=CPU, seed=1)):
        for bad in (True, 1.5, -1, 1025):
            with pytest.raises(ValueError):
                g.generate(x, 2, particles=bad)
            with pytest.raises(ValueError):
                g.generate(x, 2, given=codes, particles=bad)
        with pytest.raises(ValueError, match="temperature"):
            g.generate(x, 2, given=codes, particles=4, temperature=None)
        with pytest.raises(MnnUnsupported, match="max_notes"):
            g.generate(x, 2, given=codes, particles=4, max_notes=1)
        with pytest.raises(MnnUnsupported, match="not a ROCm device"):  # a host model, behind the argument's own checks
            g.generate(x, 2, given=codes, particles=4)
        assert g._particles(4, 1.0, None, None) == 0 and g._particles(1, None, 1, codes) == 0 and g._particles(4, 1.0, None, codes) == 4
        assert g.particle_ess() is None and g.particle_picks() is None
    rbm = RnnRBM(12, 8, [32], device=CPU, seed=1)
    assert rbm._particles(4, 1.0, None, codes) == 0 and rbm._particles("x", None, 3, codes) == 0, "RBM generators ignore the argument"


@pytest.mark.parametrize("mode", ["joint", "jamming", "composer"])
def test_modes_check_particles(mode):
    from multinn_amd._lib import MnnUnsupported
    m = _mode(mode, "NADE")
    for bad in (True, 1.5, -1, 1025):
        with pytest.raises(ValueError):
            m.generate(4, particles=bad)
        with pytest.raises(ValueError):
            m.sampler(1, particles=bad)
    cond = object()
    assert m._particles(None, 1.0, None, cond) == 0 and m._particles(1, 1.0, None, cond) == 0 and m._particles(16, 1.0, None, cond) == 16
    assert m._particles(16, 1.0, None, None) == 0, "given=None with any particles is the call without them"
    with pytest.raises(ValueError, match="temperature"):
        m._particles(16, None, None, cond)
    with pytest.raises(MnnUnsupported, match="max_notes"):
        m._particles(16, 1.0, (1, None, 2), cond)
    rbm = _mode(mode, "MultiRBM" if mode == "composer" else "RBM")
    assert rbm._particles(16, 1.0, None, cond) == 0 and rbm._particles(True, 1.0, None, cond) == 0, "RBM generators ignore the argument"


@pytest.mark.parametrize("mode", ["feedback", "feedback-rnn"])
def test_feedback_modes_have_no_particle_form(mode, monkeypatch):
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd.feedback import FeedbackRnnSampler
    from multinn_amd.common import refuse_particles
    m = _mode(mode, "NADE")
    for bad in (True, 1.5, 1025):
        with pytest.raises(ValueError):
            m.generate(4, particles=bad)
    monkeypatch.setattr(type(m._model), "_given", lambda self, n, g, gm: (g, None, None))      # (a host model refuses `given` itself, first)
    with pytest.raises(MnnUnsupported, match="particle form"):
        m.generate(4, given=torch.zeros((2, 4, 8, 3), dtype=torch.uint8), particles=4)
    smp = FeedbackRnnSampler.__new__(FeedbackRnnSampler)
    with pytest.raises(MnnUnsupported, match="particle form"):
        FeedbackRnnSampler.generate(smp, torch.zeros((2, 3, 8, 3), dtype=torch.uint8), 4, given=torch.zeros((2, 4, 8, 3), dtype=torch.uint8), particles=4)
    refuse_particles(1, "x"), refuse_particles(None, "x")


def test_signatures_and_session_property():
    import inspect
    from multinn_amd import RnnNade, RnnMultiNADE, ops
    from multinn_amd.modes import MultINNCore
    from multinn_amd.feedback import FeedbackRnnSampler
    from multinn_amd.session import GeneratorSession, ModeSession
    for f in (RnnNade.generate, RnnMultiNADE.generate, MultINNCore.generate, MultINNCore.sampler, FeedbackRnnSampler.generate):
        assert inspect.signature(f).parameters["particles"].default is None, f
    for cls in (RnnNade, RnnMultiNADE):
        assert "particles" not in inspect.signature(cls.sample_single).parameters
        ps = inspect.signature(cls.sample_single_resampled).parameters
        assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("given", "temperature", "at", "particles", "ess", "pick"))
        assert callable(cls.particle_ess) and callable(cls.particle_picks)
    assert callable(ops.nade_sample_sir) and callable(ops.nade_sample_sir_workspace_bytes)
    assert isinstance(GeneratorSession.particles, property) and isinstance(ModeSession.particles, property)

    class Stand:
        _particles = 0
    s = Stand()
    GeneratorSession.particles.fset(s, 9)
    assert GeneratorSession.particles.fget(s) == 9
    GeneratorSession.particles.fset(s, None)
    assert s._particles == 0
    for bad in (True, -1, 1025, 2.0):
        with pytest.raises(ValueError):
            GeneratorSession.particles.fset(s, bad)


def test_graph_keys_are_unchanged_without_particles(monkeypatch):
    from multinn_amd.common import ScanGraphs
    keys, kws = [], []

    class Owner:
        class _scan_graphs:
            @staticmethod
            def run(key, x, captured, warm, stale, extra=None):
                keys.append(key)
    monkeypatch.setattr(ScanGraphs, "enabled", staticmethod(lambda x: True))
    scan = lambda *a, **kw: None
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None)
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None, None, 0, 0)
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None, None, 0, 16)
    assert keys[0] == keys[1] == ("k",) and keys[2] == ("k", ("particles", 16))
    monkeypatch.setattr(ScanGraphs, "enabled", staticmethod(lambda x: False))
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, lambda *a, **kw: kws.append(kw), None, None, 0, 0)
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, lambda *a, **kw: kws.append(kw), None, None, 0, 16)
    assert kws == [{}, {"particles": 16}], "without particles the scan is called as before"


def test_header_declares_the_streams_and_symbols():
    from multinn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    assert re.search(r"MNN_STREAM_NADE_SIR\s*=\s*13\b", hdr) and re.search(r"MNN_STREAM_NADE_SIR_PICK\s*=\s*14\b", hdr)
    assert re.search(r"typedef struct \{ int particles; float\* ess; int32_t\* pick; void\* workspace; size_t workspace_bytes; \} mnn_sir;", hdr)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\(", hdr), sym
        assert sym in _lib.SIGNATURES, sym
    assert len(_lib.SIGNATURES["mnn_nade_sample_sir_at"][1]) == len(_lib.SIGNATURES["mnn_nade_sample_temps_at"][1]) + 2
    assert len(_lib.SIGNATURES["mnn_generate_scan_sir"][1]) == len(_lib.SIGNATURES["mnn_generate_scan_redraw"][1]) + 1
    assert len(_lib.SIGNATURES["mnn_generate_scan_chunk_sir"][1]) == len(_lib.SIGNATURES["mnn_generate_scan_chunk_redraw"][1]) + 1
    assert [n for n, _ in _lib.Sir._fields_] == ["particles", "ess", "pick", "workspace", "workspace_bytes"]
    assert (REF.STREAM_SIR, REF.STREAM_PICK) == (13, 14)


# ------------------------------------------------------------------------------------------------
# 2. the algorithm, on the reference
_toy = {}


def toy_reference():
    """The toy's resampled rows at (TOY_SEED, rows 0 .., sub 0), once per process (tests/test_gpu_particles.py compares the device with it)."""
    if not _toy:
        bias, we, wd, codes = REF.toy_problem()
        _toy.update(REF.resample(bias, we, wd, 1, 0, REF.TOY_D, REF.TOY_HN, codes, REF.TOY_C, TOY_SEED, np.arange(REF.TOY_N), 0))
    return _toy


def test_resampling_meets_the_bound_the_clamped_scan_misses():
    """f = the frequency of v0 = 1 among the emitted rows, p = p(v0 = 1 | v7 = 1) and rho = E_q[w^2] / E_q[w]^2 by enumeration:
    |f - p| <= 4 sqrt(p (1 - p) / N) + 2 rho / C -- four binomial standard errors plus the first-order bias of a self-normalised estimate
    of a [0, 1] function, doubled for the neglected terms.  Particle 0 of every row -- the clamped scan -- misses it."""
    bias, we, wd, codes = REF.toy_problem()
    p, rho = REF.toy_exact(bias, we, wd)
    bound = REF.toy_bound(p, rho)
    ref = toy_reference()
    f, f0 = ref["out"][:, 0].mean(), ref["v"][:, 0, 0].mean()
    print("p", p, "rho", rho, "bound", bound, "resampled", f, "clamped", f0, "mean ESS", ref["ess"].mean())
    assert 0.9 < p < 0.999 and 1.0 < rho < 4.0
    assert abs(f - p) <= bound
    assert abs(f0 - p) > bound, "the clamped scan does not condition v0 on v7"
    assert np.all(ref["out"][:, 7] == 1) and not ref["near"].any()
    assert np.all(ref["ess"] >= 1.0) and np.all(ref["ess"] <= REF.TOY_C)


def _patterns(D=10):
    codes = np.full((6, D), FREE, np.uint8)
    codes[1] = 1                                                     # everything given
    codes[2, :4] = (0, 1, 1, 0)                                      # a given prefix
    codes[3, 6:] = 1                                                 # a given suffix
    codes[4, 3] = 0                                                  # one given cell in the middle
    codes[5, 0], codes[5, 2] = 1, 0                                  # a free cell inside the given head
    return codes


def test_short_cut_patterns_return_particle_zero():
    codes = _patterns()
    assert REF.is_shortcut(codes).tolist() == [True, True, True, False, False, False]
    R = np.random.default_rng(0)
    D, Hn, C = 10, 8, 16
    bias = (R.standard_normal((6, Hn + D)) * .5).astype(np.float32)
    we, wd = (R.standard_normal((1, D, Hn))).astype(np.float32), (R.standard_normal((1, D, Hn))).astype(np.float32)
    rows = np.arange(40, 46)
    ref = REF.resample(bias, we, wd, 1, 0, D, Hn, codes, C, 9, rows, 2)
    sc = ref["shortcut"]
    assert np.all(ref["pick"][sc] == 0) and np.all(ref["ess"][sc] == C) and np.array_equal(ref["out"][sc], ref["v"][sc, 0])
    # ... because the weights of such a scan do not depend on what is drawn: the restatement itself gives ESS = C there
    lw = ref["log_w"][sc]
    assert np.allclose(lw, lw[:, :1], rtol=0, atol=1e-12)
    assert np.allclose(REF.pick_from(lw, np.full(sc.sum(), 0.5))[1], C)
    assert (ref["ess"][~sc] < C).all() and len(set(ref["pick"][~sc].tolist()) | {0}) > 1
    # particle 0 is the clamped scan of the plain sampler: stream 1, element m D + i
    from oracle import det, philox
    s0, _ = det.nade_sample(bias, we[0], wd[0], 1, 0, D, Hn, 1.0, REF.clamp_u(philox.uniform_block(9, philox.STREAM_NADE, rows, 2, D), codes))
    assert np.array_equal(ref["v"][:, 0], s0)


def test_a_larger_C_extends_a_smaller_one_and_counters_do_not_see_the_chunking():
    N, D, Hn, tracks = SHAPES[0]
    bias, we, wd, codes = REF.problem(N, D, Hn, tracks)
    rows = ROW0 + np.arange(N)
    small = REF.particles(bias, we, wd, tracks, 1, D, Hn, codes[1], 4, SEED, rows, 8)
    large = REF.particles(bias, we, wd, tracks, 1, D, Hn, codes[1], 8, SEED, rows, 8)
    for a, b in zip(small, large):
        assert np.array_equal(a, b[:, :4])
    tail = REF.particles(bias, we, wd, tracks, 1, D, Hn, codes[1], 4, SEED, rows, 8, c0=4)
    assert all(np.array_equal(a, b[:, 4:]) for a, b in zip(tail, large))
    # a row's particles do not depend on the rows around it
    one = REF.particles(bias[1:2], we, wd, tracks, 1, D, Hn, codes[1][1:2], 8, SEED, rows[1:2], 8)
    assert all(np.array_equal(a[0], b[1]) for a, b in zip(one, large))
    # a session's chunk draws step st at sub-counter step0 + cell + st: any split of six steps names the same counters, so the same uniforms
    whole = [(0, 0, st) for st in range(6)]
    for split in ((2, 1, 3), (1, 5), (6,)):
        done, subs = 0, []
        for n in split:                                              # captured chunks: step0 = 0 and the cell holds the steps done
            subs += [(0, done, st) for st in range(n)]
            done += n
        assert [sum(t) for t in subs] == [sum(t) for t in whole]
    u_a = REF.uniforms(SEED, rows, SUB + SUB_CELL, tracks, 1, D, 3)
    u_b = REF.uniforms(SEED, rows, SUB_CELL + SUB, tracks, 1, D, 3)
    assert np.array_equal(u_a, u_b) and not np.array_equal(u_a, REF.uniforms(SEED, rows, SUB, tracks, 1, D, 3))
    # particle c >= 1 reads stream 13 at element (c - 1) E4 + m D + i; E4 = 124 here, not tracks D = 122
    from oracle import philox
    assert REF.e4(tracks, D) == 124
    assert np.array_equal(u_a[:, 2], philox.uniform(SEED, 13, rows[:, None], np.uint32(8), np.uint32(124 + D) + np.arange(D, dtype=np.uint32)[None, :]))
    assert np.array_equal(REF.pick_uniform(SEED, rows, 8, 1), philox.uniform(SEED, 14, rows, np.uint32(8), np.uint32(1)).astype(np.float64))


@pytest.mark.parametrize("N,D,Hn,tracks", SHAPES + [NINE])
def test_the_gpu_tests_seeds_leave_no_scan_out(N, D, Hn, tracks):
    """tests/test_gpu_particles.py may leave a scan out of its pick comparison where u total lies within 1e-12 total of a running sum: at its
    seeds the reference leaves out none, for any C it runs, and both kinds of scan occur in every launch."""
    parts, prob, _ = REF.cached_particles(N, D, Hn, tracks, C_SHARED, SEED, ROW0, SUB + SUB_CELL, "one")
    bias, we, wd, codes = prob[:4]
    rows = ROW0 + np.arange(N)
    kinds = []
    for C in CS:
        for m in range(tracks):
            ref = REF.resample(bias, we, wd, tracks, m, D, Hn, codes[m], C, SEED, rows, SUB + SUB_CELL, parts=parts[m])
            assert not ref["near"].any()
            assert np.all(ref["ess"] >= 1 - 1e-9) and np.all(ref["ess"] <= C + 1e-9)
            kinds += ref["shortcut"].tolist()
    assert any(kinds) and not all(kinds)
