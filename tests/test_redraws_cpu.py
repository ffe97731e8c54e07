"""The polyphony cap by rejection without a device: the normalisation and every refusal (before any device work), the scan-graph keys at
redraws = 0, the session property, and the reference sampler's own properties -- redraw_reference is what the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest
import torch

import redraw_reference as RR

CPU = torch.device("cpu")
FREE = 255


def test_normalisation_and_refusals():
    from multinn_amd.common import sampling_redraws, redraws_key, MAX_REDRAWS
    assert MAX_REDRAWS == 255
    assert sampling_redraws(0, 1, 1.0) == 0 and sampling_redraws(255, (1, None), 0.7) == 255 and sampling_redraws(np.int64(4), 2, (1.0, 0.5)) == 4
    assert sampling_redraws(7, None, 1.0) == 0, "nothing to violate: the call without redraws"
    assert sampling_redraws(0, 1, None) == 0, "threshold decoding without redraws stays"
    for bad in (True, False, 1.0, 2.5, "3", None, -1, 256, (1,)):
        with pytest.raises(ValueError):
            sampling_redraws(bad, 1, 1.0)
    with pytest.raises(ValueError):
        sampling_redraws(1, 1, None)
    assert redraws_key(0) == () and redraws_key(3) == (("redraws", 3),)


def test_generate_refuses_before_device_work_and_rbm_refusals_come_first():
    from multinn_amd import RnnNade, RnnRBM
    from multinn_amd._lib import MnnUnsupported
    nade = RnnNade(12, 8, [32], device=CPU, seed=1)
    x = torch.zeros((2, 3, 12), dtype=torch.uint8)
    for bad in (True, 1.5, -1, 256):
        with pytest.raises(ValueError):
            nade.generate(x, 2, max_notes=1, redraws=bad)
    with pytest.raises(ValueError):
        nade.generate(x, 2, max_notes=1, redraws=2, temperature=None)
    with pytest.raises(ValueError):                                 # max_notes is checked first, as before
        nade.generate(x, 2, max_notes=-1, redraws=2)
    rbm = RnnRBM(12, 8, [32], device=CPU, seed=1)
    with pytest.raises(MnnUnsupported):                             # the RBM's refusal of max_notes, not a complaint about redraws
        rbm.generate(x, 2, max_notes=1, redraws=True)
    assert nade.redraw_counts() == (0, 0)


def test_signatures():
    import inspect
    from multinn_amd import RnnNade, RnnMultiNADE, ops
    from multinn_amd.modes import MultINNCore
    from multinn_amd.feedback import FeedbackRnnSampler
    for f in (RnnNade.generate, RnnMultiNADE.generate, MultINNCore.generate, MultINNCore.sampler, FeedbackRnnSampler.generate,
              FeedbackRnnSampler.generate_encoded, ops.nade_sample, ops.nade_sample_multi, ops.generate_scan, ops.generate_scan_chunk):
        assert inspect.signature(f).parameters["redraws"].default == 0, f
    for f in (ops.nade_sample, ops.nade_sample_multi, ops.generate_scan, ops.generate_scan_chunk):
        assert inspect.signature(f).parameters["redraw_stats"].default is None, f
    for cls in (RnnNade, RnnMultiNADE):
        assert "redraws" not in inspect.signature(cls.sample_single).parameters
        ps = inspect.signature(cls.sample_single_redrawn).parameters
        assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("given", "temperature", "at", "max_notes", "redraws", "redraw_stats"))


def test_graph_keys_are_unchanged_without_redraws(monkeypatch):
    """ScanGraphs.generate with a stand-in for the graph cache: the key of redraws = 0 is the key of the call without the argument."""
    from multinn_amd.common import ScanGraphs
    keys = []

    class Owner:
        class _scan_graphs:
            @staticmethod
            def run(key, x, captured, warm, stale, extra=None):
                keys.append(key)
    monkeypatch.setattr(ScanGraphs, "enabled", staticmethod(lambda x: True))
    scan = lambda *a: None
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None, (1, None))
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None, (1, None), 0)
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None, (1, None), 5)
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None, None, 0)
    assert keys[0] == keys[1] == ("k", ("max_notes", (1, None))) and keys[2] == keys[0] + (("redraws", 5),) and keys[3] == ("k",)


def test_the_entry_point_follows_the_redraws(monkeypatch):
    """ops.call recorded with the device taken away: redraws = 0 and caps that are all None launch what they launched before."""
    from multinn_amd import ops, _lib
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    N, D, Hn = 3, 12, 8
    bias, w, out = torch.zeros((N, Hn + D)), torch.zeros((1, D, Hn)), torch.zeros((N, D), dtype=torch.uint8)
    stats = torch.zeros(2, dtype=torch.int32)
    run = lambda **kw: ops.nade_sample(bias, w, w, 1, D, Hn, kw.pop("temperature", 1.0), 7, 3, 5, out, **kw)
    run(max_notes=2)
    run(max_notes=2, redraws=0, redraw_stats=stats)
    run(redraws=4)
    run(max_notes=(None,), redraws=4)
    run(max_notes=2, redraws=4, redraw_stats=stats)
    assert [c[0] for c in calls] == ["mnn_nade_sample_caps_at"] * 2 + ["mnn_nade_sample"] * 2 + ["mnn_nade_sample_redraw_at"]
    assert len(calls[4][1]) == len(calls[0][1]) + 1
    rd = C.cast(calls[4][1][-1], C.POINTER(_lib.Redraw)).contents
    assert rd.tries == 4 and rd.stats == stats.data_ptr()
    for bad in (dict(redraws=True), dict(redraws=256), dict(redraws=-1), dict(redraws=1.0), dict(redraws=2, temperature=None),
                dict(redraws=1, redraw_stats=torch.zeros(2))):
        with pytest.raises(ValueError):
            run(max_notes=2, **bad)
    assert len(calls) == 5, "a refusal launches nothing"


def test_sessions_carry_the_redraws_as_a_checked_property():
    from multinn_amd.session import GeneratorSession, ModeSession
    assert isinstance(GeneratorSession.redraws, property) and isinstance(ModeSession.redraws, property)

    class Stand:
        _redraws = 0
    s = Stand()
    GeneratorSession.redraws.fset(s, 9)
    assert GeneratorSession.redraws.fget(s) == 9
    for bad in (True, -1, 256, 2.0, None):
        with pytest.raises(ValueError):
            GeneratorSession.redraws.fset(s, bad)
    assert s._redraws == 9


# ------------------------------------------------------------------------------------------------
# the reference sampler's own properties
@pytest.mark.parametrize("N,D,Hn,tracks,caps,by_visible", [(40, 24, 32, 1, [1], False), (30, 40, 32, 1, [1, None, 2, 0, 4], True)])
def test_reference_properties(N, D, Hn, tracks, caps, by_visible):
    from oracle import det, philox
    import test_gpu_conditional as TN
    bias, we, wd, codes = RR.sparse_problem(N, D, Hn, tracks, 0)
    counter = np.arange(D) % len(caps) if by_visible else np.zeros(D, int)
    rows = np.arange(100, 100 + N)
    for c in (np.full((N, D), FREE, np.uint8), codes[:, 0]):
        s, p, acc = RR.redraw_reference(bias, we[0], wd[0], tracks, 0, D, Hn, 1.0, 5, rows, 2, c, counter, caps, 3)
        ok = acc != RR.FALLBACK
        assert ok.any() and (acc > 0).any()
        assert not RR.violations(s[ok], c[ok], counter, caps).any(), "an accepted row has no violation"
        given = c != FREE
        assert np.array_equal(s[given], c[given])
        u = philox.uniform_block(5, philox.STREAM_NADE, rows, 2, D)
        s0, p0 = det.nade_sample(bias, we[0], wd[0], tracks, 0, D, Hn, 1.0, TN.clamp_u(u, c))
        first = acc == 0
        assert first.any() and np.array_equal(s[first], s0[first]) and np.array_equal(p[first], p0[first]), "no violation on attempt 0: the uncapped draw"
        assert np.array_equal(first, ~RR.violations(s0, c, counter, caps).any(1))
        # redraws = 0 is the truncating sampler; every attempt reads its own uniforms
        import test_gpu_max_notes as TM
        t0 = RR.redraw_reference(bias, we[0], wd[0], tracks, 0, D, Hn, 1.0, 5, rows, 2, c, counter, caps, 0)
        assert np.array_equal(t0[0], TM.capped_reference(bias, we[0], wd[0], tracks, 0, D, Hn, 1.0, u, c, counter, caps)[0])
    E4 = (D + 3) // 4 * 4
    a1, a2 = RR.attempt_uniforms(5, rows, 2, 0, D, E4, 1), RR.attempt_uniforms(5, rows, 2, 0, D, E4, 2)
    assert np.array_equal(a1, philox.uniform_block(5, RR.STREAM_NADE_REDRAW, rows, 2, D))
    assert np.array_equal(a2, philox.uniform_block(5, RR.STREAM_NADE_REDRAW, rows, 2, E4 + D)[:, E4:])


def test_reference_sampler_meets_the_distribution_statements():
    """What test_gpu_redraws asserts of the device, shown for the reference alone at the chosen seed: with redraws the 9 allowed outcomes lie
    within 5 sigma of N pi, without them (the truncating sampler) some outcome misses by more than 10 sigma."""
    N, D, Hn = RR.DIST_N, RR.DIST_D, RR.DIST_HN
    bias, we, wd = RR.distribution_problem()
    pi = RR.exact_restricted(bias[0], we[0], wd[0])
    assert int((pi > 0).sum()) == 9 and abs(pi.sum() - 1) < 1e-12
    codes = np.full((N, D), FREE, np.uint8)
    args = (bias, we[0], wd[0], 1, 0, D, Hn, 1.0, RR.DIST_SEED, np.arange(RR.DIST_ROW0, RR.DIST_ROW0 + N), RR.DIST_SUB, codes, np.zeros(D, int), [1])
    s, _, acc = RR.redraw_reference(*args, RR.DIST_REDRAWS)
    counts = RR.outcome_counts(s)
    assert np.nanmax(RR.sigma_excess(counts, pi, N)) <= 5.0
    assert counts[pi == 0].sum() == 0 or (acc == RR.FALLBACK).any()
    s0, _, _ = RR.redraw_reference(*args, 0)
    assert np.nanmax(RR.sigma_excess(RR.outcome_counts(s0), pi, N)) > 10.0
