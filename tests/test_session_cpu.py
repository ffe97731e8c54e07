"""Generation sessions without a GPU: the interface on the four generator classes and the three modes that have it, every refusal and every
ValueError before any device work (the models live on the host: anything that reached a kernel would raise MnnError), the C-ABI additions
in header / loader / library, and the ops wrappers' choice of entry point."""
import inspect
import math
import os
import re
import subprocess

import pytest
import torch

from test_modes_cpu import config, params

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKS = ("Drums", "Piano", "Guitar")
# the three new families: a sub-counter base on the NADE sampling launches, on the Gibbs chain (single and grouped), and the scan as a chunk
NEW_SYMBOLS = ("mnn_nade_sample_temps_at", "mnn_rbm_gibbs_at", "mnn_rbm_gibbs_multi_at", "mnn_generate_scan_chunk")


def _generators():
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM, RnnMultiRBM
    return (RnnNade(12, 8, [32], device=CPU), RnnMultiNADE(4, 8, [32], tracks=list("abc"), device=CPU),
            RnnRBM(12, 8, [32], k=4, device=CPU), RnnMultiRBM(4, 8, [32], tracks=list("abc"), k=0, device=CPU))


def _mode(mode, gen, enc="Pass"):
    from multinn_amd import modes
    fb = [32, 16] if mode.startswith("feedback") else None
    return modes.MultINN(config(8, TRACKS), params(mode, enc=enc, enc_hidden=[6] if enc == "DBN" else None, gen=gen, feedback=fb), mode=mode, device=CPU)


# ------------------------------------------------------------------------------------------------
# 1. the interface
def test_the_interface_exists_with_the_documented_signatures():
    import multinn_amd
    from multinn_amd import session, generators, modes
    assert multinn_amd.GeneratorSession is session.GeneratorSession and multinn_amd.ModeSession is session.ModeSession
    assert {"GeneratorSession", "ModeSession"} <= set(multinn_amd.__all__)
    for cls in (generators.RnnNade, generators.RnnMultiNADE, generators.RnnRBM, generators.RnnMultiRBM):
        assert cls.session is generators.RnnEstimator.session
    assert list(inspect.signature(generators.RnnEstimator.session).parameters) == ["self", "x"]
    for cls in (modes.MultINNJoint, modes.MultINNJamming, modes.MultINNComposer):
        assert list(inspect.signature(cls.session).parameters) == ["self"]
    sig = inspect.signature(session.GeneratorSession.generate)
    assert list(sig.parameters) == ["self", "num_steps", "given", "temperature"]
    assert sig.parameters["given"].default is None and sig.parameters["temperature"].default == 1.0
    sig = inspect.signature(session.ModeSession.generate)
    assert list(sig.parameters) == ["self", "num_steps", "given", "given_mask", "temperature"]
    assert sig.parameters["given"].default is None and sig.parameters["given_mask"].default is None and sig.parameters["temperature"].default == 1.0
    for cls in (session.GeneratorSession, session.ModeSession):
        assert callable(cls.snapshot) and callable(cls.restore) and list(inspect.signature(cls.restore).parameters) == ["self", "snap"]
    assert [g.subs_per_step for g in _generators()] == [1, 1, 4, 1]          # max(k, 1) sub-counters per generated step


# ------------------------------------------------------------------------------------------------
# 2. refusals, before any device work
def test_generators_on_the_host_are_refused():
    from multinn_amd._lib import MnnError, MnnUnsupported
    x = torch.zeros((2, 3, 12), dtype=torch.uint8)
    for g in _generators():
        with pytest.raises(MnnUnsupported, match="ROCm device") as e:
            g.session(x)
        assert isinstance(e.value, MnnError) and isinstance(e.value, NotImplementedError)
        assert g.store.theta is None                                 # nothing was materialised, let alone launched
        for bad in (None, torch.zeros((2, 12), dtype=torch.uint8), torch.zeros((2, 0, 12), dtype=torch.uint8)):
            with pytest.raises(ValueError):
                g.session(bad)


@pytest.mark.parametrize("mode,gen", [("joint", "NADE"), ("joint", "RBM"), ("jamming", "NADE"), ("jamming", "RBM"), ("composer", "NADE"),
                                      ("composer", "MultiRBM")])
def test_modes_on_the_host_are_refused(mode, gen):
    from multinn_amd._lib import MnnUnsupported
    with pytest.raises(MnnUnsupported, match="ROCm device"):
        _mode(mode, gen).session()


@pytest.mark.parametrize("mode", ["feedback", "feedback-rnn"])
def test_feedback_modes_are_refused(mode):
    from multinn_amd._lib import MnnUnsupported
    with pytest.raises(MnnUnsupported, match="feedback"):
        _mode(mode, "NADE").session()


@pytest.mark.parametrize("mode", ["joint", "jamming", "composer"])
def test_dbn_encoders_are_refused(mode):
    from multinn_amd._lib import MnnUnsupported
    with pytest.raises(MnnUnsupported, match="DBN"):
        _mode(mode, "NADE", enc="DBN").session()


# ------------------------------------------------------------------------------------------------
# 3. the chunk's arguments
def test_chunk_arguments():
    from multinn_amd.session import _chunk_arguments as chunk_arguments
    nade, multi, rbm, mrbm = _generators()
    codes = torch.full((2, 3, 12), 255, dtype=torch.uint8)
    for g in (nade, multi, rbm, mrbm):
        n, gv, t = chunk_arguments(g, 2, 5, 3, codes, 1)
        assert n == 3 and gv is codes and t == 1.0 and isinstance(t, float)
        assert chunk_arguments(g, 2, 0, 1) == (1, None, 1.0)
        for bad in (0, -1, 2.0, None, True, "4"):
            with pytest.raises(ValueError, match="num_steps"):
                chunk_arguments(g, 2, 0, bad)
        for bad in (codes.float(), codes[:, :2], codes[:1], codes[:, :, :11], torch.zeros((2, 3, 4, 3), dtype=torch.uint8), [[0]]):
            with pytest.raises(ValueError, match="given"):
                chunk_arguments(g, 2, 0, 3, bad)
        for bad in (0.0, -1.0, math.nan, math.inf, (1.0,) * 9, (0.5, 0.0, 2.0), "hot"):
            with pytest.raises(ValueError):
                chunk_arguments(g, 2, 0, 3, None, bad)
    assert chunk_arguments(nade, 2, 0, 3, None, None)[2] is None and chunk_arguments(multi, 2, 0, 3, None, (0.5, 1.0, 2.0))[2] == (0.5, 1.0, 2.0)
    with pytest.raises(ValueError, match="RBM"):
        chunk_arguments(rbm, 2, 0, 3, None, None)
    # 2^32 sub-counters per row: (steps + num_steps) * max(k, 1)
    assert chunk_arguments(nade, 2, (1 << 32) - 3, 3)[0] == 3
    with pytest.raises(ValueError, match="2\\^32"):
        chunk_arguments(nade, 2, (1 << 32) - 3, 4)
    assert chunk_arguments(rbm, 2, (1 << 30) - 3, 3)[0] == 3       # k = 4
    with pytest.raises(ValueError, match="2\\^32"):
        chunk_arguments(rbm, 2, (1 << 30) - 3, 4)
    assert chunk_arguments(mrbm, 2, (1 << 32) - 3, 3)[0] == 3      # k = 0: one sub-counter per step all the same


# ------------------------------------------------------------------------------------------------
# 4. the C ABI: additions only, no version bump
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
    assert _lib.load().mnn_version() == 124
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\bT (mnn_[a-z0-9_]+)", out))
    S = _lib.SIGNATURES
    # each _at entry is the entry it extends plus the pointer; those keep the argument lists they bind
    for old, new in (("mnn_nade_sample_temps", "mnn_nade_sample_temps_at"), ("mnn_rbm_gibbs_temp", "mnn_rbm_gibbs_at"),
                     ("mnn_rbm_gibbs_multi_temps", "mnn_rbm_gibbs_multi_at")):
        assert _header_decl(header, new) == _header_decl(header, old) + ", const uint32_t* sub_base", new
        assert len(S[new][1]) == len(S[old][1]) + 1
    assert len(S["mnn_nade_sample_temps"][1]) == 19 and len(S["mnn_rbm_gibbs_temp"][1]) == 21 and len(S["mnn_rbm_gibbs_multi_temps"][1]) == 18
    a, b = _header_decl(header, "mnn_generate_scan_temps"), _header_decl(header, "mnn_generate_scan_chunk")
    assert b == a.replace("c0, const float* const* h0", "c_in, const float* const* h_in") + \
        ", float* const* c_out, float* const* h_out, uint32_t step0, const uint32_t* step_base"
    assert len(S["mnn_generate_scan_temps"][1]) == 25 and len(S["mnn_generate_scan_chunk"][1]) == 29


def test_library_checks_a_chunk_on_the_host():
    """Null device pointers throughout: the chunk's own requirements answer before anything is enqueued."""
    import ctypes as C
    from multinn_amd import _lib
    lib = _lib.load()
    t = _lib.Temps()
    t.n, t.t[0] = 1, 1.0
    one = C.c_void_p(256)
    lay = (_lib.ScanLstmLayer * 1)()
    lay[0].W, lay[0].bias, lay[0].units = one, one, 32
    ptrs = (C.c_void_p * 1)(256)

    def chunk(n_intro, num_steps, c_in, h_in, c_out=None, h_out=None):
        return lib.mnn_generate_scan_chunk(None, 2, n_intro, num_steps, one, 8, 1, lay, one, None, 24, 1, 8, 16, one, one, C.byref(t), 1, 0, one, None, 0, None,
                                           c_in, h_in, c_out, h_out, 0, None)
    assert chunk(0, 0, ptrs, ptrs) == -1 and b"one of them > 0" in lib.mnn_last_error()
    assert chunk(0, 2, None, None) == -1 and b"continues from c_in" in lib.mnn_last_error()
    assert chunk(0, 2, ptrs, None) == -1 and b"pairs" in lib.mnn_last_error()
    assert chunk(2, 0, None, None, ptrs, None) == -1 and b"pairs" in lib.mnn_last_error()
    assert chunk(-1, 2, ptrs, ptrs) == -1
    assert chunk(0, 2, ptrs, ptrs) == -1 and b"workspace" in lib.mnn_last_error()      # past the chunk's own checks: the scan's next one


# ------------------------------------------------------------------------------------------------
# 5. the ops wrappers
def test_ops_wrappers_take_the_at_entries_only_with_a_step_cell(monkeypatch):
    """The wrappers' argument building with the device taken away: without sub_base the entry points of before, with one the _at entries,
    the cell last."""
    import ctypes as C
    from multinn_amd import ops
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    monkeypatch.setattr(ops, "rbm_workspace", lambda D, Hn, device: torch.zeros(1, dtype=torch.uint8))
    monkeypatch.setattr(ops._lib, "load", lambda: type("L", (), {"mnn_rbm_workspace_bytes": staticmethod(lambda D, Hn: 4)})())
    N, D, Hn = 4, 6, 8
    cell = torch.zeros(1, dtype=torch.int32)
    bias, w, out = torch.zeros((N, Hn + D)), torch.zeros((D, Hn)), torch.zeros((N, D), dtype=torch.uint8)
    for T in (1.0, None, 0.7):
        ops.nade_sample(bias, w, w, 1, D, Hn, T, 1, 0, 3, out)
        ops.nade_sample(bias, w, w, 1, D, Hn, T, 1, 0, 3, out, sub_base=cell)
    assert [c[0] for c in calls] == ["mnn_nade_sample", "mnn_nade_sample_temps_at"] * 3
    assert all(c[1][-1].value == cell.data_ptr() for c in calls[1::2])
    calls.clear()
    v0, bh, bv = torch.zeros((N, D), dtype=torch.uint8), torch.zeros((N, Hn)), torch.zeros((N, D))
    for T in (1.0, 0.7):
        ops.rbm_gibbs(v0, w, bh, bv, 2, 1, temperature=T)
        ops.rbm_gibbs(v0, w, bh, bv, 2, 1, temperature=T, sub_base=cell)
    assert [c[0] for c in calls] == ["mnn_rbm_gibbs", "mnn_rbm_gibbs_at", "mnn_rbm_gibbs_temp", "mnn_rbm_gibbs_at"]
    assert all(c[1][-1].value == cell.data_ptr() for c in calls[1::2])
    calls.clear()
    job = dict(v0=v0, W=w, bh=bh, bv=bv, seed=1, p_v=torch.zeros((N, D)), v_out=torch.zeros((N, D), dtype=torch.uint8))
    for T in (1.0, (0.7, 1.0)):
        ops.rbm_gibbs_multi([job, dict(job)], 2, temperature=T)
        ops.rbm_gibbs_multi([job, dict(job)], 2, temperature=T, sub_base=cell)
    assert [c[0] for c in calls] == ["mnn_rbm_gibbs_multi", "mnn_rbm_gibbs_multi_at", "mnn_rbm_gibbs_multi_temps", "mnn_rbm_gibbs_multi_at"]
    assert calls[1][1][-2] is None and calls[3][1][-2] is not None and all(c[1][-1].value == cell.data_ptr() for c in calls[1::2])
    # the cell: one int32; not with training's stepped chain
    for bad in (torch.zeros(2, dtype=torch.int32), torch.zeros(1), 3):
        with pytest.raises(ValueError, match="sub_base"):
            ops.nade_sample(bias, w, w, 1, D, Hn, 1.0, 1, 0, 3, out, sub_base=bad)
        with pytest.raises(ValueError, match="sub_base"):
            ops.rbm_gibbs(v0, w, bh, bv, 2, 1, sub_base=bad)
    with pytest.raises(ValueError, match="seed_step"):
        ops.rbm_gibbs(v0, w, bh, bv, 2, 1, seed_step=torch.zeros(1, dtype=torch.int32), sub_base=cell)
