"""Ragged prompts without a device: the one normalisation (common.prompt_lengths) with every refusal, the MnnUnsupported refusals of the
paths without a ragged form -- raised before any device work --, the signatures, the scan-graph key, and the three C-ABI additions in the
header, the export list and the loader."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_max_notes_cpu import _mode

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mnn_lstm_step_det_ragged", "mnn_generate_scan_ragged", "mnn_generate_scan_chunk_ragged")


# ------------------------------------------------------------------------------------------------
# 1. the normalisation
def test_prompt_lengths_accepts_host_integers():
    from multinn_amd.common import prompt_lengths as pl
    assert pl(None, 3, 4) is None
    assert pl([1, 4, 2], 3, 4) == (1, 4, 2) and pl((1, 4, 2), 3, 4) == (1, 4, 2)
    assert pl(np.array([1, 4, 2]), 3, 4) == (1, 4, 2) and pl(np.array([1, 4, 2], np.uint8), 3, 4) == (1, 4, 2)
    assert pl(torch.tensor([1, 4, 2]), 3, 4) == (1, 4, 2) and pl(torch.tensor([1, 4, 2], dtype=torch.int32), 3, 4) == (1, 4, 2)
    assert pl([np.int64(1), np.int32(4), 2], 3, 4) == (1, 4, 2)
    got = pl(np.array([1, 4, 2]), 3, 4)
    assert all(type(v) is int for v in got)


def test_every_entry_equal_to_the_intro_is_the_call_without_the_argument():
    from multinn_amd.common import prompt_lengths as pl
    for full in ([4, 4, 4], (4, 4, 4), np.array([4, 4, 4]), torch.tensor([4, 4, 4])):
        assert pl(full, 3, 4) is None
    assert pl([1], 1, 1) is None
    assert pl([4, 4, 3], 3, 4) == (4, 4, 3)


@pytest.mark.parametrize("bad", [[True, 1, 1], [1, False, 2], True, [1.0, 2, 3], [1, 2.5, 3], np.array([1.0, 2.0, 3.0]), torch.tensor([1.0, 2.0, 3.0]),
                                 np.array([True, True, False]), torch.tensor([True, True, False]), ["1", 2, 3], "123", 3, 2.0,
                                 [1, 2], [1, 2, 3, 4], np.array([1, 2]), torch.tensor([1, 2, 3, 4]), np.array([[1, 2, 3]]), torch.tensor([[1], [2], [3]]),
                                 [0, 1, 2], [1, 2, 5], [-1, 2, 3], np.array([1, 2, 0]), torch.tensor([1, 9, 3]), [None, 1, 2]])
def test_prompt_lengths_refusals(bad):
    from multinn_amd.common import prompt_lengths as pl
    with pytest.raises(ValueError):
        pl(bad, 3, 4)


def test_a_device_tensor_is_refused_without_looking_at_it():
    from multinn_amd.common import prompt_lengths as pl
    meta = torch.empty(3, dtype=torch.int64, device="meta")          # a tensor that is not on the host and has no values to read
    with pytest.raises(ValueError, match="synchronise"):
        pl(meta, 3, 4)


# ------------------------------------------------------------------------------------------------
# 2. refusals, before any device work
def _generators():
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM, RnnMultiRBM
    return [RnnNade(12, 8, [32], device=CPU, seed=1), RnnMultiNADE(4, 8, [32], tracks=list("abc"), device=CPU, seed=1),
            RnnRBM(12, 8, [32], k=2, device=CPU, seed=1), RnnMultiRBM(4, 8, [32], tracks=list("abc"), k=2, device=CPU, seed=1)]


def test_generators_check_the_lengths_then_refuse_a_host_model():
    from multinn_amd._lib import MnnError, MnnUnsupported
    x = torch.zeros((2, 3, 12), dtype=torch.uint8)
    for g in _generators():
        for bad in ([True, 1], [1.5, 2], [1], [0, 1], [1, 4], torch.empty(2, dtype=torch.int64, device="meta")):
            with pytest.raises(ValueError):
                g.generate(x, 2, lengths=bad)
            with pytest.raises(ValueError):
                g.ragged_session(x, bad)
            with pytest.raises(ValueError):
                g.steps(x, lengths=bad)
        for call in (lambda: g.generate(x, 2, lengths=[1, 3]), lambda: g.ragged_session(x, [1, 3]), lambda: g.steps(x, lengths=[1, 3])):
            with pytest.raises(MnnUnsupported, match="ROCm device") as e:
                call()
            assert isinstance(e.value, MnnError) and isinstance(e.value, NotImplementedError)
        assert g.store.theta is None                                 # nothing was materialised, let alone launched


def test_the_throughput_recurrences_are_refused(monkeypatch):
    """MULTINN_DET_SAMPLING=0: the intro pass returns only the state behind step Ti."""
    from multinn_amd._lib import MnnUnsupported
    x = torch.zeros((2, 3, 12), dtype=torch.uint8)
    for g in _generators():
        monkeypatch.setattr(g.store, "device", torch.device("cuda:0"))          # (a device model as far as the host checks go: nothing runs)
        monkeypatch.setattr(g, "det_sampling", False)
        for call in (lambda: g.generate(x, 2, lengths=[1, 3]), lambda: g.ragged_session(x, [1, 3]), lambda: g.steps(x, lengths=[1, 3])):
            with pytest.raises(MnnUnsupported, match="MULTINN_DET_SAMPLING"):
                call()
        assert g.store.theta is None


@pytest.mark.parametrize("mode", ["feedback", "feedback-rnn"])
def test_feedback_modes_have_no_ragged_form(mode):
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd.feedback import FeedbackRnnSampler
    m = _mode(mode, "NADE")
    for bad in ([True, 1], [1.5, 2], [0, 1]):
        with pytest.raises(ValueError):
            m.generate(4, intro_lengths=bad)
        with pytest.raises(ValueError):
            m.sampler(1, intro_lengths=bad)
    with pytest.raises(MnnUnsupported, match="feedback module's state"):
        m.generate(4, intro_lengths=[1, 2])
    with pytest.raises(MnnUnsupported, match="feedback module's state"):
        m.sampler(1, intro_lengths=[1, 2])
    with pytest.raises(MnnUnsupported):                              # sessions do not exist for these modes at all
        m.ragged_session([1, 2])
    smp = FeedbackRnnSampler.__new__(FeedbackRnnSampler)
    x = torch.zeros((2, 3, 8, 3), dtype=torch.uint8)
    with pytest.raises(MnnUnsupported, match="feedback module's state"):
        FeedbackRnnSampler.generate(smp, x, 4, lengths=[1, 3])
    with pytest.raises(ValueError):
        FeedbackRnnSampler.generate(smp, x, 4, lengths=[1, 4])


@pytest.mark.parametrize("mode,gen", [("joint", "NADE"), ("jamming", "NADE"), ("composer", "NADE"), ("joint", "RBM"), ("jamming", "RBM"), ("composer", "MultiRBM")])
def test_modes_check_the_lengths_then_refuse_a_host_model(mode, gen):
    from multinn_amd._lib import MnnUnsupported
    m = _mode(mode, gen)
    for bad in ([True, 1], [1.5, 2], [0, 1], "ab"):
        with pytest.raises(ValueError):
            m.generate(4, intro_lengths=bad)
        with pytest.raises(ValueError):
            m.sampler(1, intro_lengths=bad)
    with pytest.raises(MnnUnsupported, match="ROCm device"):
        m.generate(4, intro_lengths=[1, 2])
    with pytest.raises(MnnUnsupported, match="ROCm device"):
        m.sampler(1, intro_lengths=[1, 2])
    with pytest.raises(MnnUnsupported, match="ROCm device"):
        m.ragged_session([1, 2])
    with pytest.raises(ValueError):                                   # the head of the call stays _generate_arguments: its refusals come first
        m.generate(4, temperature=-1.0, intro_lengths=[1, 2])
    assert m._intro_lengths(None) is None


@pytest.mark.parametrize("mode", ["joint", "jamming", "composer"])
def test_dbn_encoders_are_refused(mode):
    from multinn_amd._lib import MnnUnsupported
    m = _mode(mode, "NADE", enc="DBN")
    with pytest.raises(MnnUnsupported, match="DBN encoders"):
        m.generate(4, intro_lengths=[1, 2])
    with pytest.raises(MnnUnsupported, match="DBN encoders"):
        m.ragged_session([1, 2])


def test_a_built_mode_hands_its_generators_the_lengths_plus_the_zero_step(monkeypatch):
    """The generators' encoded intros carry one all-zero step in front of the built x, so prompt lengths 1..T of x are 2..T + 1 there; all T
    is the call without the argument."""
    m = _mode("joint", "NADE")
    monkeypatch.setattr(m, "_x", torch.zeros((2, 3, 8, 3), dtype=torch.uint8))
    monkeypatch.setattr(m, "_refuse_intro_lengths", lambda who: None)
    assert m._intro_lengths([3, 3]) is None
    assert m._intro_lengths([1, 3]) == (2, 4) and m._intro_lengths(np.array([2, 1])) == (3, 2)
    for bad in ([1, 4], [0, 1], [1], [1, 2, 3]):
        with pytest.raises(ValueError):
            m._intro_lengths(bad)


# ------------------------------------------------------------------------------------------------
# 3. the interface
def test_signatures():
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM, RnnMultiRBM, ops, lstm_stack
    from multinn_amd.generators import RnnEstimator
    from multinn_amd.modes import MultINNCore
    from multinn_amd.feedback import FeedbackRnnSampler
    from multinn_amd.common import ScanGraphs
    from multinn_amd.session import GeneratorSession, ModeSession
    for cls in (RnnNade, RnnMultiNADE, RnnRBM, RnnMultiRBM):
        assert cls.generate is RnnEstimator.generate and cls.ragged_session is RnnEstimator.ragged_session and cls.steps is RnnEstimator.steps
    for f in (RnnEstimator.generate, RnnEstimator.steps, FeedbackRnnSampler.generate, ops.lstm_step_det, ops.generate_scan, GeneratorSession.__init__,
              ops.generate_scan_chunk, lstm_stack.det_steps, lstm_stack.LstmStack.det_step, ScanGraphs.generate, ScanGraphs.run):
        assert inspect.signature(f).parameters["lengths"].default is None, f
    for f in (MultINNCore.generate, MultINNCore.sampler, ModeSession.__init__):
        assert inspect.signature(f).parameters["intro_lengths"].default is None, f
    # session() keeps the signature tests/test_session_cpu.py pins; a ragged session has an entry of its own
    assert list(inspect.signature(RnnEstimator.session).parameters) == ["self", "x"] and list(inspect.signature(MultINNCore.session).parameters) == ["self"]
    assert list(inspect.signature(RnnEstimator.ragged_session).parameters) == ["self", "x", "lengths"]
    assert list(inspect.signature(MultINNCore.ragged_session).parameters) == ["self", "intro_lengths"]
    for f in (ops.lstm_step_det, lstm_stack.det_steps, lstm_stack.LstmStack.det_step):
        assert inspect.signature(f).parameters["t"].default == 0, f
    assert list(inspect.signature(RnnEstimator.steps).parameters) == ["self", "inputs", "initial_state", "lengths"]


def test_the_graph_key_gains_lengths_and_nothing_else(monkeypatch):
    from multinn_amd.common import ScanGraphs
    keys, run_kw, scan_kw = [], [], []

    class Owner:
        class _scan_graphs:
            @staticmethod
            def run(key, x, captured, warm, stale, extra=None, **kw):
                keys.append(key)
                run_kw.append(kw)
    monkeypatch.setattr(ScanGraphs, "enabled", staticmethod(lambda x: True))
    scan = lambda *a, **kw: None
    lens = object()
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None)
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, scan, None, lengths=lens)
    ScanGraphs.generate(Owner, ("k",), None, 4, object(), 0.5, scan, None, None, 0, 16)
    ScanGraphs.generate(Owner, ("k",), None, 4, object(), 0.5, scan, None, None, 0, 16, lengths=lens)
    assert keys[0] == ("k",) and keys[1] == ("k", "lengths")
    assert keys[3] == keys[2] + ("lengths",) and "given" in keys[2] and ("particles", 16) in keys[2]
    assert run_kw[0] == {} and run_kw[1] == {"lengths": lens}, "without lengths the graph cache is called as before"
    monkeypatch.setattr(ScanGraphs, "enabled", staticmethod(lambda x: False))
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, lambda *a, **kw: scan_kw.append(kw), None)
    ScanGraphs.generate(Owner, ("k",), None, 4, None, 1.0, lambda *a, **kw: scan_kw.append(kw), None, lengths=lens)
    assert scan_kw == [{}, {"lengths": lens}], "without lengths the scan is called as before"


# ------------------------------------------------------------------------------------------------
# 4. the C ABI
def test_header_export_list_and_loader_hold_the_three_symbols(lib):
    from multinn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "multinn_amd", "libmultinn_hip.so")], text=True)
    exported = set(re.findall(r"\bT (mnn_[a-z0-9_]+)", out))
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\(", hdr), sym
        assert sym in _lib.SIGNATURES and sym in exported, sym
        assert hasattr(lib, sym)
    assert re.search(r"#define MNN_ABI_VERSION 124\b", hdr) and _lib.ABI_VERSION == 124
    assert len(_lib.SIGNATURES["mnn_lstm_step_det_ragged"][1]) == len(_lib.SIGNATURES["mnn_lstm_step_det"][1]) + 2
    assert len(_lib.SIGNATURES["mnn_generate_scan_ragged"][1]) == len(_lib.SIGNATURES["mnn_generate_scan_sir"][1]) + 1
    assert len(_lib.SIGNATURES["mnn_generate_scan_chunk_ragged"][1]) == len(_lib.SIGNATURES["mnn_generate_scan_chunk_sir"][1]) + 1
    assert re.search(r"mnn_lstm_step_det_ragged\([^)]*const int32_t\* lengths, int t\)", hdr)
    for sym in NEW_SYMBOLS[1:]:
        assert re.search(sym + r"\([^)]*const mnn_sir\* sir, const int32_t\* intro_lengths\)", hdr), sym


def test_the_entries_refuse_what_the_issue_lists_on_the_host(lib):
    """lengths == NULL for the step; n_intro == 0 with lengths for the scans: host-side checks that run before anything touches the device."""
    import ctypes as C
    from multinn_amd import _lib
    job = (_lib.DetLstmJob * 1)()
    assert lib.mnn_lstm_step_det_ragged(None, 4, 1, job, None, 0) == -1 and b"lengths" in lib.mnn_last_error()
    some = C.c_void_p(256)                                            # never dereferenced on the host
    for sym in NEW_SYMBOLS[1:]:
        args = [None if t in (C.c_void_p, C.POINTER(C.c_void_p)) else 0 for t in _lib.SIGNATURES[sym][1]]
        args[1], args[2], args[3], args[-1] = 4, 0, 2, some             # B, n_intro == 0, num_steps, intro_lengths
        assert getattr(lib, sym)(*args) == -1 and b"intro_lengths" in lib.mnn_last_error(), sym
