"""Conditional NLL (mnn_rbm_ais_given / mnn_rbm_raise_given, ops.rbm_ais(given=) / ops.rbm_raise_given, estimate_nll(given_mask=),
driver.evaluate(given_mask=)): the parts that need no GPU.  The C ABI's declarations, bindings and host-side refusals, the early refusals of
the ops and of the model API (every one before any device work), the split of a mask over a mode's generators, and that a call without
the new arguments reaches the old entry points."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_header_declares_and_loader_binds_both_entries(lib):
    from multinn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    for name, base in (("mnn_rbm_ais_given", "mnn_rbm_ais"), ("mnn_rbm_raise_given", "mnn_rbm_raise")):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl and decl.group(1).rstrip().endswith("const uint8_t* given, int ld_given"), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[base][1]) + 2
        assert _lib.SIGNATURES[name][1][:-2] == _lib.SIGNATURES[base][1]                # the old entry's arguments, then the two new ones
        assert hasattr(lib, name) and hasattr(lib, base)
    assert _lib.ABI_VERSION == lib.mnn_version() == 124                                 # a pure addition


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_four_clamped_kernels_are_built_and_none_spills_a_vector_register(tmp_path):
    """forward / reverse x matrix-core / streaming; the matrix-core ones on v_mfma_f32_32x32x2_f32."""
    from multinn_amd import build
    out = str(tmp_path / "ais.s")
    subprocess.check_call([HIPCC] + build.flags_for("rbm_ais.hip") + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "rbm_ais.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    spills = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text)}
    kernels = {k: v for k, v in spills.items() if "rbm_given_" in k}
    assert sorted(k.split("rbm_given_")[1].split("_kernel")[0] for k in kernels) == ["ais_mfma", "ais_stream", "raise_mfma", "raise_stream"], kernels
    assert all(v == 0 for v in kernels.values()), kernels
    bodies = {m.group(1): m.group(0) for m in re.finditer(r"\n(_Z\w*rbm_given_(\w+?)_kernel\w*):.*?s_endpgm", text, re.S)}
    mfma = [b for name, b in bodies.items() if "mfma" in name]
    assert len(mfma) == 2 and all("v_mfma_f32_32x32x2_f32" in b for b in mfma)


def _args(entry, **over):
    a = dict(N=2, D=8, Hn=16, S=4, L=10, betas=1, W=1, bh=1, ld_bh=0, bv=1, ld_bv=0, v=1, log_z=1, ws=1, given=1, ld_given=8)
    a.update(over)
    p = lambda x: None if x is None else 16        # any non-null address: nothing may be dereferenced before the checks fail
    data = (p(a["v"]),) if entry == "mnn_rbm_raise_given" else ()
    return (None, a["N"], a["D"], a["Hn"], a["S"], a["L"], p(a["betas"]), p(a["W"]), p(a["bh"]), a["ld_bh"], p(a["bv"]), a["ld_bv"], *data,
            7, 0, None, p(a["log_z"]), None, None, None, p(a["ws"]), p(a["given"]), a["ld_given"])


@pytest.mark.parametrize("entry", ["mnn_rbm_ais_given", "mnn_rbm_raise_given"])
@pytest.mark.parametrize("over,word", [(dict(ld_given=7), b"ld_given"), (dict(ld_given=0), b"ld_given"), (dict(L=1), b"n_betas"),
                                       (dict(betas=None), b"null"), (dict(ld_bv=5), b"leading"), (dict(given=None, ld_given=0, S=0), b"n_chains"),
                                       (dict(D=40000, Hn=40000, ld_given=40000), b"code bytes")])
def test_c_abi_refuses_bad_arguments_without_a_device(lib, entry, over, word):
    rc = getattr(lib, entry)(*_args(entry, **over))
    msg = lib.mnn_last_error()
    assert rc == -1 and word in msg and msg.startswith(entry[:-len("_given")].encode()), (rc, msg)


def test_the_lds_refusal_counts_the_code_bytes(lib):
    """8 chains' f32 states of D + Hn = 5112 units and the reduction's 256 bytes fill the 160 KB exactly: the free call passes the LDS check
    (and meets the next one: 2^28 rows of 8 chain blocks exceed the grid), the clamped one does not -- and says why."""
    shape = dict(D=5096, Hn=16, ld_given=5096, N=1 << 28, S=64)
    assert lib.mnn_rbm_ais_given(*_args("mnn_rbm_ais_given", given=None, **shape)) == -1 and b"grid" in lib.mnn_last_error()
    assert lib.mnn_rbm_ais_given(*_args("mnn_rbm_ais_given", **shape)) == -1
    assert b"LDS" in lib.mnn_last_error() and b"code bytes" in lib.mnn_last_error()


def _operands():
    betas = torch.linspace(0, 1, 5)
    betas[-1] = 1.0
    return torch.zeros(8, 16), torch.zeros(2, 16), torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.uint8), betas


def test_ops_refuse_bad_codes_before_allocating(monkeypatch):
    from multinn_amd import ops, _lib
    W, bh, bv, v, betas = _operands()
    good = torch.full((2, 8), 255, dtype=torch.uint8)

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the checks were through")
    wide = torch.full((2, 16), 255, dtype=torch.uint8)
    monkeypatch.setattr(torch, "empty", no_alloc)
    for bad in (good.float(), good.bool(), good.to(torch.int8), torch.zeros(2, 7, dtype=torch.uint8), torch.zeros(2, 8, 1, dtype=torch.uint8),
                torch.zeros(16, dtype=torch.uint8), torch.zeros(8, 2, dtype=torch.uint8).t(), wide[:, ::2][:, :8], wide[:, :7], [[255] * 8] * 2):
        with pytest.raises(ValueError, match="given u8"):
            ops.rbm_ais(W, bh, bv, betas, 4, 0, given=bad)
        with pytest.raises(ValueError, match="given u8"):
            ops.rbm_raise_given(W, bh, bv, v, bad, betas, 4, 0)
    with pytest.raises(ValueError, match="bias rows"):
        ops.rbm_ais(W, bh, bv, betas, 4, 0, given=torch.zeros(3, 8, dtype=torch.uint8))
    for codes in (good, wide[:, :8]):                                      # a row stride above D is read in place
        with pytest.raises(_lib.MnnError, match="CPU"):                    # no CPU path: host tensors are refused, still before any allocation
            ops.rbm_ais(W, bh, bv, betas, 4, 0, given=codes)
        with pytest.raises(_lib.MnnError, match="CPU"):
            ops.rbm_raise_given(W, bh, bv, v, codes, betas, 4, 0)


def test_calls_without_the_new_arguments_reach_the_old_entry_points(monkeypatch):
    """ops.rbm_ais / rbm_raise (and rbm_raise_given(given=None)) call mnn_rbm_ais / mnn_rbm_raise with the arguments they always passed;
    with codes they call the _given entries with the same arguments and (given, ld_given) behind them."""
    from multinn_amd import ops
    W, bh, bv, v, betas = _operands()
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else id(t))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops._lib, "load", lambda: type("L", (), {"mnn_rbm_ais_workspace_bytes": staticmethod(lambda *a: 256)})())
    wide = torch.full((2, 12), 255, dtype=torch.uint8)
    codes = wide[:, :8]
    ops.rbm_ais(W, bh, bv, betas, 4, 7)
    ops.rbm_ais(W, bh, bv, betas, 4, 7, given=codes)
    ops.rbm_raise(W, bh, bv, v, betas, 4, 7)
    ops.rbm_raise_given(W, bh, bv, v, None, betas, 4, 7)
    ops.rbm_raise_given(W, bh, bv, v, codes, betas, 4, 7)
    assert [c[0] for c in calls] == ["mnn_rbm_ais", "mnn_rbm_ais_given", "mnn_rbm_raise", "mnn_rbm_raise", "mnn_rbm_raise_given"]
    n_ais, n_raise = 20, 21
    assert [len(c[1]) for c in calls] == [n_ais, n_ais + 2, n_raise, n_raise, n_raise + 2]
    assert calls[1][1][-2:] == (id(codes), 12) and calls[4][1][-2:] == (id(codes), 12)
    head = lambda a: a[:12]                                                # stream, sizes, ladder, W, biases and their leading dimensions
    assert head(calls[0][1])[1:6] == head(calls[1][1])[1:6] == (2, 8, 16, 4, 5)


def config(P=8, tracks=("Drums", "Piano")):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 24, "highest": 24 + P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def params(gen="RBM", enc="Pass", mode="jamming"):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": enc, "num_hidden": [8] if enc != "Pass" else None},
            "generator": {"type": gen, "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": [16]}}


def test_generators_refuse_bad_masks_before_any_work():
    from multinn_amd.generators import RnnRBM, RnnNade, RnnMultiRBM
    x = torch.zeros(2, 4, 10, dtype=torch.uint8)
    gens = (RnnRBM(10, 8, [32, 32], device=CPU), RnnNade(10, 8, [32, 32], device=CPU), RnnMultiRBM(5, 8, [32, 32], tracks=["a", "b"], device=CPU))
    for g in gens:
        for bad in (torch.ones(10), torch.ones(10, dtype=torch.uint8), torch.ones(2, 4, 10, dtype=torch.int64)):
            with pytest.raises(ValueError, match="bool"):
                g.estimate_nll(x, given_mask=bad)
        with pytest.raises(ValueError, match="bool"):
            g.estimate_nll(x, given_mask=[True] * 10)
        for bad in (torch.ones(9, dtype=torch.bool), torch.ones(3, 4, 10, dtype=torch.bool), torch.ones(2, 4, 10, 1, dtype=torch.bool)):
            with pytest.raises(ValueError, match="broadcast"):
                g.estimate_nll(x, given_mask=bad)
        assert g.store.theta is None                                        # nothing was materialised


def test_a_partial_mask_on_a_nade_is_unsupported_before_any_work():
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd.generators import RnnNade, RnnMultiNADE
    x = torch.zeros(2, 4, 10, dtype=torch.uint8)
    half = torch.arange(10) < 5
    g = RnnNade(10, 8, [32, 32], device=CPU)
    with pytest.raises(MnnUnsupported, match="not a sum of its conditionals"):
        g.estimate_nll(x, given_mask=half)
    assert g.store.theta is None
    for ok in (torch.zeros(10, dtype=torch.bool), torch.ones(10, dtype=torch.bool)):      # all or nothing passes that check: the next refusal
        with pytest.raises(MnnUnsupported, match="ROCm"):
            g.estimate_nll(x, given_mask=ok)
    m = RnnMultiNADE(5, 8, [32, 32], tracks=["a", "b"], device=CPU)                      # features i * 2 + m
    with pytest.raises(MnnUnsupported, match="not a sum of its conditionals"):
        m.estimate_nll(x, given_mask=half)
    with pytest.raises(MnnUnsupported, match="ROCm"):                                     # track 0 wholly given, track 1 wholly free
        m.estimate_nll(x, given_mask=torch.arange(10) % 2 == 0)


def test_modes_refuse_before_any_work():
    from multinn_amd import MultINN
    from multinn_amd._lib import MnnUnsupported
    x = torch.zeros(2, 4, 8, 2, dtype=torch.uint8)
    track0 = torch.tensor([True, False])
    low = (torch.arange(8) < 4)[:, None].expand(8, 2)
    # the joint NADE: all or nothing
    m = MultINN(config(), params(gen="NADE", mode="joint"), mode="joint", device=CPU)
    for mask in (track0, low):
        with pytest.raises(MnnUnsupported, match=r"ordered p M \+ m.*not a sum of its conditionals"):
            m.estimate_nll(x, given_mask=mask)
    for mask in (torch.tensor([True, True]), torch.tensor([False, False])):
        with pytest.raises(MnnUnsupported, match="ROCm"):
            m.estimate_nll(x, given_mask=mask)
    # one NADE per track: whole tracks pass the mask check (and meet the host-model refusal), a partly given track does not
    for mode, gen in (("jamming", "NADE"), ("feedback", "NADE"), ("composer", "NADE")):
        m = MultINN(config(), params(gen=gen, mode=mode), mode=mode, device=CPU)
        with pytest.raises(MnnUnsupported, match="not a sum of its conditionals"):
            m.estimate_nll(x, given_mask=low)
        with pytest.raises(MnnUnsupported, match="ROCm"):
            m.estimate_nll(x, given_mask=track0)
    # RBM generators take any mask: the host-model refusal is the first thing they meet
    for mode, gen in (("joint", "RBM"), ("jamming", "RBM"), ("composer", "MultiRBM")):
        m = MultINN(config(), params(gen=gen, mode=mode), mode=mode, device=CPU)
        for mask in (track0, low, torch.zeros(2, 4, 8, 2, dtype=torch.bool)):
            with pytest.raises(MnnUnsupported, match="ROCm"):
                m.estimate_nll(x, given_mask=mask, method="both")
        for bad, word in ((torch.ones(2), "bool"), (torch.ones(3, dtype=torch.bool), "broadcast"), (torch.ones(2, 8, dtype=torch.bool), "broadcast"),
                          ([True, False], "bool")):
            with pytest.raises(ValueError, match=word):
                m.estimate_nll(x, given_mask=bad)
    # DBN encoders stay refused as they are, mask or none
    m = MultINN(config(), params(gen="RBM", enc="DBN", mode="jamming"), mode="jamming", device=CPU)
    with pytest.raises(MnnUnsupported, match="DBN"):
        m.estimate_nll(x, given_mask=track0)


def test_the_mask_is_split_over_the_generators():
    from multinn_amd import MultINN
    codes = torch.arange(2 * 3 * 8 * 2, dtype=torch.int64).reshape(2, 3, 8, 2).to(torch.uint8)
    whole, some = [True, False], [True, True]
    m = MultINN(config(), params(gen="RBM", mode="jamming"), mode="jamming", device=CPU)
    parts = m._nll_given_split(whole, some)
    assert [(w, s) for _, w, s in parts] == [([True], [True]), ([False], [True])]
    assert all(torch.equal(take(codes), codes[..., i]) and take(codes).is_contiguous() for i, (take, _, _) in enumerate(parts))
    m = MultINN(config(), params(gen="MultiRBM", mode="composer"), mode="composer", device=CPU)
    (take, w, s), = m._nll_given_split(whole, some)
    assert (w, s) == (whole, some) and torch.equal(take(codes), codes.reshape(2, 3, 16))
    m = MultINN(config(), params(gen="RBM", mode="joint"), mode="joint", device=CPU)
    (take, w, s), = m._nll_given_split(whole, some)
    assert (w, s) == ([False], [True]) and torch.equal(take(codes), codes.reshape(2, 3, 16))


def test_given_mask_tracks_views_the_features_by_track():
    from multinn_amd.common import given_mask_tracks
    even = torch.arange(10) % 2 == 0
    mask4, shape4, whole, some = given_mask_tracks(even, (2, 4, 10), 2)
    assert shape4 == (2, 4, 5, 2) and tuple(mask4.shape) == shape4 and (whole, some) == ([True, False], [True, False])
    assert bool(mask4[..., 0].all()) and not bool(mask4[..., 1].any())
    _, shape4, whole, some = given_mask_tracks(even, (2, 4, 10), 1)
    assert shape4 == (2, 4, 10, 1) and (whole, some) == ([False], [True])
    _, shape4, whole, some = given_mask_tracks(torch.tensor([True, False]), (2, 4, 5, 2), 1)       # a joint generator fed [B, T, P, M]
    assert shape4 == (2, 4, 10, 1) and (whole, some) == ([False], [True])
    m, shape4, whole, some = given_mask_tracks(torch.tensor([True, False]), (2, 4, 5, 2), 2)
    assert shape4 == (2, 4, 5, 2) and tuple(m.shape) == (2,) and (whole, some) == ([True, False], [True, False])


def test_driver_evaluate_refuses_a_bad_mask_before_any_work():
    from multinn_amd import driver
    X, lengths = np.zeros((2, 4, 8, 2), np.uint8), np.array([4, 4])
    with pytest.raises(ValueError, match="given_mask needs nll"):
        driver.evaluate(object(), X, lengths, 2, 4, given_mask=[True, False])
    for bad in ([1, 0], np.ones((2, 4, 8, 2), bool), True):
        with pytest.raises(ValueError, match="batch-independent bool"):
            driver.evaluate(object(), X, lengths, 2, 4, nll="bracket", given_mask=bad)


def test_model_api_signatures():
    from multinn_amd.common import RBM
    from multinn_amd.generators import RnnRBM, RnnNade, RnnMultiRBM, rbm_nll_side
    from multinn_amd.modes import MultINNCore
    from multinn_amd import ops, driver
    for f in (ops.rbm_ais, RBM.log_partition, RBM.log_partition_reverse, rbm_nll_side, RnnRBM._nll_rows_built, RnnNade._nll_rows_built,
              RnnMultiRBM._nll_rows_built):
        assert inspect.signature(f).parameters["given"].default is None, f
    assert list(inspect.signature(ops.rbm_raise_given).parameters)[:5] == ["W", "bh", "bv", "v", "given"]
    for f in (RnnRBM.estimate_nll, RnnNade.estimate_nll, RnnMultiRBM.estimate_nll, MultINNCore.estimate_nll, driver.evaluate):
        assert inspect.signature(f).parameters["given_mask"].default is None, f
