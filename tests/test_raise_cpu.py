"""Reverse annealed importance sampling (mnn_rbm_raise, ops.rbm_raise, estimate_nll(method=...), driver.evaluate(nll="raise" | "bracket")):
the parts that need no GPU.  The C ABI's declaration, binding and host-side refusals, the early refusals of the op and of the model API, the
NllBracket arithmetic, and the estimator's algebra in float64 against exact enumeration."""
import inspect
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def test_header_declares_and_loader_binds_the_entry(lib):
    from multinn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    decl = re.search(r"\bint mnn_rbm_raise\(([^;]*)\);", hdr)
    assert decl and "const uint8_t* v," in decl.group(1)
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["mnn_rbm_raise"][1]) == len(_lib.SIGNATURES["mnn_rbm_ais"][1]) + 1
    assert hasattr(lib, "mnn_rbm_raise")
    assert _lib.ABI_VERSION == lib.mnn_version() == 124                   # a pure addition


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_reverse_kernels_are_built_beside_the_forward_ones(tmp_path):
    """Both chain forms have a reverse instantiation, the matrix-core one on v_mfma_f32_32x32x2_f32, and neither spills a vector register."""
    from multinn_amd import build
    out = str(tmp_path / "ais.s")
    subprocess.check_call([HIPCC] + build.flags_for("rbm_ais.hip") + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "rbm_ais.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    spills = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text)}
    kernels = {k: v for k, v in spills.items() if "rbm_raise_" in k}
    assert sorted(k.split("rbm_raise_")[1].split("_kernel")[0] for k in kernels) == ["mfma", "stream"] and all(v == 0 for v in kernels.values()), kernels
    bodies = {m.group(1): m.group(0) for m in re.finditer(r"\n(_Z\w*rbm_raise_(\w+?)_kernel\w*):.*?s_endpgm", text, re.S)}
    mfma = [b for name, b in bodies.items() if "mfma" in name]
    assert len(mfma) == 1 and "v_mfma_f32_32x32x2_f32" in mfma[0]


def _raise_args(**over):
    a = dict(N=2, D=8, Hn=16, S=4, L=10, betas=1, W=1, bh=1, ld_bh=0, bv=1, ld_bv=0, v=1, log_z=1, ws=1)
    a.update(over)
    p = lambda x: None if x is None else 16        # any non-null address: nothing may be dereferenced before the checks fail
    return (None, a["N"], a["D"], a["Hn"], a["S"], a["L"], p(a["betas"]), p(a["W"]), p(a["bh"]), a["ld_bh"], p(a["bv"]), a["ld_bv"], p(a["v"]),
            7, 0, None, p(a["log_z"]), None, None, None, p(a["ws"]))


@pytest.mark.parametrize("over,word", [(dict(L=1), b"n_betas"), (dict(S=0), b"n_chains"), (dict(N=0), b"sizes"), (dict(Hn=-1), b"sizes"),
                                       (dict(S=1 << 22, L=1 << 10), b"32-bit"), (dict(betas=None), b"null"), (dict(ws=None), b"null"),
                                       (dict(log_z=None), b"null"), (dict(v=None), b"null"), (dict(ld_bh=3), b"leading"),
                                       (dict(ld_bv=5), b"leading"), (dict(D=40000, Hn=40000), b"LDS")])
def test_c_abi_refuses_bad_arguments_without_a_device(lib, over, word):
    rc = lib.mnn_rbm_raise(*_raise_args(**over))
    msg = lib.mnn_last_error()
    assert rc == -1 and word in msg and msg.startswith(b"mnn_rbm_raise"), (rc, msg)


def _operands():
    betas = torch.linspace(0, 1, 5)
    betas[-1] = 1.0
    return torch.zeros(8, 16), torch.zeros(2, 16), torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.uint8), betas


@pytest.mark.parametrize("betas,word", [([0.0], "two"), ([0.0, 0.5, 0.4, 1.0], "non-decreasing"), ([0.1, 1.0], "start at 0"),
                                        ([0.0, 0.9], "end at 1"), ([0.0, float("nan"), 1.0], "finite")])
def test_ops_refuses_bad_ladders(betas, word):
    from multinn_amd import ops
    W, bh, bv, v, _ = _operands()
    with pytest.raises(ValueError, match="rbm_raise.*" + word):
        ops.rbm_raise(W, bh, bv, v, torch.tensor(betas, dtype=torch.float32), 4, 0)


def test_ops_refuses_bad_data_rows_before_allocating(monkeypatch):
    from multinn_amd import ops, _lib
    W, bh, bv, v, betas = _operands()

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the checks were through")
    monkeypatch.setattr(torch, "empty", no_alloc)
    for bad in (v.float(), v.to(torch.int8), torch.zeros(2, 7, dtype=torch.uint8), torch.zeros(2, 8, 1, dtype=torch.uint8),
                torch.zeros(16, dtype=torch.uint8), torch.zeros(8, 2, dtype=torch.uint8).t(), None):
        with pytest.raises(ValueError, match="v u8"):
            ops.rbm_raise(W, bh, bv, bad, betas, 4, 0)
    with pytest.raises(ValueError, match="bias rows"):
        ops.rbm_raise(W, bh, bv, torch.zeros(3, 8, dtype=torch.uint8), betas, 4, 0)
    with pytest.raises(ValueError, match="non-decreasing"):
        ops.rbm_raise(W, bh, bv, v, torch.tensor([0.0, 0.7, 0.2, 1.0]), 4, 0)
    with pytest.raises(ValueError, match="num_chains"):
        ops.rbm_raise(W, bh, bv, v, betas, 0, 0)
    with pytest.raises(ValueError, match="log_w"):
        ops.rbm_raise(W, bh, bv, v, betas, 4, 0, log_w=torch.zeros(2, 5))
    with pytest.raises(_lib.MnnError, match="CPU"):                        # no CPU path: host tensors are refused, still before any allocation
        ops.rbm_raise(W, bh, bv, v, betas, 4, 0)


def config(P=8, tracks=("Drums", "Piano")):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 24, "highest": 24 + P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def params(gen="RBM", enc="Pass", mode="jamming"):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": enc, "num_hidden": [8] if enc != "Pass" else None},
            "generator": {"type": gen, "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": [16]}}


def test_a_bad_method_is_a_value_error_before_any_work():
    from multinn_amd import MultINN
    from multinn_amd.generators import RnnRBM, RnnNade, RnnMultiRBM
    x = torch.zeros(2, 4, 10, dtype=torch.uint8)
    gens = (RnnRBM(10, 8, [32, 32], device=CPU), RnnNade(10, 8, [32, 32], device=CPU), RnnMultiRBM(5, 8, [32, 32], tracks=["a", "b"], device=CPU))
    for g in gens:
        with pytest.raises(ValueError, match="method"):
            g.estimate_nll(x, method="reverse")
        assert g.store.theta is None                                        # nothing was materialised
    for mode, gen in (("jamming", "RBM"), ("joint", "NADE"), ("composer", "MultiRBM")):
        m = MultINN(config(), params(gen=gen, mode=mode), mode=mode, device=CPU)
        with pytest.raises(ValueError, match="method"):
            m.estimate_nll(torch.zeros(2, 4, 8, 2, dtype=torch.uint8), method="bracket")


@pytest.mark.parametrize("method", ["raise", "both"])
def test_a_host_model_is_unsupported_before_any_work(method):
    from multinn_amd import MultINN
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd.generators import RnnRBM
    g = RnnRBM(10, 8, [32, 32], device=CPU)
    with pytest.raises(MnnUnsupported, match="ROCm"):
        g.estimate_nll(torch.zeros(2, 4, 10, dtype=torch.uint8), method=method)
    assert g.store.theta is None
    for mode, gen, enc, word in (("jamming", "RBM", "Pass", "ROCm"), ("composer", "MultiRBM", "Pass", "ROCm"), ("jamming", "RBM", "DBN", "DBN")):
        m = MultINN(config(), params(gen=gen, enc=enc, mode=mode), mode=mode, device=CPU)
        with pytest.raises(MnnUnsupported, match=word):
            m.estimate_nll(torch.zeros(2, 4, 8, 2, dtype=torch.uint8), method=method)


def test_driver_evaluate_refuses_a_bad_nll_before_any_work():
    from multinn_amd import driver
    for bad in ("both", "reverse", None):
        with pytest.raises(ValueError, match="nll"):
            driver.evaluate(object(), np.zeros((2, 4, 8, 2), np.uint8), np.array([4, 4]), 2, 4, nll=bad)


def test_model_api_signatures():
    from multinn_amd.common import RBM
    from multinn_amd.generators import RnnRBM, RnnNade, RnnMultiRBM
    from multinn_amd import ops
    sig = inspect.signature(RBM.log_partition_reverse).parameters
    assert list(sig)[:2] == ["self", "v"]
    assert [sig[k].default for k in ("bh", "bv", "num_chains", "num_betas", "betas", "seed")] == [None, None, 64, 1000, None, None]
    for cls in (RnnRBM, RnnNade, RnnMultiRBM):
        assert inspect.signature(cls.estimate_nll).parameters["method"].default == "ais"
        assert inspect.signature(cls._nll_rows_built).parameters["method"].default == "ais"
    assert list(inspect.signature(ops.rbm_raise).parameters) == ["W", "bh", "bv", "v", "betas", "num_chains", "seed", "row0", "row_ids", "log_z", "log_w",
                                                                 "v_out", "stats"]


def test_bracket_arithmetic_on_hand_made_estimates():
    from multinn_amd.generators import NllEstimate, NllBracket
    t = lambda *a: torch.tensor(a, dtype=torch.float32)
    lower = NllEstimate(t(1.0, 2.0, 3.0), t(0.5, 0.5, 0.5), t(0.5, 1.5, 2.5), t(0.3, 0.0, 0.4), t(8.0, 6.0, 7.0))
    upper = NllEstimate(t(1.5, 2.5, 4.0), t(1.0, 1.0, 1.5), t(0.5, 1.5, 2.5), t(0.0, 1.2, 0.0), t(5.0, 6.0, 7.0))
    b = NllBracket(lower, upper)
    assert b.lower is lower and b.upper is upper
    assert b.gap == upper.mean - lower.mean and abs(b.gap - 2.0 / 3.0) < 1e-12
    assert abs(lower.stderr - 0.5 / 3) < 1e-7 and abs(upper.stderr - 1.2 / 3) < 1e-7       # float32 rows
    assert b.gap_stderr == math.sqrt(lower.stderr ** 2 + upper.stderr ** 2) and abs(b.gap_stderr - 1.3 / 3) < 1e-7
    # several models of the same rows: each side is NllEstimate.total of that side
    tot = NllBracket.total([b, NllBracket(upper, lower)])
    assert torch.equal(tot.lower.nll, lower.nll + upper.nll) and torch.equal(tot.upper.nll, upper.nll + lower.nll)
    assert torch.equal(tot.lower.row_stderr, NllEstimate.total([lower, upper]).row_stderr) and tot.lower.ess == 5.0 and tot.gap == 0.0
    assert NllBracket.total([b]).lower is lower and NllBracket.total([b]).upper is upper
    # exact rows: one estimate on both sides
    e = NllEstimate(t(1.0, 2.0))
    x = NllBracket(e, e)
    assert x.gap == 0.0 and x.gap_stderr == 0.0
    xx = NllBracket.total([x, x])
    assert xx.lower is xx.upper and torch.equal(xx.lower.nll, 2 * e.nll) and xx.gap == 0.0
    one = NllEstimate(t(1.0, 1.0, 1.0))
    mixed = NllBracket.total([b, NllBracket(one, one)])                                  # an exact model beside an estimated one
    assert torch.equal(mixed.lower.nll, lower.nll + 1.0) and torch.equal(mixed.upper.nll, upper.nll + 1.0) and abs(mixed.gap - b.gap) < 1e-12


# ------------------------------------------------------------------------------------------------
# the estimator's algebra in float64 (DESIGN.md section 4 "Reverse AIS"), NumPy's generator for the draws
def softplus(x):
    return np.logaddexp(0.0, x)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def exact_log_z(W, bh, bv):
    Hn = W.shape[1]
    h = np.array(list(itertools.product([0.0, 1.0], repeat=Hn)))
    t = h @ bh + softplus(bv[None, :] + h @ W.T).sum(1)
    m = t.max()
    return m + np.log(np.exp(t - m).sum())


def raise_f64(W, bh, bv, v, betas, S, rng):
    """(log Z^_rev, log w [S]) of one row from the data vector v."""
    D, Hn = W.shape
    L = len(betas)
    x = np.tile(v.astype(np.float64), (S, 1))
    A = np.zeros(S)
    for k in range(L - 1, -1, -1):
        s = x @ W
        if k < L - 1:
            A += (softplus(bh + betas[k + 1] * s) - softplus(bh + betas[k] * s)).sum(1)
        if k > 0:
            h = (rng.random((S, Hn)) < sigmoid(bh + betas[k] * s)).astype(np.float64)
            x = (rng.random((S, D)) < sigmoid(bv + betas[k] * (h @ W.T))).astype(np.float64)
    lw = -A
    m = lw.max()
    return softplus(bv).sum() + softplus(bh).sum() - (m + np.log(np.exp(lw - m).mean())), lw


def stderr_of(lw):
    w = np.exp(lw - lw.max())
    S = len(w)
    ess = w.sum() ** 2 / (w ** 2).sum()
    return np.sqrt(max(S / ess - 1.0, 0.0) / (S - 1))


@pytest.mark.parametrize("D,Hn,seed", [(6, 5, 0), (9, 4, 1)])
def test_float64_reverse_ais_matches_exact_enumeration(D, Hn, seed):
    R = np.random.default_rng(seed)
    W = R.standard_normal((D, Hn)) * 0.8
    bh, bv = R.standard_normal(Hn) * 0.5, R.standard_normal(D) * 0.5
    v = R.random(D) < 0.25
    est, lw = raise_f64(W, bh, bv, v, np.linspace(0.0, 1.0, 400), 400, R)
    ref = exact_log_z(W, bh, bv)
    assert abs(est - ref) <= max(0.02, 4 * stderr_of(lw)), (est, ref, stderr_of(lw))
    # W = 0: every increment is 0, every weight is 1
    est0, lw0 = raise_f64(np.zeros((D, Hn)), bh, bv, v, np.linspace(0.0, 1.0, 5), 8, R)
    assert np.all(lw0 == 0.0) and abs(est0 - (softplus(bv).sum() + softplus(bh).sum())) < 1e-12
