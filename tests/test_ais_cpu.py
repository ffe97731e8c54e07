"""Log-likelihood estimation of RBM generators by annealed importance sampling (AIS): the parts that need no GPU.  The estimator's algebra in
float64 against exact enumeration, the host-side refusals of the C ABI and of ops.rbm_ais, the early refusals of the model API, and the build
guard of the AIS kernels."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CPU = torch.device("cpu")


def softplus(x):
    return np.logaddexp(0.0, x)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def exact_log_z(W, bh, bv):
    """log sum_{v,h} exp(bv.v + bh.h + v W h), summing the visibles out analytically over all 2^Hn hidden states."""
    Hn = W.shape[1]
    h = np.array(list(itertools.product([0.0, 1.0], repeat=Hn)))
    t = h @ bh + softplus(bv[None, :] + h @ W.T).sum(1)
    m = t.max()
    return m + np.log(np.exp(t - m).sum())


def ais_f64(W, bh, bv, betas, S, rng):
    """The estimator of DESIGN.md section 4, restated in float64 with NumPy's generator: (log Z^, log w [S])."""
    D, Hn = W.shape
    log_z0 = softplus(bv).sum() + softplus(bh).sum()
    v = (rng.random((S, D)) < sigmoid(bv)).astype(np.float64)
    lw = np.zeros(S)
    L = len(betas)
    for k in range(1, L):
        s = v @ W
        lw += (softplus(bh + betas[k] * s) - softplus(bh + betas[k - 1] * s)).sum(1)
        if k < L - 1:
            h = (rng.random((S, Hn)) < sigmoid(bh + betas[k] * s)).astype(np.float64)
            v = (rng.random((S, D)) < sigmoid(bv + betas[k] * (h @ W.T))).astype(np.float64)
    m = lw.max()
    return log_z0 + m + np.log(np.exp(lw - m).mean()), lw


def stderr_of(lw):
    w = np.exp(lw - lw.max())
    S = len(w)
    ess = w.sum() ** 2 / (w ** 2).sum()
    return np.sqrt(max(S / ess - 1.0, 0.0) / (S - 1))


@pytest.mark.parametrize("D,Hn,seed", [(6, 5, 0), (9, 4, 1)])
def test_float64_ais_matches_exact_enumeration(D, Hn, seed):
    R = np.random.default_rng(seed)
    W = R.standard_normal((D, Hn)) * 0.8
    bh, bv = R.standard_normal(Hn) * 0.5, R.standard_normal(D) * 0.5
    est, lw = ais_f64(W, bh, bv, np.linspace(0.0, 1.0, 400), 400, R)
    ref = exact_log_z(W, bh, bv)
    assert abs(est - ref) <= max(0.02, 4 * stderr_of(lw)), (est, ref, stderr_of(lw))
    # W = 0: the base distribution is the target, every weight is 1
    est0, lw0 = ais_f64(np.zeros((D, Hn)), bh, bv, np.linspace(0.0, 1.0, 5), 8, R)
    assert np.all(lw0 == 0.0) and abs(est0 - (softplus(bv).sum() + softplus(bh).sum())) < 1e-12


def _ais_args(**over):
    a = dict(N=2, D=8, Hn=16, S=4, L=10, betas=1, W=1, bh=1, ld_bh=0, bv=1, ld_bv=0, log_z=1, ws=1)
    a.update(over)
    p = lambda x: None if x is None else 16        # any non-null address: nothing may be dereferenced before the checks fail
    return (None, a["N"], a["D"], a["Hn"], a["S"], a["L"], p(a["betas"]), p(a["W"]), p(a["bh"]), a["ld_bh"], p(a["bv"]), a["ld_bv"], 7, 0,
            None, p(a["log_z"]), None, None, None, p(a["ws"]))


@pytest.mark.parametrize("over,word", [(dict(L=1), b"n_betas"), (dict(S=0), b"n_chains"), (dict(N=0), b"sizes"), (dict(Hn=-1), b"sizes"),
                                       (dict(S=1 << 22, L=1 << 10), b"32-bit"), (dict(betas=None), b"null"), (dict(ws=None), b"null"),
                                       (dict(log_z=None), b"null"), (dict(ld_bh=3), b"leading"), (dict(ld_bv=5), b"leading"),
                                       (dict(D=40000, Hn=40000), b"LDS")])
def test_c_abi_refuses_bad_arguments_without_a_device(lib, over, word):
    rc = lib.mnn_rbm_ais(*_ais_args(**over))
    assert rc == -1 and word in lib.mnn_last_error(), (rc, lib.mnn_last_error())


def test_c_abi_workspace_and_version(lib):
    from multinn_amd import _lib
    assert _lib.ABI_VERSION == lib.mnn_version() == 124
    assert lib.mnn_rbm_ais_workspace_bytes(3, 88, 256, 64, 1000) >= 3 * 64 * 8
    assert lib.mnn_rbm_ais_workspace_bytes(0, 88, 256, 64, 1000) == 0


@pytest.mark.parametrize("betas,word", [([0.0], "two"), ([0.0, 0.5, 0.4, 1.0], "non-decreasing"), ([0.1, 1.0], "start at 0"),
                                        ([0.0, 0.9], "end at 1"), ([0.0, float("nan"), 1.0], "finite"), ([0.0, float("inf"), 1.0], "finite")])
def test_ops_refuses_bad_ladders(betas, word):
    from multinn_amd import ops
    W, bh, bv = torch.zeros(8, 16), torch.zeros(1, 16), torch.zeros(1, 8)
    with pytest.raises(ValueError, match=word):
        ops.rbm_ais(W, bh, bv, torch.tensor(betas, dtype=torch.float32), 4, 0)


def test_ops_refuses_bad_operands_and_cpu_tensors():
    from multinn_amd import ops, _lib
    betas = torch.linspace(0, 1, 5)
    betas[-1] = 1.0
    W = torch.zeros(8, 16)
    with pytest.raises(ValueError, match="bias rows"):
        ops.rbm_ais(W, torch.zeros(3, 16), torch.zeros(2, 8), betas, 4, 0)
    with pytest.raises(ValueError, match="betas"):
        ops.rbm_ais(W, torch.zeros(1, 16), torch.zeros(1, 8), betas.double(), 4, 0)
    with pytest.raises(ValueError, match="num_chains"):
        ops.rbm_ais(W, torch.zeros(1, 16), torch.zeros(1, 8), betas, 0, 0)
    with pytest.raises(_lib.MnnError, match="CPU"):
        ops.rbm_ais(W, torch.zeros(1, 16), torch.zeros(1, 8), betas, 4, 0)


def config(P=8, tracks=("Drums", "Piano")):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 24, "highest": 24 + P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def params(gen="RBM", enc="Pass"):
    return {"mode": "jamming", "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": enc, "num_hidden": [8] if enc != "Pass" else None},
            "generator": {"type": gen, "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": [16]}}


def test_dbn_encoder_modes_refuse_estimate_nll():
    from multinn_amd import MultINN
    from multinn_amd._lib import MnnUnsupported
    m = MultINN(config(), params(enc="DBN"), mode="jamming", device=CPU)
    with pytest.raises(MnnUnsupported, match="DBN"):
        m.estimate_nll(torch.zeros(2, 4, 8, 2, dtype=torch.uint8))


@pytest.mark.parametrize("mode,gen", [("jamming", "RBM"), ("joint", "RBM"), ("joint", "NADE")])
def test_estimate_nll_on_a_cpu_model_fails_early(mode, gen):
    from multinn_amd import MultINN
    from multinn_amd._lib import MnnError
    m = MultINN(config(), params(gen=gen), mode=mode, device=CPU)
    with pytest.raises(NotImplementedError) as e:
        m.estimate_nll(torch.zeros(2, 4, 8, 2, dtype=torch.uint8))
    assert isinstance(e.value, MnnError) and "ROCm" in str(e.value)


def test_generator_estimate_nll_on_a_cpu_model_fails_early():
    from multinn_amd.generators import RnnRBM, RnnNade
    from multinn_amd._lib import MnnError
    for g in (RnnRBM(10, 8, [32, 32], device=CPU), RnnNade(10, 8, [32, 32], device=CPU)):
        with pytest.raises(NotImplementedError) as e:
            g.estimate_nll(torch.zeros(2, 4, 10, dtype=torch.uint8))
        assert isinstance(e.value, MnnError)
        assert g.store.theta is None                                    # nothing was materialised


def test_model_api_signatures():
    import inspect
    from multinn_amd.common import RBM
    from multinn_amd.generators import RnnRBM
    from multinn_amd import driver
    sig = inspect.signature(RBM.log_partition).parameters
    assert [sig[k].default for k in ("bh", "bv", "num_chains", "num_betas", "betas", "seed")] == [None, None, 64, 1000, None, None]
    sig = inspect.signature(RnnRBM.estimate_nll).parameters
    assert [sig[k].default for k in ("lengths", "num_chains", "num_betas", "betas", "seed")] == [None, 64, 1000, None, None]
    assert inspect.signature(driver.evaluate).parameters["nll"].default == "loss"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ais_kernels_use_no_scratch_and_the_matrix_cores(tmp_path):
    from multinn_amd import build
    assert "rbm_ais.hip" in build.SOURCES
    out = str(tmp_path / "ais.s")
    subprocess.check_call([HIPCC] + build.flags_for("rbm_ais.hip") + ["-S", "--cuda-device-only", os.path.join(build.CSRC, "rbm_ais.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    sizes = {m.group(1): int(m.group(2))
             for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    kernels = {k: v for k, v in sizes.items() if "rbm_ais_" in k}
    assert len(kernels) == 3 and all(v == 0 for v in kernels.values()), kernels
    bodies = {m.group(1): m.group(0) for m in re.finditer(r"\n(_Z\w*rbm_ais_(\w+?)_kernel\w*):.*?s_endpgm", text, re.S)}
    mfma = [b for name, b in bodies.items() if "mfma" in name]
    assert len(mfma) == 1 and "v_mfma_f32_32x32x2_f32" in mfma[0]
