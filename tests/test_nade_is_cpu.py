"""The NADE importance estimator (mnn_nade_given_is, ops.nade_given_is, estimate_nll(partial="importance"), driver.evaluate(partial=)): the
parts that need no GPU.  The C ABI's declaration, binding and host-side refusals, the early refusals of the op and of the model API (every
one before any device work, the default call with the old text), and the reference of tests/nade_is_reference.py itself against exact
enumeration: its accuracy with many particles and the direction of the two biases with two -- at the seeds the GPU tests then use."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import nade_is_reference as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------
# 1. the C ABI
def test_header_declares_and_loader_binds_the_entry(lib):
    from multinn_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "multinn_hip.h")).read()
    decl = re.search(r"\bint mnn_nade_given_is\(([^;]*)\);", hdr)
    assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES["mnn_nade_given_is"][1]) == 22
    assert re.search(r"size_t mnn_nade_given_is_workspace_bytes\(int tracks, int N, int n_particles\);", hdr)
    assert re.search(r"MNN_STREAM_NADE_IS = 11, MNN_STREAM_NADE_IS_DATA = 12", hdr)
    assert hasattr(lib, "mnn_nade_given_is") and hasattr(lib, "mnn_nade_given_is_workspace_bytes")
    assert "nade_is.hip" in build.SOURCES
    assert _lib.ABI_VERSION == lib.mnn_version() == 124                                 # a pure addition
    assert lib.mnn_nade_given_is_workspace_bytes(2, 3, 5) >= 2 * 3 * 5 * 4 and lib.mnn_nade_given_is_workspace_bytes(2, 3, 0) == 0


def _args(**over):
    a = dict(tracks=2, N=3, D=8, Hn=16, bias=1, ld_bias=48, w_enc=1, w_dec=1, given=1, gs=24, data=None, ds=24, C=4, log_pg=1, ws=1)
    a.update(over)
    p = lambda x: None if x is None else 16        # any non-null address: nothing may be dereferenced before the checks fail
    return (None, a["tracks"], a["N"], a["D"], a["Hn"], p(a["bias"]), a["ld_bias"], p(a["w_enc"]), p(a["w_dec"]), p(a["given"]), a["gs"],
            p(a["data"]), a["ds"], a["C"], 7, 0, None, p(a["log_pg"]), None, None, None, p(a["ws"]))


@pytest.mark.parametrize("over,word", [(dict(C=0), b"n_particles"), (dict(C=-3), b"n_particles"), (dict(given=None), b"null"), (dict(ws=None), b"null"),
                                       (dict(log_pg=None), b"null"), (dict(D=1537, ld_bias=4000), b"D <= 1536"), (dict(Hn=257, ld_bias=4000), b"Hn<=256"),
                                       (dict(Hn=0), b"Hn"), (dict(ld_bias=47), b"ld_bias"), (dict(gs=23), b"g_track_stride"),
                                       (dict(data=1, ds=23), b"d_track_stride"), (dict(tracks=0), b"tracks")])
def test_c_abi_refuses_bad_arguments_without_a_device(lib, over, word):
    rc = lib.mnn_nade_given_is(*_args(**over))
    msg = lib.mnn_last_error()
    assert rc == -1 and word in msg and msg.startswith(b"mnn_nade_given_is"), (rc, msg)


# ------------------------------------------------------------------------------------------------
# 2. the op
def _operands(tracks=2, N=3, D=8, Hn=16):
    return (torch.zeros(N, tracks * (Hn + D)), torch.zeros(tracks, D, Hn), torch.zeros(tracks, D, Hn),
            torch.full((tracks, N, D), 255, dtype=torch.uint8))


def test_op_refuses_bad_operands_before_allocating(monkeypatch):
    from multinn_amd import ops, _lib
    bias, we, wd, codes = _operands()

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the checks were through")
    monkeypatch.setattr(torch, "empty", no_alloc)
    for bad in (codes.float(), codes.bool(), codes[:, :, :7], codes[:1], codes.reshape(3, 2, 8), codes.transpose(0, 1), None, [[255] * 8] * 3):
        with pytest.raises(ValueError, match="given u8"):
            ops.nade_given_is(bias, we, wd, 2, 8, 16, bad, 4, 0)
    for bad in (codes.float(), codes[:, :2], codes.reshape(3, 2, 8)):
        with pytest.raises(ValueError, match="data u8"):
            ops.nade_given_is(bias, we, wd, 2, 8, 16, codes, 4, 0, data=bad)
    for c in (0, -1):
        with pytest.raises(ValueError, match="num_particles"):
            ops.nade_given_is(bias, we, wd, 2, 8, 16, codes, c, 0)
    with pytest.raises(ValueError, match="bias"):
        ops.nade_given_is(bias[:, :47], we, wd, 2, 8, 16, codes, 4, 0)
    with pytest.raises(ValueError, match="weights"):
        ops.nade_given_is(bias, we[:1], wd, 2, 8, 16, codes, 4, 0)
    with pytest.raises(ValueError, match="D <= 1536"):
        ops.nade_given_is(bias, we, wd, 2, 1537, 16, codes, 4, 0)
    with pytest.raises(ValueError, match="row_ids"):
        ops.nade_given_is(bias, we, wd, 2, 8, 16, codes, 4, 0, row_ids=torch.zeros(3, dtype=torch.int64))
    for kw, word in ((dict(log_w=torch.zeros(2, 3, 5)), "log_w"), (dict(stats=torch.zeros(2, 3)), "stats"),
                     (dict(v_out=torch.zeros(2, 3, 4, 8)), "v_out"), (dict(log_pg=torch.zeros(3, 2)), "log_pg")):
        with pytest.raises(ValueError, match=word):
            ops.nade_given_is(bias, we, wd, 2, 8, 16, codes, 4, 0, **kw)
    for data in (None, torch.zeros(2, 3, 8, dtype=torch.uint8)):
        with pytest.raises(_lib.MnnError, match="CPU"):                    # no CPU path: host tensors are refused, still before any allocation
            ops.nade_given_is(bias, we, wd, 2, 8, 16, codes, 4, 0, data=data)


def test_op_passes_the_planes_and_both_sides_to_the_entry(monkeypatch):
    from multinn_amd import ops
    bias, we, wd, codes = _operands()
    data = torch.zeros(2, 3, 8, dtype=torch.uint8)
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else id(t))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops._lib, "load", lambda: type("L", (), {"mnn_nade_given_is_workspace_bytes": staticmethod(lambda *a: 256)})())
    ids = torch.arange(3, dtype=torch.int32)
    out = ops.nade_given_is(bias, we, wd, 2, 8, 16, codes, 5, 9, row0=4)
    ops.nade_given_is(bias, we, wd, 2, 8, 16, codes, 5, 9, row_ids=ids, data=data)
    assert tuple(out.shape) == (2, 3) and [c[0] for c in calls] == ["mnn_nade_given_is"] * 2 and all(len(c[1]) == 22 for c in calls)
    lower, upper = calls[0][1], calls[1][1]
    assert lower[1:5] == (2, 3, 8, 16) and lower[6] == 48 and lower[9:16] == (id(codes), 24, None, 24, 5, 9, 4) and lower[16] is None
    assert upper[9:14] == (id(codes), 24, id(data), 24, 5) and upper[16] == id(ids)


# ------------------------------------------------------------------------------------------------
# 3. the model API: validation and refusals, all before store.theta exists
def test_signatures_carry_partial_with_the_refusing_default():
    from multinn_amd.generators import RnnRBM, RnnNade, RnnMultiNADE, RnnMultiRBM
    from multinn_amd.modes import MultINNCore
    from multinn_amd import driver
    for f in (RnnRBM.estimate_nll, RnnNade.estimate_nll, RnnMultiNADE.estimate_nll, RnnMultiRBM.estimate_nll, MultINNCore.estimate_nll, driver.evaluate,
              RnnNade._nll_rows_built, RnnRBM._nll_rows_built, RnnNade._refuse_nll_given):
        assert inspect.signature(f).parameters["partial"].default == "refuse", f


def test_generators_validate_partial_before_any_work():
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd.generators import RnnRBM, RnnNade, RnnMultiNADE, NADE_MASK_REFUSAL
    x = torch.zeros(2, 4, 10, dtype=torch.uint8)
    half = torch.arange(10) < 5
    gens = (RnnNade(10, 8, [32, 32], device=CPU), RnnMultiNADE(5, 8, [32, 32], tracks=["a", "b"], device=CPU), RnnRBM(10, 8, [32, 32], device=CPU))
    for g in gens:
        for bad in ("is", "Importance", None, True, 1):
            with pytest.raises(ValueError, match="partial must be"):
                g.estimate_nll(x, given_mask=half, partial=bad)
            with pytest.raises(ValueError, match="partial must be"):
                g.estimate_nll(x, partial=bad)
        assert g.store.theta is None
    for g in gens[:2]:
        for kw in ({}, dict(partial="refuse")):                              # the default call still refuses, with the old text
            with pytest.raises(MnnUnsupported) as e:
                g.estimate_nll(x, given_mask=half, **kw)
            assert str(e.value) == NADE_MASK_REFUSAL and "not a sum of its conditionals" in str(e.value)
        for bad in (0, -2, 2.0, True):
            with pytest.raises(ValueError, match="num_chains particles"):
                g.estimate_nll(x, given_mask=half, partial="importance", num_chains=bad)
        with pytest.raises(MnnUnsupported, match="ROCm"):                    # the partial mask passes with "importance": the next refusal
            g.estimate_nll(x, given_mask=half, partial="importance")
        with pytest.raises(ValueError, match="method must be"):
            g.estimate_nll(x, given_mask=half, partial="importance", method="lower")
        assert g.store.theta is None
    with pytest.raises(MnnUnsupported, match="ROCm"):                        # RBM estimators accept and ignore it
        gens[2].estimate_nll(x, given_mask=half, partial="importance", num_chains=0)
    assert gens[2].store.theta is None


def config(P=8, tracks=("Drums", "Piano")):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 24, "highest": 24 + P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def params(gen="RBM", enc="Pass", mode="jamming"):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": enc, "num_hidden": [8] if enc != "Pass" else None},
            "generator": {"type": gen, "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": [16]}}


def no_theta(m):
    return all(g.store.theta is None for g in m._generators)


def test_modes_validate_partial_before_any_work():
    from multinn_amd import MultINN
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd.generators import NADE_MASK_REFUSAL
    x = torch.zeros(2, 4, 8, 2, dtype=torch.uint8)
    track0 = torch.tensor([True, False])
    low = (torch.arange(8) < 4)[:, None].expand(8, 2)
    for mode, mask in (("joint", track0), ("joint", low), ("jamming", low), ("feedback", low), ("composer", low)):
        m = MultINN(config(), params(gen="NADE", mode=mode), mode=mode, device=CPU)
        with pytest.raises(MnnUnsupported) as e:                             # the default: the old refusal, word for word
            m.estimate_nll(x, given_mask=mask)
        assert str(e.value) == NADE_MASK_REFUSAL
        with pytest.raises(ValueError, match="partial must be"):
            m.estimate_nll(x, given_mask=mask, partial="sample")
        with pytest.raises(ValueError, match="num_chains particles"):
            m.estimate_nll(x, given_mask=mask, partial="importance", num_chains=0)
        with pytest.raises(MnnUnsupported, match="ROCm"):                    # let through: the host-model refusal is next
            m.estimate_nll(x, given_mask=mask, partial="importance", method="both")
        assert no_theta(m)
    m = MultINN(config(), params(gen="RBM", mode="joint"), mode="joint", device=CPU)
    with pytest.raises(MnnUnsupported, match="ROCm"):
        m.estimate_nll(x, given_mask=track0, partial="importance")
    # the DBN refusal stays first
    m = MultINN(config(), params(gen="NADE", enc="DBN", mode="jamming"), mode="jamming", device=CPU)
    with pytest.raises(MnnUnsupported, match="DBN"):
        m.estimate_nll(x, given_mask=low, partial="importance")


def test_driver_evaluate_validates_partial_before_any_work():
    from multinn_amd import driver
    X, lengths = np.zeros((2, 4, 8, 2), np.uint8), np.array([4, 4])
    with pytest.raises(ValueError, match="partial must be"):
        driver.evaluate(object(), X, lengths, 2, 4, nll="bracket", given_mask=[True, False], partial="is")


# ------------------------------------------------------------------------------------------------
# 4. the reference itself (D = 10, Hn = 8), at the seeds the GPU tests use
ACCURACY = dict(n_rows=16, w_scale=1.0, seed=5, C=4096, draw_seed=3)
BIAS = dict(n_rows=1500, w_scale=2.0, seed=1, C=2, draw_seed=7)


def toy_exact(bias, we, wd, codes):
    b_enc, b_dec = REF.split_bias(bias, 1, 0, REF.TOY_D, REF.TOY_HN)
    return REF.exact_log_pg(b_enc, b_dec, we[0], wd[0], codes)


def test_enumeration_sums_to_one_and_factorises():
    """No cell given: log p(nothing) = 0 (up to the 1e-6 inside the logs); every cell given: -NLL(x); a given prefix: the product of its
    conditionals, which no free cell behind it touches."""
    from oracle import nade as onade
    bias, we, wd, x, codes = REF.toy_problem(6, 1.0, 2)
    b_enc, b_dec = REF.split_bias(bias.astype(np.float64), 1, 0, REF.TOY_D, REF.TOY_HN)
    free = np.full_like(codes, REF.FREE)
    np.testing.assert_allclose(toy_exact(bias, we, wd, free), 0.0, atol=1e-4)
    nll, cp = onade.log_prob(x.astype(np.float64), b_enc, b_dec, we[0].astype(np.float64), wd[0].astype(np.float64))
    np.testing.assert_allclose(toy_exact(bias, we, wd, x), -nll, rtol=1e-12)
    prefix = free.copy()
    prefix[:, :4] = x[:, :4]
    q = np.where(x[:, :4] > 0, cp[:, :4], 1 - cp[:, :4])
    np.testing.assert_allclose(toy_exact(bias, we, wd, prefix), np.log(1e-6 + q).sum(1), rtol=1e-4, atol=1e-5)


def test_reference_lower_estimate_matches_enumeration():
    """C = 4096: every row within 5 of its own reported standard errors of the exact log p(x_G)."""
    a = ACCURACY
    bias, we, wd, _, codes = REF.toy_problem(a["n_rows"], a["w_scale"], a["seed"])
    exact = toy_exact(bias, we, wd, codes)
    _, _, log_pg, ess, se = REF.estimate(bias, we, wd, 1, 0, REF.TOY_D, REF.TOY_HN, codes, None, a["C"], a["draw_seed"], np.arange(a["n_rows"]))
    err = np.abs(log_pg - exact) / se
    print("lower estimate against enumeration, C = 4096: error in reported standard errors, max", err.max(), "stderr max", se.max(), "min ESS", ess.min())
    assert np.all(se > 0) and np.all(err < 5), (err.max(), se.max())


def test_reference_biases_point_in_opposite_directions():
    """1500 rows drawn from the model, C = 2, weights N(0, 2^2): mean lower < mean exact < mean upper, each gap more than 3 standard errors
    of the paired differences (the float64 NumPy check behind the design had about 8)."""
    b = BIAS
    bias, we, wd, x, codes = REF.toy_problem(b["n_rows"], b["w_scale"], b["seed"])
    exact = toy_exact(bias, we, wd, codes)
    ids = np.arange(b["n_rows"])
    lower = REF.estimate(bias, we, wd, 1, 0, REF.TOY_D, REF.TOY_HN, codes, None, b["C"], b["draw_seed"], ids)[2]
    upper = REF.estimate(bias, we, wd, 1, 0, REF.TOY_D, REF.TOY_HN, codes, x, b["C"], b["draw_seed"], ids)[2]
    below, above = REF.paired_margin(exact, lower), REF.paired_margin(upper, exact)
    print("means: lower", lower.mean(), "exact", exact.mean(), "upper", upper.mean(), "| margins in standard errors:", below, above)
    assert lower.mean() < exact.mean() < upper.mean() and below > 3 and above > 3, (below, above)


def test_upper_side_particle_zero_is_the_data_and_reads_no_uniform():
    bias, we, wd, x, codes = REF.toy_problem(8, 1.0, 4)
    ids = np.arange(100, 108)
    v1, lw1 = REF.particles(bias, we, wd, 1, 0, REF.TOY_D, REF.TOY_HN, codes, x, 3, 1, ids)
    v2, lw2 = REF.particles(bias, we, wd, 1, 0, REF.TOY_D, REF.TOY_HN, codes, x, 3, 2, ids)
    assert np.array_equal(v1[:, 0], x) and np.array_equal(lw1[:, 0], lw2[:, 0]) and not np.array_equal(v1[:, 1:], v2[:, 1:])
    lo, _ = REF.particles(bias, we, wd, 1, 0, REF.TOY_D, REF.TOY_HN, codes, None, 3, 1, ids)
    assert not np.array_equal(lo[:, 1:], v1[:, 1:])                          # the two sides of one seed share no uniform
