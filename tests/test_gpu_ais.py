"""Annealed importance sampling of RBM log partition functions (ops.rbm_ais, RBM.log_partition, estimate_nll) on the device: each kernel form
against the deterministic checker and a float32 restatement bit for bit, the log weights against float64, the estimate against exact
enumeration, the counter invariances, and the model-level API."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import det, philox   # noqa: E402

DEV = "cuda:0"
STREAM_H, STREAM_V = 6, 7

# (N, D, Hn, bcast): shapes that reach each form of the AIS kernel
FORMS = [(3, 10, 8, False),        # streaming (Hn < 32)
         (2, 88, 12, True),        # streaming, broadcast bias rows
         (2, 440, 256, False),     # streaming (W does not fit LDS: joint mode's D)
         (3, 88, 256, False),      # matrix cores (C1 / C3 widths)
         (2, 30, 100, True)]       # matrix cores, partial unit and visible tiles


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def softplus(x):
    return np.logaddexp(0.0, x)


def problem(N, D, Hn, bcast, seed, scale=0.3):
    R = np.random.default_rng(seed)
    W = (R.standard_normal((D, Hn)) * scale).astype(np.float32)
    bh = (R.standard_normal((1 if bcast else N, Hn)) * 0.3).astype(np.float32)
    bv = (R.standard_normal((1 if bcast else N, D)) * 0.3 - 1.0).astype(np.float32)
    return W, bh, bv


def run_ais(ops, W, bh, bv, betas, S, seed, row0=0, row_ids=None, N=None):
    N = N or max(bh.shape[0], bv.shape[0])
    D = W.shape[0]
    log_z = torch.full((N,), -7.0, device=DEV)
    log_w = torch.full((N, S), -7.0, device=DEV)
    v_out = torch.full((N, S, D), 9, device=DEV, dtype=torch.uint8)
    stats = torch.full((N, 2), -7.0, device=DEV)
    ops.rbm_ais(dev(W), dev(bh), dev(bv), dev(np.asarray(betas, np.float32)), S, seed, row0,
                None if row_ids is None else dev(np.asarray(row_ids, np.int32)), log_z, log_w, v_out, stats)
    torch.cuda.synchronize()
    return log_z.cpu().numpy(), log_w.cpu().numpy(), v_out.cpu().numpy(), stats.cpu().numpy()


def chain_index(N, S, L, ids):
    """Flattened (row, chain) pairs: global row id and c L per flattened chain."""
    rid = np.repeat(np.asarray(ids, np.uint32), S)
    c = np.tile(np.arange(S, dtype=np.uint32), N)
    return rid, c * np.uint32(L)


def rows_of(b, N, S):
    return np.repeat(np.broadcast_to(b, (N, b.shape[1])), S, axis=0).astype(np.float32)


def base_draw(seed, rid, cL, bv_rep):
    D = bv_rep.shape[1]
    u = philox.uniform(seed, STREAM_V, rid[:, None], cL[:, None], np.arange(D)[None, :])
    return (u < det.sigmoid(bv_rep)).astype(np.uint8)


def exact_tm(a, b):
    """True where the float64 sum a + b is exact (TwoSum error term zero)."""
    s = a + b
    bb = s - a
    return ((a - (s - bb)) + (b - bb)) == 0.0


def restated_chains(W, bh_rep, bv_rep, betas, seed, rid, cL):
    """The chains in float32: s as an ascending float32 sum over the active rows of W, fmaf(beta, s, b) = float32(beta s + b) (asserted
    exact in float64 on the dyadic ladder), det sigmoid, u < p.  Returns (final v, float64 log w along the restated states)."""
    L = len(betas)
    D, Hn = W.shape
    v = base_draw(seed, rid, cL, bv_rep)
    lw = np.zeros(len(rid))
    b64 = np.asarray(betas, np.float32).astype(np.float64)
    for k in range(1, L):
        s = np.cumsum(v[:, :, None].astype(np.float32) * W[None], axis=1, dtype=np.float32)[:, -1].astype(np.float64)
        lw += (softplus(bh_rep + b64[k] * s) - softplus(bh_rep + b64[k - 1] * s)).sum(1)
        if k == L - 1:
            break
        a = b64[k] * s
        assert exact_tm(a, bh_rep.astype(np.float64)).all()
        p = det.sigmoid((a + bh_rep).astype(np.float32))
        h = (philox.uniform(seed, STREAM_H, rid[:, None], (cL + k)[:, None], np.arange(Hn)[None, :]) < p).astype(np.float32)
        t = np.cumsum(h[:, :, None] * W.T[None], axis=1, dtype=np.float32)[:, -1].astype(np.float64)
        a = b64[k] * t
        assert exact_tm(a, bv_rep.astype(np.float64)).all()
        p = det.sigmoid((a + bv_rep).astype(np.float32))
        v = (philox.uniform(seed, STREAM_V, rid[:, None], (cL + k)[:, None], np.arange(D)[None, :]) < p).astype(np.uint8)
    return v, lw


# ------------------------------------------------------------------------------------------------
# 1. W = 0: the base distribution is the target
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
def test_zero_weights_give_log_z0(ops, N, D, Hn, bcast):
    _, bh, bv = problem(N, D, Hn, bcast, 1)
    W = np.zeros((D, Hn), np.float32)
    log_z, log_w, _, stats = run_ais(ops, W, bh, bv, np.linspace(0, 1, 7), 37, 5, N=N)
    assert np.all(log_w == 0.0)
    ref = softplus(np.broadcast_to(bv, (N, D)).astype(np.float64)).sum(1) + softplus(np.broadcast_to(bh, (N, Hn)).astype(np.float64)).sum(1)
    np.testing.assert_allclose(log_z, ref, rtol=2e-6)
    np.testing.assert_allclose(stats[:, 0], 37.0, rtol=1e-6)
    assert np.all(stats[:, 1] == 0.0)


# 2. a ladder [0, 1, 1, ..., 1]: one weight step, then Gibbs iterations at beta = 1 -- the checker's chain
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
@pytest.mark.parametrize("with_ids", [False, True])
def test_beta_one_tail_is_the_gibbs_chain(ops, N, D, Hn, bcast, with_ids):
    W, bh, bv = problem(N, D, Hn, bcast, 2)
    S, L, seed = 40, 6, 11
    ids = np.array([70001 + 3 * n for n in range(N)], np.uint32) if with_ids else np.arange(5, 5 + N, dtype=np.uint32)
    _, log_w, v_out, _ = run_ais(ops, W, bh, bv, [0.0] + [1.0] * (L - 1), S, seed, row0=5, row_ids=ids if with_ids else None, N=N)
    rid, cL = chain_index(N, S, L, ids)
    bh_rep, bv_rep = rows_of(bh, N, S), rows_of(bv, N, S)
    v1 = base_draw(seed, rid, cL, bv_rep)
    u_h = np.stack([philox.uniform(seed, STREAM_H, rid[:, None], (cL + k)[:, None], np.arange(Hn)[None, :]) for k in range(1, L - 1)])
    u_v = np.stack([philox.uniform(seed, STREAM_V, rid[:, None], (cL + k)[:, None], np.arange(D)[None, :]) for k in range(1, L - 1)])
    _, v = det.rbm_gibbs(v1, W, bh_rep, bv_rep, L - 2, u_h, u_v)
    np.testing.assert_array_equal(v_out.reshape(N * S, D), v)
    s = v1.astype(np.float64) @ W.astype(np.float64)
    ref = (softplus(bh_rep + s) - softplus(bh_rep.astype(np.float64))).sum(1)
    np.testing.assert_allclose(log_w.reshape(-1), ref, rtol=1e-5, atol=1e-5)


# 3 + 4. a general dyadic ladder: every final state bit for bit, the log weights against float64 increments along the same states
@pytest.mark.parametrize("N,D,Hn,bcast,L,S", [(1, 88, 256, False, 1025, 64), (2, 30, 100, True, 129, 40), (1, 440, 256, False, 33, 9),
                                              (2, 10, 8, False, 257, 24)])
def test_dyadic_ladder_bit_for_bit(ops, N, D, Hn, bcast, L, S):
    W, bh, bv = problem(N, D, Hn, bcast, 3)
    betas = np.arange(L, dtype=np.float64) / (L - 1)             # multiples of 1/1024 or coarser: exact in float32
    seed = 2024
    _, log_w, v_out, _ = run_ais(ops, W, bh, bv, betas, S, seed, row0=9, N=N)
    rid, cL = chain_index(N, S, L, np.arange(9, 9 + N))
    v, lw = restated_chains(W, rows_of(bh, N, S).astype(np.float64), rows_of(bv, N, S).astype(np.float64), betas, seed, rid, cL)
    np.testing.assert_array_equal(v_out.reshape(N * S, D), v)
    np.testing.assert_allclose(log_w.reshape(-1), lw, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(lw).max()))


# 5. the estimate against exact enumeration
def exact_log_z_hidden(W, bh, bv):
    Hn = W.shape[1]
    h = np.array(list(itertools.product([0.0, 1.0], repeat=Hn)))
    t = (h @ bh.T).T + softplus(bv[:, None, :] + (h @ W.T)[None]).sum(2)          # [N, 2^Hn]
    m = t.max(1, keepdims=True)
    return (m + np.log(np.exp(t - m).sum(1, keepdims=True)))[:, 0]


def exact_log_z_visible(W, bh, bv):
    D = W.shape[0]
    v = np.array(list(itertools.product([0.0, 1.0], repeat=D)))
    s = v @ W
    out = []
    for n in range(bh.shape[0]):
        t = v @ bv[n] + softplus(bh[n][None, :] + s).sum(1)
        m = t.max()
        out.append(m + np.log(np.exp(t - m).sum()))
    return np.array(out)


@pytest.mark.parametrize("D,Hn,N,enum,scale", [(10, 8, 64, "h", 0.5), (88, 12, 64, "h", 0.3), (16, 256, 24, "v", 0.15)])
def test_estimate_matches_exact_enumeration(ops, D, Hn, N, enum, scale):
    R = np.random.default_rng(D * 1000 + Hn)
    W = (R.standard_normal((D, Hn)) * scale).astype(np.float32)
    bh = (R.standard_normal((N, Hn)) * 0.5).astype(np.float32)
    bv = (R.standard_normal((N, D)) * 0.5).astype(np.float32)
    log_z, _, _, stats = run_ais(ops, W, bh, bv, np.arange(2000) / 1999.0, 256, 77)
    f = exact_log_z_hidden if enum == "h" else exact_log_z_visible
    ref = f(W.astype(np.float64), bh.astype(np.float64), bv.astype(np.float64))
    err = np.abs(log_z - ref)
    assert np.all(err <= np.maximum(0.02, 4 * stats[:, 1])), (err.max(), stats[:, 1].max(), stats[:, 0].min())


# 6. counters: halves with their row ids, S-prefix, seeds
@pytest.mark.parametrize("N,D,Hn,bcast", [FORMS[0], FORMS[3], FORMS[4]])
def test_invariances_and_determinism(ops, N, D, Hn, bcast):
    N = 4
    W, bh, bv = problem(N, D, Hn, bcast, 4)
    betas = np.arange(50) / 49.0
    z, w, v, st = run_ais(ops, W, bh, bv, betas, 64, 31, row0=100, N=N)
    h = N // 2
    pieces = [run_ais(ops, W, bh if bcast else bh[a:b], bv if bcast else bv[a:b], betas, 64, 31, row_ids=np.arange(100 + a, 100 + b), N=b - a)
              for a, b in ((0, h), (h, N))]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in pieces]), z)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in pieces]), w)
    np.testing.assert_array_equal(np.concatenate([p[2] for p in pieces]), v)
    z2, w2, v2, _ = run_ais(ops, W, bh, bv, betas, 128, 31, row0=100, N=N)
    np.testing.assert_array_equal(w2[:, :64], w)
    np.testing.assert_array_equal(v2[:, :64], v)
    z3, w3, v3, st3 = run_ais(ops, W, bh, bv, betas, 64, 31, row0=100, N=N)
    assert z3.tobytes() == z.tobytes() and w3.tobytes() == w.tobytes() and v3.tobytes() == v.tobytes() and st3.tobytes() == st.tobytes()
    z4, w4, _, _ = run_ais(ops, W, bh, bv, betas, 64, 32, row0=100, N=N)
    assert not np.array_equal(w4, w)


def test_forms_agree_on_the_chains(ops, monkeypatch):
    """The streaming form reaches the matrix-core form's states at a shape both take (the same draws; log w may differ in its last bits)."""
    W, bh, bv = problem(2, 88, 256, False, 5)
    betas = np.arange(65) / 64.0
    z, w, v, _ = run_ais(ops, W, bh, bv, betas, 16, 3)
    monkeypatch.setenv("MNN_RBM_NO_MFMA", "1")
    zs, ws, vs, _ = run_ais(ops, W, bh, bv, betas, 16, 3)
    np.testing.assert_array_equal(vs, v)
    np.testing.assert_allclose(ws, w, rtol=1e-5, atol=1e-4)


# 7. model level
def tiny_rbm(seed=5):
    from multinn_amd.generators import RnnRBM
    g = RnnRBM(10, 8, [32, 32], precision="fp32", seed=seed)
    g._materialize(10)
    R = np.random.default_rng(seed)
    with torch.no_grad():                                                  # livelier weights than the glorot start
        g.store["rbm/W"].copy_(dev((R.standard_normal((10, 8)) * 0.5).astype(np.float32)))
        g.store["Wuh"].mul_(3.0)
        g.store["Wuv"].mul_(3.0)
    g._packed_step = -1
    return g


def sequences(B=3, T=5, P=10, seed=0):
    R = np.random.default_rng(seed)
    return dev((R.random((B, T, P)) < 0.25).astype(np.uint8))


def test_rnn_rbm_estimate_matches_exact_nll(ops):
    g = tiny_rbm()
    x = sequences()
    est = g.estimate_nll(x, num_chains=256, num_betas=2000)
    Hn, D = 8, 10
    out = g._ctx["out"][g._idx()].double().cpu().numpy()
    bh, bv = out[:, :Hn], out[:, Hn:Hn + D]
    W = g.store["rbm/W"].double().cpu().numpy()
    v = x.reshape(-1, D).cpu().numpy().astype(np.float64)                  # API order: b-major, then t
    F = -(v * bv).sum(1) - softplus(bh + v @ W).sum(1)
    ref = F + exact_log_z_hidden(W, bh, bv)
    nll = est.nll.cpu().numpy()
    assert nll.shape == (15,) and np.isfinite(est.mean)
    np.testing.assert_allclose(est.free_energy.cpu().numpy(), F, rtol=1e-5, atol=1e-4)
    tol = np.maximum(0.02, 4 * est.row_stderr.cpu().numpy())
    assert np.all(np.abs(nll - ref) <= tol), (np.abs(nll - ref).max(), tol.max())
    assert est.ess > 1 and 0 < est.stderr < 0.05
    assert abs(est.mean - nll.mean()) < 1e-5


def test_ragged_lengths_drop_padding_rows(ops):
    g = tiny_rbm()
    x = sequences()
    full = g.estimate_nll(x, num_chains=32, num_betas=100, seed=9)
    lengths = torch.tensor([5, 2, 4], dtype=torch.int32)
    rag = g.estimate_nll(x, lengths=lengths, num_chains=32, num_betas=100, seed=9)
    keep = (torch.arange(5)[None, :] < lengths[:, None]).reshape(-1).to(DEV)
    assert rag.nll.numel() == 11
    assert torch.equal(rag.log_z, full.log_z[keep])                    # same bias rows, same row ids: the same chains
    torch.testing.assert_close(rag.nll, full.nll[keep], rtol=1e-6, atol=1e-5)


def mode_config(P=10, tracks=("Piano", "Guitar")):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 24, "highest": 24 + P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def mode_params(mode, gen):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
            "generator": {"type": gen, "num_hidden": 8, "num_hidden_rnn": [32, 32], "feedback": [16]}}


def test_jamming_estimate_is_the_sum_over_generators(ops):
    from multinn_amd import MultINN
    from multinn_amd.generators import NllEstimate
    m = MultINN(mode_config(), mode_params("jamming", "RBM"), mode="jamming", precision="fp32")
    R = np.random.default_rng(1)
    x = dev((R.random((3, 4, 10, 2)) < 0.3).astype(np.uint8))
    est = m.estimate_nll(x, num_chains=32, num_betas=50)
    parts = [g._nll_rows_built(num_chains=32, num_betas=50) for g in m._generators]
    assert len(parts) == 2 and est.nll.numel() == 12
    tot = NllEstimate.total(parts)
    assert torch.equal(est.nll, parts[0].nll + parts[1].nll) and torch.equal(est.nll, tot.nll)
    assert torch.equal(est.log_z, parts[0].log_z + parts[1].log_z)
    assert abs(est.mean - float(est.nll.double().mean())) < 1e-4


def test_nade_joint_rows_are_the_eval_loss_rows(ops):
    from multinn_amd import MultINN
    m = MultINN(mode_config(), mode_params("joint", "NADE"), mode="joint", precision="fp32")
    R = np.random.default_rng(2)
    x = dev((R.random((3, 4, 10, 2)) < 0.3).astype(np.uint8))
    lengths = torch.tensor([4, 3, 4], dtype=torch.int32, device=DEV)
    est = m.estimate_nll(x, lengths=lengths)
    rows = m._generators[0].log_probs
    assert est.stderr == 0.0 and est.log_z is None
    assert torch.equal(est.nll, rows) and est.nll.numel() == 11
    m.build_pianoroll(x, lengths, is_train=False, mode="eval")
    assert torch.equal(m._generators[0].log_probs, rows)


def test_driver_evaluate_keeps_the_loss_and_reports_ais(ops):
    from multinn_amd import MultINN, driver
    m = MultINN(mode_config(), mode_params("jamming", "RBM"), mode="jamming", precision="fp32")
    R = np.random.default_rng(3)
    X = (R.random((4, 8, 10, 2)) < 0.3).astype(np.uint8)
    lengths = np.array([8, 8, 6, 8])
    a = driver.evaluate(m, X, lengths, 2, 8)
    b = driver.evaluate(m, X, lengths, 2, 8, nll="loss")
    assert a == b
    c = driver.evaluate(m, X, lengths, 2, 8, nll="ais", ais=dict(num_chains=16, num_betas=40))
    assert np.isfinite(c) and c > 0
