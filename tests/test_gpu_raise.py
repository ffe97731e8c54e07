"""Reverse annealed importance sampling of RBM log partition functions (ops.rbm_raise, RBM.log_partition_reverse, estimate_nll(method=...))
on the device: each kernel form against the deterministic checker and a float32 restatement bit for bit, the log weights against float64, the
estimate against exact enumeration, the direction of the forward and reverse biases on model-distributed data, the counter invariances, and
the model-level API (method="raise" / "both", the modes, driver.evaluate).  The helpers restate tests/test_gpu_ais.py's for the reverse run."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import det, philox   # noqa: E402

DEV = "cuda:0"
STREAM_H, STREAM_V = 8, 9                     # the reverse chains' Philox streams (the forward chains draw from 6 / 7)

# (N, D, Hn, bcast): shapes that reach each form of the kernel
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


def data_rows(N, D, seed, density=0.25):
    return (np.random.default_rng(1000 + seed).random((N, D)) < density).astype(np.uint8)


def outputs(N, S, D):
    return (torch.full((N,), -7.0, device=DEV), torch.full((N, S), -7.0, device=DEV), torch.full((N, S, D), 9, device=DEV, dtype=torch.uint8),
            torch.full((N, 2), -7.0, device=DEV))


def run_raise(ops, W, bh, bv, v, betas, S, seed, row0=0, row_ids=None):
    N, D = v.shape
    out = outputs(N, S, D)
    ops.rbm_raise(dev(W), dev(bh), dev(bv), dev(v), dev(np.asarray(betas, np.float32)), S, seed, row0,
                  None if row_ids is None else dev(np.asarray(row_ids, np.int32)), *out)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def run_ais(ops, W, bh, bv, N, betas, S, seed, row0=0):
    out = outputs(N, S, W.shape[0])
    ops.rbm_ais(dev(W), dev(bh), dev(bv), dev(np.asarray(betas, np.float32)), S, seed, row0, None, *out)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def chain_index(N, S, L, ids):
    """Flattened (row, chain) pairs: global row id and c L per flattened chain."""
    rid = np.repeat(np.asarray(ids, np.uint32), S)
    c = np.tile(np.arange(S, dtype=np.uint32), N)
    return rid, c * np.uint32(L)


def rows_of(b, N, S):
    return np.repeat(np.broadcast_to(b, (N, b.shape[1])), S, axis=0).astype(np.float32)


def uniforms(seed, stream, rid, sub, n):
    return philox.uniform(seed, stream, rid[:, None], sub[:, None], np.arange(n)[None, :])


def exact_tm(a, b):
    """True where the float64 sum a + b is exact (TwoSum error term zero)."""
    s = a + b
    bb = s - a
    return ((a - (s - bb)) + (b - bb)) == 0.0


def ascending_sum(x, W):
    """x [n, K] of 0 / 1 times W [K, m] as the ascending float32 sum over k from 0, one rounding per term (the device's fmaf chain: a
    product with 0 or 1 is exact) -> float64 [n, m]."""
    acc = np.zeros((x.shape[0], W.shape[1]), np.float32)
    xf = x.astype(np.float32)
    for k in range(W.shape[0]):
        acc += xf[:, k:k + 1] * W[k]
    return acc.astype(np.float64)


def restated_chains(W, bh_rep, bv_rep, x0, betas, seed, rid, cL):
    """The reverse chains in float32: s as an ascending float32 sum over the active rows of W, fmaf(beta, s, b) = float32(beta s + b)
    (asserted exact in float64 on the dyadic ladder), det sigmoid, u < p, from k = L-1 down to 1; the increment between b_k and b_{k+1} on
    the state that enters rung k.  Returns (final x, float64 log w = -A along the restated states)."""
    L = len(betas)
    D, Hn = W.shape
    Wt = np.ascontiguousarray(W.T)
    x = x0.copy()
    lw = np.zeros(len(rid))
    b64 = np.asarray(betas, np.float32).astype(np.float64)
    for k in range(L - 1, -1, -1):
        s = ascending_sum(x, W)
        if k < L - 1:
            lw -= (softplus(bh_rep + b64[k + 1] * s) - softplus(bh_rep + b64[k] * s)).sum(1)
        if k == 0:
            break
        a = b64[k] * s
        assert exact_tm(a, bh_rep.astype(np.float64)).all()
        p = det.sigmoid((a + bh_rep).astype(np.float32))
        h = (uniforms(seed, STREAM_H, rid, cL + k, Hn) < p).astype(np.float32)
        t = ascending_sum(h, Wt)
        a = b64[k] * t
        assert exact_tm(a, bv_rep.astype(np.float64)).all()
        p = det.sigmoid((a + bv_rep).astype(np.float32))
        x = (uniforms(seed, STREAM_V, rid, cL + k, D) < p).astype(np.uint8)
    return x, lw


# ------------------------------------------------------------------------------------------------
# 1. W = 0: every increment is exactly 0, the estimate is log Z_0
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
def test_zero_weights_give_log_z0(ops, N, D, Hn, bcast):
    _, bh, bv = problem(N, D, Hn, bcast, 1)
    W = np.zeros((D, Hn), np.float32)
    log_z, log_w, _, stats = run_raise(ops, W, bh, bv, data_rows(N, D, 1), np.linspace(0, 1, 7), 37, 5)
    assert np.all(log_w == 0.0)
    ref = softplus(np.broadcast_to(bv, (N, D)).astype(np.float64)).sum(1) + softplus(np.broadcast_to(bh, (N, Hn)).astype(np.float64)).sum(1)
    np.testing.assert_allclose(log_z, ref, rtol=2e-6)
    np.testing.assert_allclose(stats[:, 0], 37.0, rtol=1e-6)
    assert np.all(stats[:, 1] == 0.0)


# 2. a ladder [0, 1, 1, ..., 1]: L - 1 Gibbs iterations at beta = 1 from the data -- the checker's chain -- then the one weight step
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
@pytest.mark.parametrize("with_ids", [False, True])
def test_beta_one_head_is_the_gibbs_chain(ops, N, D, Hn, bcast, with_ids):
    W, bh, bv = problem(N, D, Hn, bcast, 2)
    v = data_rows(N, D, 2)
    S, L, seed = 40, 6, 11
    ids = np.array([70001 + 3 * n for n in range(N)], np.uint32) if with_ids else np.arange(5, 5 + N, dtype=np.uint32)
    _, log_w, v_out, _ = run_raise(ops, W, bh, bv, v, [0.0] + [1.0] * (L - 1), S, seed, row0=5, row_ids=ids if with_ids else None)
    rid, cL = chain_index(N, S, L, ids)
    bh_rep, bv_rep = rows_of(bh, N, S), rows_of(bv, N, S)
    order = range(L - 1, 0, -1)                                                # execution order: k = L-1 .. 1
    u_h = np.stack([uniforms(seed, STREAM_H, rid, cL + k, Hn) for k in order])
    u_v = np.stack([uniforms(seed, STREAM_V, rid, cL + k, D) for k in order])
    _, x = det.rbm_gibbs(np.repeat(v, S, axis=0), W, bh_rep, bv_rep, L - 1, u_h, u_v)
    np.testing.assert_array_equal(v_out.reshape(N * S, D), x)
    s = x.astype(np.float64) @ W.astype(np.float64)
    ref = -(softplus(bh_rep + s) - softplus(bh_rep.astype(np.float64))).sum(1)
    np.testing.assert_allclose(log_w.reshape(-1), ref, rtol=1e-5, atol=1e-5)


# 3. a general dyadic ladder: every final state bit for bit, the log weights against float64 increments along the same states
@pytest.mark.parametrize("N,D,Hn,bcast,L,S", [(1, 88, 256, False, 1025, 64), (2, 30, 100, True, 129, 40), (1, 440, 256, False, 33, 9),
                                              (2, 10, 8, False, 257, 24)])
def test_dyadic_ladder_bit_for_bit(ops, N, D, Hn, bcast, L, S):
    W, bh, bv = problem(N, D, Hn, bcast, 3)
    v = data_rows(N, D, 3)
    betas = np.arange(L, dtype=np.float64) / (L - 1)             # multiples of 1/1024 or coarser: exact in float32
    seed = 2024
    _, log_w, v_out, _ = run_raise(ops, W, bh, bv, v, betas, S, seed, row0=9)
    rid, cL = chain_index(N, S, L, np.arange(9, 9 + N))
    x, lw = restated_chains(W, rows_of(bh, N, S).astype(np.float64), rows_of(bv, N, S).astype(np.float64), np.repeat(v, S, axis=0), betas, seed,
                            rid, cL)
    np.testing.assert_array_equal(v_out.reshape(N * S, D), x)
    np.testing.assert_allclose(log_w.reshape(-1), lw, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(lw).max()))


# 4. the estimate against exact enumeration, arbitrary data
def exact_log_z_hidden(W, bh, bv):
    Hn = W.shape[1]
    h = np.array(list(itertools.product([0.0, 1.0], repeat=Hn)))
    t = (h @ bh.T).T + softplus(bv[:, None, :] + (h @ W.T)[None]).sum(2)          # [N, 2^Hn]
    m = t.max(1, keepdims=True)
    return (m + np.log(np.exp(t - m).sum(1, keepdims=True)))[:, 0]


def visible_log_terms(W, bh, bv):
    """log of the unnormalised p(v) of every visible vector, per row: (v [2^D, D], terms [N, 2^D])."""
    D = W.shape[0]
    v = np.array(list(itertools.product([0.0, 1.0], repeat=D)))
    s = v @ W
    return v, np.stack([v @ bv[n] + softplus(bh[n][None, :] + s).sum(1) for n in range(bh.shape[0])])


def exact_log_z_visible(W, bh, bv):
    t = visible_log_terms(W, bh, bv)[1]
    m = t.max(1, keepdims=True)
    return (m + np.log(np.exp(t - m).sum(1, keepdims=True)))[:, 0]


@pytest.mark.parametrize("D,Hn,N,enum,scale", [(10, 8, 64, "h", 0.5), (88, 12, 64, "h", 0.3), (16, 256, 24, "v", 0.15)])
def test_estimate_matches_exact_enumeration(ops, D, Hn, N, enum, scale):
    R = np.random.default_rng(D * 1000 + Hn)
    W = (R.standard_normal((D, Hn)) * scale).astype(np.float32)
    bh = (R.standard_normal((N, Hn)) * 0.5).astype(np.float32)
    bv = (R.standard_normal((N, D)) * 0.5).astype(np.float32)
    log_z, _, _, stats = run_raise(ops, W, bh, bv, data_rows(N, D, 4), np.arange(2000) / 1999.0, 256, 77)
    f = exact_log_z_hidden if enum == "h" else exact_log_z_visible
    ref = f(W.astype(np.float64), bh.astype(np.float64), bv.astype(np.float64))
    err = np.abs(log_z - ref)
    print("reverse AIS against enumeration: max error", err.max(), "max stderr", stats[:, 1].max(), "min ESS", stats[:, 0].min())
    assert np.all(err <= np.maximum(0.02, 4 * stats[:, 1])), (err.max(), stats[:, 1].max(), stats[:, 0].min())


# 5. the direction of the two biases: data drawn exactly from each row's own RBM, a ladder far too short
def test_biases_point_in_opposite_directions(ops):
    """mean over rows of (log Z^ - exact) is above +5 standard errors for the reverse estimate and below -5 for the forward one at L = 2, and
    still above +5 for the reverse one at L = 5 (uniform).  How far a two-rung ladder misses depends on the one shared W that the seed
    draws: in a float64 NumPy restatement of both estimators the margins over NumPy seeds 0..9 ranged from 4 to 43 standard errors, so the
    seed here is the first of them whose three margins all exceeded 10 (twice the bound) under each of three chain seeds -- seed 8: +35..43,
    -17..19, +12..14.5, means +3.4, -3.4, +0.77."""
    D, Hn, N, S = 10, 8, 256, 16
    R = np.random.default_rng(8)
    W = (R.standard_normal((D, Hn)) * 1.5).astype(np.float32)
    bh = (R.standard_normal((N, Hn)) * 0.5).astype(np.float32)
    bv = (R.standard_normal((N, D)) * 0.5).astype(np.float32)
    states, t = visible_log_terms(W.astype(np.float64), bh.astype(np.float64), bv.astype(np.float64))
    m = t.max(1, keepdims=True)
    exact = (m + np.log(np.exp(t - m).sum(1, keepdims=True)))[:, 0]
    cdf = np.cumsum(np.exp(t - exact[:, None]), axis=1)                        # each row's exact distribution over the 2^D vectors
    pick = np.minimum((cdf < R.random((N, 1))).sum(1), len(states) - 1)
    v = states[pick].astype(np.uint8)

    def margin(log_z):
        d = log_z.astype(np.float64) - exact
        return d.mean() / (d.std(ddof=1) / np.sqrt(N))

    rev2 = margin(run_raise(ops, W, bh, bv, v, [0.0, 1.0], S, 3)[0])
    ais2 = margin(run_ais(ops, W, bh, bv, N, [0.0, 1.0], S, 3)[0])
    rev5 = margin(run_raise(ops, W, bh, bv, v, np.arange(5) / 4.0, S, 3)[0])
    print("bias margins in standard errors: reverse L=2", rev2, "forward L=2", ais2, "reverse L=5", rev5)
    assert rev2 > 5 and ais2 < -5 and rev5 > 5, (rev2, ais2, rev5)


# 6. counters: halves with their row ids, S-prefix, seeds, and no uniform shared with the forward chains
@pytest.mark.parametrize("N,D,Hn,bcast", [FORMS[0], FORMS[3], FORMS[4]])
def test_invariances_and_determinism(ops, N, D, Hn, bcast):
    N = 4
    W, bh, bv = problem(N, D, Hn, bcast, 4)
    x = data_rows(N, D, 6)
    betas = np.arange(50) / 49.0
    z, w, v, st = run_raise(ops, W, bh, bv, x, betas, 64, 31, row0=100)
    h = N // 2
    pieces = [run_raise(ops, W, bh if bcast else bh[a:b], bv if bcast else bv[a:b], x[a:b], betas, 64, 31, row_ids=np.arange(100 + a, 100 + b))
              for a, b in ((0, h), (h, N))]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in pieces]), z)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in pieces]), w)
    np.testing.assert_array_equal(np.concatenate([p[2] for p in pieces]), v)
    z2, w2, v2, _ = run_raise(ops, W, bh, bv, x, betas, 128, 31, row0=100)
    np.testing.assert_array_equal(w2[:, :64], w)
    np.testing.assert_array_equal(v2[:, :64], v)
    z3, w3, v3, st3 = run_raise(ops, W, bh, bv, x, betas, 64, 31, row0=100)
    assert z3.tobytes() == z.tobytes() and w3.tobytes() == w.tobytes() and v3.tobytes() == v.tobytes() and st3.tobytes() == st.tobytes()
    z4, w4, _, _ = run_raise(ops, W, bh, bv, x, betas, 64, 32, row0=100)
    assert not np.array_equal(w4, w)
    vf = run_ais(ops, W, bh, bv, N, betas, 64, 31, row0=100)[2]
    assert not np.array_equal(vf, v)


# 7. the two forms
def test_forms_agree_on_the_chains(ops, monkeypatch):
    """The streaming form reaches the matrix-core form's states at a shape both take (the same draws; log w may differ in its last bits)."""
    W, bh, bv = problem(2, 88, 256, False, 5)
    x = data_rows(2, 88, 7)
    betas = np.arange(65) / 64.0
    z, w, v, _ = run_raise(ops, W, bh, bv, x, betas, 16, 3)
    monkeypatch.setenv("MNN_RBM_NO_MFMA", "1")
    zs, ws, vs, _ = run_raise(ops, W, bh, bv, x, betas, 16, 3)
    np.testing.assert_array_equal(vs, v)
    np.testing.assert_allclose(ws, w, rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------------------------------------
# model level
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


# 8.
def test_rnn_rbm_reverse_estimate_matches_exact_nll(ops):
    from multinn_amd.generators import NllEstimate
    g = tiny_rbm()
    x = sequences()
    est = g.estimate_nll(x, num_chains=256, num_betas=2000, method="raise")
    assert isinstance(est, NllEstimate)
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
    assert est.ess > 1 and abs(est.mean - nll.mean()) < 1e-5


def same_bytes(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# 9.
def test_both_is_the_two_single_method_calls(ops):
    from multinn_amd.generators import NllBracket
    g = tiny_rbm()
    x = sequences()
    kw = dict(num_chains=32, num_betas=100, seed=9)
    both = g.estimate_nll(x, method="both", **kw)
    lower, upper = g.estimate_nll(x, method="ais", **kw), g.estimate_nll(x, method="raise", **kw)
    assert isinstance(both, NllBracket)
    assert same_bytes(both.lower.nll, lower.nll) and same_bytes(both.upper.nll, upper.nll)
    assert same_bytes(lower.nll, g.estimate_nll(x, **kw).nll)                       # "ais" is the call without a method
    assert not same_bytes(lower.log_z, upper.log_z)
    assert both.gap == both.upper.mean - both.lower.mean == upper.mean - lower.mean
    assert both.gap_stderr == (lower.stderr ** 2 + upper.stderr ** 2) ** 0.5 > 0
    lengths = torch.tensor([5, 2, 4], dtype=torch.int32)
    rag = g.estimate_nll(x, lengths=lengths, method="both", **kw)
    keep = (torch.arange(5)[None, :] < lengths[:, None]).reshape(-1).to(DEV)
    for side, full in ((rag.lower, lower), (rag.upper, upper)):
        assert side.nll.numel() == 11
        assert torch.equal(side.log_z, full.log_z[keep])                             # same bias rows, targets and row ids: the same chains
        torch.testing.assert_close(side.nll, full.nll[keep], rtol=1e-6, atol=1e-5)


def mode_config(P=10, tracks=("Piano", "Guitar")):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 24, "highest": 24 + P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def mode_params(mode, gen):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
            "generator": {"type": gen, "num_hidden": 8, "num_hidden_rnn": [32, 32], "feedback": [16]}}


def mode_batch(seed, B=3, T=4):
    return dev((np.random.default_rng(seed).random((B, T, 10, 2)) < 0.3).astype(np.uint8))


# 10.
def test_jamming_sides_are_the_sums_over_generators(ops):
    from multinn_amd import MultINN
    from multinn_amd.generators import NllEstimate
    m = MultINN(mode_config(), mode_params("jamming", "RBM"), mode="jamming", precision="fp32")
    x = mode_batch(1)
    both = m.estimate_nll(x, num_chains=32, num_betas=50, method="both")
    parts = [g._nll_rows_built(num_chains=32, num_betas=50, method="both") for g in m._generators]
    assert len(parts) == 2 and both.lower.nll.numel() == both.upper.nll.numel() == 12
    for side, ps in ((both.lower, [p.lower for p in parts]), (both.upper, [p.upper for p in parts])):
        assert torch.equal(side.nll, ps[0].nll + ps[1].nll) and torch.equal(side.nll, NllEstimate.total(ps).nll)
        assert torch.equal(side.log_z, ps[0].log_z + ps[1].log_z)
    up = m.estimate_nll(x, num_chains=32, num_betas=50, method="raise")
    assert same_bytes(up.nll, both.upper.nll) and same_bytes(m.estimate_nll(x, num_chains=32, num_betas=50).nll, both.lower.nll)
    assert both.gap == both.upper.mean - both.lower.mean


def test_composer_multirbm_sides_sum_the_tracks_with_their_seeds(ops):
    from multinn_amd import MultINN
    from multinn_amd import ops as o
    m = MultINN(mode_config(), mode_params("composer", "MultiRBM"), mode="composer", precision="fp32")
    x = mode_batch(4)
    B, T, seed = 3, 4, 40
    both = m.estimate_nll(x, num_chains=32, num_betas=50, seed=seed, method="both")
    g = m._generators[0]
    assert len(m._generators) == 1 and len(g._rbms) == 2
    idx = g._idx()
    bh_t, bv_t = g._split(g._ctx["out"])
    ids = torch.tensor([t * 65536 + g.row0 + b for b in range(B) for t in range(T)], dtype=torch.int32, device=DEV)   # API order
    lower = upper = 0
    for k, r in enumerate(g._rbms):
        bh, bv, tgt = bh_t[k][idx].contiguous(), bv_t[k][idx].contiguous(), g._ctx["tgt"][k][idx].contiguous()
        F = o.rbm_free_energy(tgt, r.W, bh, bv, torch.empty(B * T, device=DEV))
        lower = lower + (F + r.log_partition(bh, bv, 32, 50, None, seed + k, row_ids=ids))
        upper = upper + (F + r.log_partition_reverse(tgt, bh, bv, 32, 50, None, seed + k, row_ids=ids))
    assert torch.equal(both.lower.nll, lower) and torch.equal(both.upper.nll, upper)
    assert same_bytes(m.estimate_nll(x, num_chains=32, num_betas=50, seed=seed, method="raise").nll, both.upper.nll)


def test_nade_rows_are_exact_under_every_method(ops):
    from multinn_amd.generators import RnnNade, NllBracket
    g = RnnNade(10, 8, [32, 32], precision="fp32", seed=3)
    x = sequences(seed=2)
    lengths = torch.tensor([5, 3, 4], dtype=torch.int32, device=DEV)
    for method in ("ais", "raise"):
        est = g.estimate_nll(x, lengths=lengths, method=method)
        assert est.stderr == 0.0 and est.log_z is None and est.nll.numel() == 12
        assert torch.equal(est.nll, g.log_probs)                                     # the eval loss rows of the build it ran
    both = g.estimate_nll(x, lengths=lengths, method="both")
    assert isinstance(both, NllBracket) and both.lower is both.upper and both.gap == 0.0 and both.gap_stderr == 0.0
    assert torch.equal(both.lower.nll, g.log_probs) and both.lower.stderr == 0.0


# 11.
def test_driver_evaluate_reports_raise_and_bracket(ops):
    from multinn_amd import MultINN, driver
    m = MultINN(mode_config(), mode_params("jamming", "RBM"), mode="jamming", precision="fp32")
    R = np.random.default_rng(3)
    X = (R.random((4, 8, 10, 2)) < 0.3).astype(np.uint8)
    lengths = np.array([8, 8, 6, 8])
    loss = driver.evaluate(m, X, lengths, 2, 8)
    kw = dict(num_chains=16, num_betas=40)
    lo = driver.evaluate(m, X, lengths, 2, 8, nll="ais", ais=kw)
    up = driver.evaluate(m, X, lengths, 2, 8, nll="raise", ais=kw)
    br = driver.evaluate(m, X, lengths, 2, 8, nll="bracket", ais=kw)
    assert np.isfinite(up) and up > 0 and up != lo
    assert set(br) == {"lower", "upper", "gap"} and br["lower"] == lo and br["upper"] == up and br["gap"] == up - lo
    assert driver.evaluate(m, X, lengths, 2, 8) == loss == driver.evaluate(m, X, lengths, 2, 8, nll="loss")
