"""Conditional NLL on the device: clamped AIS and clamped reverse AIS (ops.rbm_ais(given=), ops.rbm_raise_given, RBM.log_partition /
log_partition_reverse(given=), estimate_nll(given_mask=), driver.evaluate(given_mask=)).  The checking method of tests/test_gpu_ais.py and
tests/test_gpu_raise.py carried over whole, with their helpers: all codes free against the unconditioned call byte for byte, each kernel
form against the deterministic checker and a float32 restatement bit for bit, the log weights against float64, the estimates against exact
enumeration of the clamped sum, the direction of the two biases, and the model-level API.

The checker needs no change: a clamped iteration is det.rbm_gibbs with the visible uniform -1 where the code is 1 and 2 where it is 0
(u < p, p in [0, 1]); every free visible reads the uniform of the unconditioned chain (tests/test_gpu_conditional_rbm.py)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_ais as TA     # noqa: E402
import test_gpu_raise as TR   # noqa: E402
from oracle import det        # noqa: E402

DEV = "cuda:0"
FREE = 255
FORMS = TA.FORMS
DIRECTIONS = ["ais", "raise"]
STREAMS = {"ais": (TA.STREAM_H, TA.STREAM_V), "raise": (TR.STREAM_H, TR.STREAM_V)}
dev, softplus, problem, chain_index, rows_of, uniforms, data_rows = TA.dev, TA.softplus, TA.problem, TA.chain_index, TA.rows_of, TR.uniforms, TR.data_rows


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def random_codes(R, shape, density=0.4):
    vals = (R.random(shape) < 0.3).astype(np.uint8)
    return np.where(R.random(shape) < density, vals, FREE).astype(np.uint8)


def some_clamped(R, N, D, n_clamped):
    """n_clamped cells of every row, picked by a permutation, at random values."""
    vals = (R.random((N, D)) < 0.3).astype(np.uint8)
    codes = np.full((N, D), FREE, np.uint8)
    for n in range(N):
        cells = R.permutation(D)[:n_clamped]
        codes[n, cells] = vals[n, cells]
    return codes


def clamp(codes, x):
    return np.where(codes != FREE, codes, x).astype(np.uint8)


def clamp_u(u, codes):
    """The visible uniforms that make det.rbm_gibbs emit the clamped values."""
    return np.where(codes == 1, np.float32(-1.0), np.where(codes == 0, np.float32(2.0), u)).astype(np.float32)


def run(ops, direction, W, bh, bv, v, betas, S, seed, row0=0, row_ids=None, given=None, N=None, free_entry=False):
    """One launch of either direction -> (log_z, log_w, v_out, stats).  given: codes [N, D] (a device tensor is passed as it is), or None;
    free_entry: the call without the argument (ops.rbm_ais / ops.rbm_raise as they were)."""
    D = W.shape[0]
    N = N or max(bh.shape[0], bv.shape[0], 0 if v is None else v.shape[0], 0 if given is None else given.shape[0])
    out = TR.outputs(N, S, D)
    ids = None if row_ids is None else dev(np.asarray(row_ids, np.int32))
    g = given if given is None or torch.is_tensor(given) else dev(given)
    b = dev(np.asarray(betas, np.float32))
    if direction == "ais":
        if free_entry:
            ops.rbm_ais(dev(W), dev(bh), dev(bv), b, S, seed, row0, ids, *out)
        else:
            ops.rbm_ais(dev(W), dev(bh), dev(bv), b, S, seed, row0, ids, *out, given=g)
    elif free_entry:
        ops.rbm_raise(dev(W), dev(bh), dev(bv), dev(v), b, S, seed, row0, ids, *out)
    else:
        ops.rbm_raise_given(dev(W), dev(bh), dev(bv), dev(v), g, b, S, seed, row0, ids, *out)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def clamped_log_z0(bh, bv, codes):
    """sum_F softplus(bv_d) + sum_G bv_d c_d + sum_j softplus(bh_j) in float64, per row."""
    N = codes.shape[0]
    bv = np.broadcast_to(bv, (N, bv.shape[1])).astype(np.float64)
    bh = np.broadcast_to(bh, (N, bh.shape[1])).astype(np.float64)
    return np.where(codes == FREE, softplus(bv), bv * (codes == 1)).sum(1) + softplus(bh).sum(1)


# ------------------------------------------------------------------------------------------------
# 1. every code free: the unconditioned call, byte for byte
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
def test_all_codes_free_is_the_call_without_given(ops, N, D, Hn, bcast, direction):
    W, bh, bv = problem(N, D, Hn, bcast, 11)
    v = data_rows(N, D, 11)
    betas, S, seed = np.arange(17) / 16.0, 40, 21
    free = run(ops, direction, W, bh, bv, v, betas, S, seed, row0=3, N=N, free_entry=True)
    none = run(ops, direction, W, bh, bv, v, betas, S, seed, row0=3, N=N)                  # given=None: the same entry
    wide = torch.full((N, D + 5), FREE, dtype=torch.uint8, device=DEV)                   # a row stride above D is read in place
    wide[:, D:] = 0
    for got in (none, run(ops, direction, W, bh, bv, v, betas, S, seed, row0=3, given=np.full((N, D), FREE, np.uint8)),
                run(ops, direction, W, bh, bv, v, betas, S, seed, row0=3, given=wide[:, :D])):
        for a, b in zip(got, free):
            assert a.tobytes() == b.tobytes()


# 2. W = 0: the clamped base distribution is the clamped target
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
def test_zero_weights_give_the_clamped_log_z0(ops, N, D, Hn, bcast, direction):
    _, bh, bv = problem(N, D, Hn, bcast, 1)
    W = np.zeros((D, Hn), np.float32)
    codes = random_codes(np.random.default_rng(5), (N, D))
    assert 0.25 < (codes != FREE).mean() < 0.55 and (codes == 1).any() and (codes == 0).any()
    log_z, log_w, v_out, stats = run(ops, direction, W, bh, bv, data_rows(N, D, 1), np.linspace(0, 1, 7), 37, 5, given=codes)
    assert np.all(log_w == 0.0)
    np.testing.assert_allclose(log_z, clamped_log_z0(bh, bv, codes), rtol=2e-6)
    np.testing.assert_allclose(stats[:, 0], 37.0, rtol=1e-6)
    assert np.all(stats[:, 1] == 0.0)
    held = np.broadcast_to((codes != FREE)[:, None, :], v_out.shape)
    np.testing.assert_array_equal(v_out[held], np.broadcast_to(codes[:, None, :], v_out.shape)[held])


# 3. a ladder [0, 1, 1, ..., 1]: Gibbs iterations at beta = 1 -- the checker's clamped chain
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
@pytest.mark.parametrize("with_ids", [False, True])
def test_beta_one_rungs_are_the_clamped_gibbs_chain(ops, N, D, Hn, bcast, with_ids, direction):
    """Forward: the clamped base draw, one weight step, L - 2 clamped iterations.  Reverse: L - 1 clamped iterations from the clamped data
    row, then the one weight step."""
    W, bh, bv = problem(N, D, Hn, bcast, 2)
    x0 = data_rows(N, D, 2)
    codes = random_codes(np.random.default_rng(6), (N, D))
    S, L, seed = 40, 6, 11
    sh, sv = STREAMS[direction]
    ids = np.array([70001 + 3 * n for n in range(N)], np.uint32) if with_ids else np.arange(5, 5 + N, dtype=np.uint32)
    _, log_w, v_out, _ = run(ops, direction, W, bh, bv, x0, [0.0] + [1.0] * (L - 1), S, seed, row0=5, row_ids=ids if with_ids else None, given=codes)
    rid, cL = chain_index(N, S, L, ids)
    bh_rep, bv_rep, c_rep = rows_of(bh, N, S), rows_of(bv, N, S), np.repeat(codes, S, axis=0)
    if direction == "ais":
        start = clamp(c_rep, (uniforms(seed, sv, rid, cL, D) < det.sigmoid(bv_rep)).astype(np.uint8))
        order = range(1, L - 1)
    else:
        start = clamp(c_rep, np.repeat(x0, S, axis=0))
        order = range(L - 1, 0, -1)
    u_h = np.stack([uniforms(seed, sh, rid, cL + k, Hn) for k in order])
    u_v = np.stack([clamp_u(uniforms(seed, sv, rid, cL + k, D), c_rep) for k in order])
    _, end = det.rbm_gibbs(start, W, bh_rep, bv_rep, len(order), u_h, u_v)
    np.testing.assert_array_equal(v_out.reshape(N * S, D), end)
    assert np.array_equal(end[c_rep != FREE], c_rep[c_rep != FREE])
    s = (start if direction == "ais" else end).astype(np.float64) @ W.astype(np.float64)         # the state of the one weight step
    ref = (softplus(bh_rep + s) - softplus(bh_rep.astype(np.float64))).sum(1) * (1.0 if direction == "ais" else -1.0)
    np.testing.assert_allclose(log_w.reshape(-1), ref, rtol=1e-5, atol=1e-5)


# 4. a general dyadic ladder: every final state bit for bit, the log weights against float64 increments along the same states
def restated_clamped_chains(direction, W, bh_rep, bv_rep, x0, codes, betas, seed, rid, cL):
    """test_gpu_ais.restated_chains / test_gpu_raise.restated_chains with the clamp inserted: the float32 chains (ascending float32 sums,
    fmaf(beta, s, b) asserted exact in float64 on the dyadic ladder, det sigmoid, u < p) with every clamped cell held at its code -- in the
    base draw (forward), the start from the data row (reverse) and after each visible phase.  Returns (final state, float64 log w)."""
    L = len(betas)
    D, Hn = W.shape
    sh, sv = STREAMS[direction]
    Wt = np.ascontiguousarray(W.T)
    b64 = np.asarray(betas, np.float32).astype(np.float64)
    bh64, bv64 = bh_rep.astype(np.float64), bv_rep.astype(np.float64)
    lw = np.zeros(len(rid))
    if direction == "ais":
        x = clamp(codes, (uniforms(seed, sv, rid, cL, D) < det.sigmoid(bv_rep)).astype(np.uint8))
        rungs = range(1, L)
    else:
        x = clamp(codes, x0)
        rungs = range(L - 1, -1, -1)
    for k in rungs:
        s = TR.ascending_sum(x, W)
        if direction == "ais":
            lw += (softplus(bh64 + b64[k] * s) - softplus(bh64 + b64[k - 1] * s)).sum(1)
            if k == L - 1:
                break
        else:
            if k < L - 1:
                lw -= (softplus(bh64 + b64[k + 1] * s) - softplus(bh64 + b64[k] * s)).sum(1)
            if k == 0:
                break
        a = b64[k] * s
        assert TR.exact_tm(a, bh64).all()
        h = (uniforms(seed, sh, rid, cL + k, Hn) < det.sigmoid((a + bh64).astype(np.float32))).astype(np.float32)
        a = b64[k] * TR.ascending_sum(h, Wt)
        assert TR.exact_tm(a, bv64).all()
        x = clamp(codes, (uniforms(seed, sv, rid, cL + k, D) < det.sigmoid((a + bv64).astype(np.float32))).astype(np.uint8))
    return x, lw


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("N,D,Hn,bcast,L,S", [(1, 88, 256, False, 1025, 64), (2, 30, 100, True, 129, 40), (1, 440, 256, False, 33, 9),
                                              (2, 10, 8, False, 257, 24)])
def test_dyadic_ladder_bit_for_bit(ops, N, D, Hn, bcast, L, S, direction):
    W, bh, bv = problem(N, D, Hn, bcast, 3)
    x0 = data_rows(N, D, 3)
    codes = random_codes(np.random.default_rng(7), (N, D))
    betas = np.arange(L, dtype=np.float64) / (L - 1)             # multiples of 1/1024 or coarser: exact in float32
    seed = 2024
    _, log_w, v_out, _ = run(ops, direction, W, bh, bv, x0, betas, S, seed, row0=9, given=codes)
    rid, cL = chain_index(N, S, L, np.arange(9, 9 + N))
    x, lw = restated_clamped_chains(direction, W, rows_of(bh, N, S), rows_of(bv, N, S), np.repeat(x0, S, axis=0), np.repeat(codes, S, axis=0),
                                    betas, seed, rid, cL)
    np.testing.assert_array_equal(v_out.reshape(N * S, D), x)
    np.testing.assert_allclose(log_w.reshape(-1), lw, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(lw).max()))


# 5. the estimates against exact enumeration of the clamped sum
def logsumexp_rows(t):
    m = t.max(1, keepdims=True)
    return (m + np.log(np.exp(t - m).sum(1, keepdims=True)))[:, 0]


def exact_clamped_log_z_hidden(W, bh, bv, codes):
    """Over the hidden vectors: per h, bh.h + sum_G c_d (bv_d + (W h)_d) + sum_F softplus(bv_d + (W h)_d)."""
    h = np.array(list(itertools.product([0.0, 1.0], repeat=W.shape[1])))
    a = bv[:, None, :] + (h @ W.T)[None]                                          # [N, 2^Hn, D]
    c = codes[:, None, :]
    return logsumexp_rows((h @ bh.T).T + np.where(c == FREE, softplus(a), a * (c == 1)).sum(2))


def clamped_visible_terms(W, bh, bv, codes):
    """log of the unnormalised p(v) over all 2^D visible vectors in itertools.product order, -inf where v disagrees with the row's codes:
    (v [2^D, D], terms [N, 2^D])."""
    v, t = TR.visible_log_terms(W, bh, bv)
    agree = ((codes[:, None, :] == FREE) | (codes[:, None, :] == v[None].astype(np.uint8))).all(2)
    return v, np.where(agree, t, -np.inf)


def exact_clamped_log_z_visible(W, bh, bv, codes):
    """Over the free visibles of each row (the clamped ones at their codes)."""
    out = []
    for n in range(codes.shape[0]):
        free = np.flatnonzero(codes[n] == FREE)
        v = np.tile((codes[n] == 1).astype(np.float64), (2 ** len(free), 1))
        v[:, free] = np.array(list(itertools.product([0.0, 1.0], repeat=len(free))))
        out.append(logsumexp_rows((v @ bv[n] + softplus(bh[n][None, :] + v @ W).sum(1))[None])[0])
    return np.array(out)


def test_the_two_enumerations_agree():
    R = np.random.default_rng(0)
    W, bh, bv = R.standard_normal((7, 5)), R.standard_normal((3, 5)), R.standard_normal((3, 7))
    codes = some_clamped(R, 3, 7, 3)
    a, b = exact_clamped_log_z_hidden(W, bh, bv, codes), exact_clamped_log_z_visible(W, bh, bv, codes)
    c = logsumexp_rows(clamped_visible_terms(W, bh, bv, codes)[1])
    np.testing.assert_allclose(a, b, rtol=1e-12)
    np.testing.assert_allclose(a, c, rtol=1e-12)


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("D,Hn,N,n_clamped,enum,scale", [(10, 8, 64, 4, "h", 0.5), (16, 12, 32, 6, "h", 0.5), (16, 256, 24, 6, "v", 0.15)])
def test_estimate_matches_exact_enumeration(ops, D, Hn, N, n_clamped, enum, scale, direction):
    R = np.random.default_rng(D * 1000 + Hn)
    W = (R.standard_normal((D, Hn)) * scale).astype(np.float32)
    bh = (R.standard_normal((N, Hn)) * 0.5).astype(np.float32)
    bv = (R.standard_normal((N, D)) * 0.5).astype(np.float32)
    codes = some_clamped(R, N, D, n_clamped)
    log_z, _, _, stats = run(ops, direction, W, bh, bv, data_rows(N, D, 4), np.arange(2000) / 1999.0, 256, 77, given=codes)
    f = exact_clamped_log_z_hidden if enum == "h" else exact_clamped_log_z_visible
    ref = f(W.astype(np.float64), bh.astype(np.float64), bv.astype(np.float64), codes)
    err = np.abs(log_z - ref)
    print(direction, "clamped against enumeration: max error", err.max(), "max stderr", stats[:, 1].max(), "min ESS", stats[:, 0].min())
    assert np.all(err <= np.maximum(0.02, 4 * stats[:, 1])), (err.max(), stats[:, 1].max(), stats[:, 0].min())


# 6. fully clamped rows among free rows
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
def test_fully_clamped_rows_among_free_rows(ops, N, D, Hn, bcast, direction):
    N = 4
    W, bh, bv = problem(N, D, Hn, bcast, 8)
    x0 = data_rows(N, D, 8)
    R = np.random.default_rng(9)
    codes = random_codes(R, (N, D))
    full = [1, 3]
    codes[full] = (R.random((2, D)) < 0.3).astype(np.uint8)
    betas, S, seed = np.arange(33) / 32.0, 40, 13
    ids = np.arange(200, 200 + N)
    log_z, log_w, v_out, stats = run(ops, direction, W, bh, bv, x0, betas, S, seed, row_ids=ids, given=codes)
    lw = log_w[full]
    assert np.all(lw.view(np.uint32) == lw.view(np.uint32)[:, :1])                       # one state, one weight: every chain the same bits
    s = codes[full].astype(np.float64) @ W.astype(np.float64)
    b = np.broadcast_to(bh, (N, Hn))[full].astype(np.float64)
    ref = (softplus(b + s) - softplus(b)).sum(1) * (1.0 if direction == "ais" else -1.0)
    np.testing.assert_allclose(lw[:, 0], ref, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(ref).max()))
    assert np.all(stats[full, 0] == S) and np.all(stats[full, 1] == 0.0)
    np.testing.assert_array_equal(v_out[full], np.broadcast_to(codes[full][:, None, :], (2, S, D)))
    rest = [0, 2]
    sub = lambda a: a if a.shape[0] == 1 else a[rest]
    alone = run(ops, direction, W, sub(bh), sub(bv), x0[rest], betas, S, seed, row_ids=ids[rest], given=codes[rest])
    for a, b in zip((log_z, log_w, v_out, stats), alone):
        assert a[rest].tobytes() == b.tobytes()


# 7. the two forms
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_forms_agree_on_the_clamped_chains(ops, monkeypatch, direction):
    """The streaming form reaches the matrix-core form's states at a shape both take (the same draws; log w may differ in its last bits)."""
    W, bh, bv = problem(2, 88, 256, False, 5)
    x0 = data_rows(2, 88, 7)
    codes = random_codes(np.random.default_rng(10), (2, 88))
    betas = np.arange(65) / 64.0
    z, w, v, _ = run(ops, direction, W, bh, bv, x0, betas, 16, 3, given=codes)
    monkeypatch.setenv("MNN_RBM_NO_MFMA", "1")
    zs, ws, vs, _ = run(ops, direction, W, bh, bv, x0, betas, 16, 3, given=codes)
    np.testing.assert_array_equal(vs, v)
    np.testing.assert_allclose(ws, w, rtol=1e-5, atol=1e-4)


# 8. the direction of the two biases under a clamp
def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


def clamped_f64(direction, W, bh, bv, v, codes, betas, S, rng):
    """The float64 NumPy restatement of both clamped estimators over all rows at once, NumPy's generator for the draws -> log Z^_c [N]."""
    N, D = codes.shape
    Hn = W.shape[1]
    L = len(betas)
    held = np.broadcast_to((codes != FREE)[:, None, :], (N, S, D))
    at = np.broadcast_to((codes == 1).astype(np.float64)[:, None, :], (N, S, D))
    bh_, bv_ = bh[:, None, :], bv[:, None, :]
    if direction == "ais":
        x = np.where(held, at, rng.random((N, S, D)) < sigmoid64(bv_))
        rungs = range(1, L)
    else:
        x = np.where(held, at, np.broadcast_to(v.astype(np.float64)[:, None, :], (N, S, D)))
        rungs = range(L - 1, -1, -1)
    lw = np.zeros((N, S))
    for k in rungs:
        s = x @ W
        other = k - 1 if direction == "ais" else min(k + 1, L - 1)
        lw += (softplus(bh_ + betas[k] * s) - softplus(bh_ + betas[other] * s)).sum(2)
        if k == (L - 1 if direction == "ais" else 0):
            break
        h = (rng.random((N, S, Hn)) < sigmoid64(bh_ + betas[k] * s)).astype(np.float64)
        x = np.where(held, at, rng.random((N, S, D)) < sigmoid64(bv_ + betas[k] * (h @ W.T)))
    m = lw.max(1, keepdims=True)
    lme = (m + np.log(np.exp(lw - m).mean(1, keepdims=True)))[:, 0]
    z0 = clamped_log_z0(bh, bv, codes)
    return z0 + lme if direction == "ais" else z0 - lme


def bias_problem():
    """D 10, Hn 8, N 1024: one shared W of scale 1.5, biases of scale 0.5, 4 cells of every row clamped to random values, and each row's free
    cells drawn exactly from its own conditional (inverse CDF over the enumeration)."""
    D, Hn, N = 10, 8, 1024
    R = np.random.default_rng(8)
    W = (R.standard_normal((D, Hn)) * 1.5).astype(np.float32)
    bh = (R.standard_normal((N, Hn)) * 0.5).astype(np.float32)
    bv = (R.standard_normal((N, D)) * 0.5).astype(np.float32)
    g = (R.random((N, D)) < 0.3).astype(np.uint8)
    codes = np.full((N, D), FREE, np.uint8)
    for n in range(N):
        cells = R.permutation(D)[:4]
        codes[n, cells] = g[n, cells]
    states, t = clamped_visible_terms(W.astype(np.float64), bh.astype(np.float64), bv.astype(np.float64), codes)
    exact = logsumexp_rows(t)
    cdf = np.cumsum(np.exp(t - exact[:, None]), axis=1)                        # each row's exact conditional over the 2^D vectors
    pick = np.minimum((cdf < R.random(N)[:, None]).sum(1), len(states) - 1)
    v = states[pick].astype(np.uint8)
    assert np.array_equal(v[codes != FREE], codes[codes != FREE])
    return W, bh, bv, codes, v, exact


def bias_margin(log_z, exact):
    d = log_z.astype(np.float64) - exact
    return d.mean() / (d.std(ddof=1) / np.sqrt(len(d)))


def test_biases_point_in_opposite_directions_under_a_clamp(ops):
    """The method of test_gpu_raise.test_biases_point_in_opposite_directions with 4 of 10 cells clamped: over 1024 rows whose free cells are
    drawn exactly from the row's own conditional, the mean of (log Z^_c - exact) is above +5 standard errors for the reverse estimate and
    below -5 for the forward one at L = 2, and still above +5 for the reverse one at L = 5 (uniform); 16 chains.  The float64 NumPy
    restatement clamped_f64 gave, with default_rng(0 / 1 / 2) for the chains: reverse L = 2 +46.0 / +44.4 / +43.2, forward L = 2 -19.8 /
    -19.2 / -19.0, reverse L = 5 +15.2 / +14.6 / +14.8 (means about +1.75, -1.1, +0.32) -- every margin above twice the bound, which N = 256
    did not give at L = 5 (6 to 8)."""
    W, bh, bv, codes, v, exact = bias_problem()
    S = 16
    rev2 = bias_margin(run(ops, "raise", W, bh, bv, v, [0.0, 1.0], S, 3, given=codes)[0], exact)
    ais2 = bias_margin(run(ops, "ais", W, bh, bv, None, [0.0, 1.0], S, 3, given=codes)[0], exact)
    rev5 = bias_margin(run(ops, "raise", W, bh, bv, v, np.arange(5) / 4.0, S, 3, given=codes)[0], exact)
    print("clamped bias margins in standard errors: reverse L=2", rev2, "forward L=2", ais2, "reverse L=5", rev5)
    assert rev2 > 5 and ais2 < -5 and rev5 > 5, (rev2, ais2, rev5)


# ------------------------------------------------------------------------------------------------
# 9. model level
tiny_rbm, sequences, same_bytes = TR.tiny_rbm, TR.sequences, TR.same_bytes
PATTERN = [True, False, False, True, False, False, True, False, False, True]                 # a [P] mask: pitches 0, 3, 6, 9 given


def model_rows(g, x, D, Hn):
    """(W, bh, bv, v) of the last build's valid rows in API order, float64."""
    out = g._ctx["out"][g._idx()].double().cpu().numpy()
    return g._rbm.W.double().cpu().numpy(), out[:, :Hn], out[:, Hn:Hn + D], x.reshape(-1, D).cpu().numpy().astype(np.float64)


def test_rnn_rbm_conditional_estimate_matches_exact_enumeration(ops):
    from multinn_amd.generators import NllBracket
    g = tiny_rbm()
    x = sequences()
    mask = torch.tensor(PATTERN)
    both = g.estimate_nll(x, given_mask=mask, num_chains=256, num_betas=2000, method="both")
    assert isinstance(both, NllBracket)
    W, bh, bv, v = model_rows(g, x, 10, 8)
    codes = np.where(np.array(PATTERN)[None, :], v, FREE).astype(np.uint8)
    F = -(v * bv).sum(1) - softplus(bh + v @ W).sum(1)
    ref = F + exact_clamped_log_z_hidden(W, bh, bv, codes)
    free = F + TA.exact_log_z_hidden(W, bh, bv)
    assert np.all(ref < free)                                               # fewer cells to pay for
    for est in (both.lower, both.upper):
        nll = est.nll.cpu().numpy()
        assert nll.shape == (15,) and np.isfinite(est.mean)
        np.testing.assert_allclose(est.free_energy.cpu().numpy(), F, rtol=1e-5, atol=1e-4)
        tol = np.maximum(0.02, 4 * est.row_stderr.cpu().numpy())
        assert np.all(np.abs(nll - ref) <= tol), (np.abs(nll - ref).max(), tol.max())
        assert est.ess > 1 and abs(est.mean - nll.mean()) < 1e-5


def test_both_ragged_and_the_trivial_masks(ops, monkeypatch):
    from multinn_amd import ops as o
    g = tiny_rbm()
    x = sequences()
    mask = torch.tensor(PATTERN)
    kw = dict(num_chains=32, num_betas=100, seed=9)
    both = g.estimate_nll(x, method="both", given_mask=mask, **kw)
    lower, upper = g.estimate_nll(x, method="ais", given_mask=mask, **kw), g.estimate_nll(x, method="raise", given_mask=mask, **kw)
    assert same_bytes(both.lower.nll, lower.nll) and same_bytes(both.upper.nll, upper.nll)
    assert same_bytes(lower.nll, g.estimate_nll(x, given_mask=mask, **kw).nll) and not same_bytes(lower.log_z, upper.log_z)
    assert both.gap == upper.mean - lower.mean
    free = g.estimate_nll(x, method="both", **kw)
    assert not same_bytes(free.lower.log_z, lower.log_z) and same_bytes(free.lower.free_energy, lower.free_energy)
    # ragged lengths drop the padding rows
    lengths = torch.tensor([5, 2, 4], dtype=torch.int32)
    rag = g.estimate_nll(x, lengths=lengths, method="both", given_mask=mask, **kw)
    keep = (torch.arange(5)[None, :] < lengths[:, None]).reshape(-1).to(DEV)
    for side, full in ((rag.lower, lower), (rag.upper, upper)):
        assert side.nll.numel() == 11
        assert torch.equal(side.log_z, full.log_z[keep])                             # same bias rows, targets, codes and row ids: the same chains
        torch.testing.assert_close(side.nll, full.nll[keep], rtol=1e-6, atol=1e-5)
    # a mask of any shape that broadcasts: the rows' codes are the targets under it, in the targets' row order
    R = np.random.default_rng(4)
    cells = torch.from_numpy(R.random((3, 5, 10)) < 0.4)
    est = g.estimate_nll(x, given_mask=cells, **kw)
    idx = g._idx()
    out = g._ctx["out"][idx]
    rows = torch.where(cells.to(DEV), x, torch.full_like(x, FREE)).reshape(15, 10)                   # API order: b-major, then t
    ids = torch.tensor([t * 65536 + g.row0 + b for b in range(3) for t in range(5)], dtype=torch.int32, device=DEV)
    direct = g._rbm.log_partition(out[:, :8].contiguous(), out[:, 8:18].contiguous(), 32, 100, None, 9, row_ids=ids, given=rows)
    assert torch.equal(est.log_z, direct)
    # no cell given: the call without a mask; every cell given: zeros, and no chain is run
    for none in (torch.zeros(10, dtype=torch.bool), torch.zeros(3, 5, 10, dtype=torch.bool)):
        e = g.estimate_nll(x, method="both", given_mask=none, **kw)
        assert same_bytes(e.lower.nll, free.lower.nll) and same_bytes(e.upper.nll, free.upper.nll) and same_bytes(e.lower.log_z, free.lower.log_z)

    def no_chains(*a, **k):
        raise AssertionError("a chain was launched for rows with nothing to estimate")
    monkeypatch.setattr(o, "_rbm_anneal", no_chains)
    for method in ("ais", "raise", "both"):
        e = g.estimate_nll(x, lengths=lengths, method=method, given_mask=torch.ones(10, dtype=torch.bool), **kw)
        sides = (e.lower, e.upper) if method == "both" else (e,)
        assert all(s.nll.numel() == 11 and bool((s.nll == 0).all()) and s.mean == 0.0 and s.stderr == 0.0 for s in sides)


# 10. the modes
mode_config, mode_params, mode_batch = TR.mode_config, TR.mode_params, TR.mode_batch
TRACK0 = torch.tensor([True, False])


def test_joint_rbm_conditions_one_track_on_the_other(ops):
    from multinn_amd import MultINN
    m = MultINN(mode_config(), mode_params("joint", "RBM"), mode="joint", precision="fp32")
    x = mode_batch(5)
    both = m.estimate_nll(x, given_mask=TRACK0, num_chains=256, num_betas=2000, method="both")
    g = m._generators[0]
    W, bh, bv, v = model_rows(g, x, 20, 8)                                  # the one RBM over p M + m
    codes = np.where((np.arange(20) % 2 == 0)[None, :], v, FREE).astype(np.uint8)
    F = -(v * bv).sum(1) - softplus(bh + v @ W).sum(1)
    ref = F + exact_clamped_log_z_hidden(W, bh, bv, codes)
    for est in (both.lower, both.upper):
        nll = est.nll.cpu().numpy()
        tol = np.maximum(0.02, 4 * est.row_stderr.cpu().numpy())
        assert nll.shape == (12,) and np.all(np.abs(nll - ref) <= tol), (np.abs(nll - ref).max(), tol.max())


def test_jamming_rbm_a_given_track_adds_nothing(ops):
    from multinn_amd import MultINN
    m = MultINN(mode_config(), mode_params("jamming", "RBM"), mode="jamming", precision="fp32")
    x = mode_batch(1)
    kw = dict(num_chains=32, num_betas=50)
    both = m.estimate_nll(x, given_mask=TRACK0, seed=70, method="both", **kw)
    own = m._generators[1]._nll_rows_built(seed=71, method="both", **kw)             # the free generator's own estimate, seed s + i
    for side, part in ((both.lower, own.lower), (both.upper, own.upper)):
        assert side.nll.numel() == 12 and same_bytes(side.nll, part.nll) and same_bytes(side.log_z, part.log_z)
    free = m.estimate_nll(x, seed=70, method="both", **kw)
    assert free.lower.mean > both.lower.mean                                      # the marginal of one track against the joint of two
    everything = m.estimate_nll(x, given_mask=torch.tensor([True, True]), seed=70, **kw)
    assert everything.nll.numel() == 12 and bool((everything.nll == 0).all())
    # a [P, M] mask: each generator's conditional with its own codes, seeds s + i
    low = (torch.arange(10) < 4)[:, None] & torch.tensor([True, True])
    est = m.estimate_nll(x, given_mask=low, seed=70, **kw)
    codes = torch.where(low.to(DEV), x, torch.full_like(x, FREE))
    parts = [g._nll_rows_built(seed=70 + i, given=(codes[..., i].contiguous(), [False], [True]), **kw) for i, g in enumerate(m._generators)]
    assert torch.equal(est.nll, parts[0].nll + parts[1].nll) and not same_bytes(est.nll, free.lower.nll)


def test_composer_multirbm_conditions_per_track(ops):
    from multinn_amd import MultINN
    from multinn_amd import ops as o
    m = MultINN(mode_config(), mode_params("composer", "MultiRBM"), mode="composer", precision="fp32")
    x = mode_batch(4)
    B, T, seed = 3, 4, 40
    kw = dict(num_chains=32, num_betas=50, seed=seed)
    g = m._generators[0]
    ids = torch.tensor([t * 65536 + g.row0 + b for b in range(B) for t in range(T)], dtype=torch.int32, device=DEV)   # API order
    low = (torch.arange(10) < 4)[:, None] & torch.tensor([False, True])              # track 0 free, the low pitches of track 1 given
    for mask, tracks in ((TRACK0, [1]), (low, [0, 1])):
        both = m.estimate_nll(x, given_mask=mask, method="both", **kw)
        idx = g._idx()
        bh_t, bv_t = g._split(g._ctx["out"])
        codes = torch.where(mask.to(DEV), x, torch.full_like(x, FREE))
        lower = upper = 0
        for k in tracks:
            r = g._rbms[k]
            bh, bv, tgt = bh_t[k][idx].contiguous(), bv_t[k][idx].contiguous(), g._ctx["tgt"][k][idx].contiguous()
            assert torch.equal(tgt, x[..., k].reshape(B * T, 10))
            c = codes[..., k].reshape(B * T, 10).contiguous() if bool(mask.expand(10, 2)[:, k].any()) else None
            F = o.rbm_free_energy(tgt, r.W, bh, bv, torch.empty(B * T, device=DEV))
            lower = lower + (F + r.log_partition(bh, bv, 32, 50, None, seed + k, row_ids=ids, given=c))
            upper = upper + (F + r.log_partition_reverse(tgt, bh, bv, 32, 50, None, seed + k, row_ids=ids, given=c))
        assert torch.equal(both.lower.nll, lower) and torch.equal(both.upper.nll, upper)


def test_nade_modes_take_whole_tracks_or_refuse(ops):
    from multinn_amd import MultINN
    from multinn_amd._lib import MnnUnsupported
    m = MultINN(mode_config(), mode_params("jamming", "NADE"), mode="jamming", precision="fp32")
    x = mode_batch(2)
    lengths = torch.tensor([4, 3, 4], dtype=torch.int32, device=DEV)
    est = m.estimate_nll(x, lengths=lengths, given_mask=TRACK0)
    assert est.stderr == 0.0 and est.log_z is None and est.nll.numel() == 11
    assert torch.equal(est.nll, m._generators[1].log_probs)                          # the free track's exact rows
    free = m.estimate_nll(x, lengths=lengths)
    assert torch.equal(free.nll, m._generators[0].log_probs + m._generators[1].log_probs)
    c = MultINN(mode_config(), mode_params("composer", "NADE"), mode="composer", precision="fp32")
    est = c.estimate_nll(x, lengths=lengths, given_mask=torch.tensor([False, True]))
    assert est.stderr == 0.0 and torch.equal(est.nll, c._generators[0].log_probs[0])
    j = MultINN(mode_config(), mode_params("joint", "NADE"), mode="joint", precision="fp32")
    with pytest.raises(MnnUnsupported, match="not a sum of its conditionals"):
        j.estimate_nll(x, given_mask=TRACK0)
    assert bool((j.estimate_nll(x, given_mask=torch.tensor([True, True])).nll == 0).all())
    assert torch.equal(j.estimate_nll(x, given_mask=torch.tensor([False, False])).nll, j.estimate_nll(x).nll)


# 11.
def test_driver_evaluate_reports_the_conditional_bracket(ops):
    from multinn_amd import MultINN, driver
    m = MultINN(mode_config(), mode_params("joint", "RBM"), mode="joint", precision="fp32")
    R = np.random.default_rng(3)
    X = (R.random((4, 8, 10, 2)) < 0.3).astype(np.uint8)
    lengths = np.array([8, 8, 6, 8])
    kw = dict(num_chains=16, num_betas=40)
    mask = [True, False]
    lo = driver.evaluate(m, X, lengths, 2, 8, nll="ais", ais=kw, given_mask=mask)
    up = driver.evaluate(m, X, lengths, 2, 8, nll="raise", ais=kw, given_mask=np.array(mask))
    br = driver.evaluate(m, X, lengths, 2, 8, nll="bracket", ais=kw, given_mask=torch.tensor(mask))
    assert set(br) == {"lower", "upper", "gap"} and br["lower"] == lo and br["upper"] == up and br["gap"] == up - lo
    assert np.isfinite(lo) and np.isfinite(up) and up != lo
    free = driver.evaluate(m, X, lengths, 2, 8, nll="bracket", ais=kw)
    assert 0 < br["lower"] < free["lower"] and 0 < br["upper"] < free["upper"]        # one track given the other costs less than both
