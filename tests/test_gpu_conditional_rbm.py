"""Conditional generation with RBM generators: the clamped Gibbs chain (ops.rbm_gibbs(..., given=)) in each of its three kernel forms
against the deterministic checker, the forms against one another, the conditional it samples, RnnRBM.generate and the mode classes.

The checker needs no change.  Each iteration of det.rbm_gibbs depends only on the visible state, so a k-step clamped chain is: clamp v0, then
k one-iteration calls with the visible uniforms u = -1 where the code is 1 and u = 2 where it is 0 (u < p, p in [0, 1]) -- every free
visible reads the uniform of the unconditioned chain."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_modes as TM   # noqa: E402
from oracle import det, generators as G   # noqa: E402

DEV = "cuda:0"
FREE = 255


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def clamp_u(u, codes):
    """The visible uniforms that make det.rbm_gibbs emit the clamped values."""
    return np.where(codes == 1, np.float32(-1.0), np.where(codes == 0, np.float32(2.0), u)).astype(np.float32)


def random_codes(R, shape, density):
    vals = (R.random(shape) < 0.3).astype(np.uint8)
    return np.where(R.random(shape) < density, vals, FREE).astype(np.uint8)


def clamped_gibbs(v0, W, bh, bv, k, u_h, u_v, codes):
    """The clamped k-step chain composed from the checker: (p_v, v)."""
    v = np.where(codes != FREE, codes, v0).astype(np.uint8)
    p = v.astype(np.float32)
    for it in range(k):
        p, v = det.rbm_gibbs(v, W, bh, bv, 1, u_h[it:it + 1], clamp_u(u_v[it:it + 1], codes))
    return p, v


# the shapes of test_gpu_kernels.py::test_rbm_gibbs_bit_exact that reach each form of the chain
FORMS = [(20, 88, 256, False),      # W resident in LDS
         (9, 30, 20, True),         # W resident in LDS, rows split over spare threads, broadcast bias rows
         (2101, 88, 256, False),    # matrix cores (training-sized batch)
         (33, 300, 100, False),     # matrix cores at small N (D > 256: the LDS form does not apply)
         (17, 440, 256, False),     # streaming (W does not fit LDS)
         (2050, 300, 280, False)]   # streaming


def rbm_problem(N, D, Hn, bcast, seed):
    R = np.random.default_rng(seed)
    W = (R.standard_normal((D, Hn)) * .3).astype(np.float32)
    bh = (R.standard_normal((1 if bcast else N, Hn)) * .3).astype(np.float32)
    bv = (R.standard_normal((1 if bcast else N, D)) * .3).astype(np.float32)
    v0 = (R.random((N, D)) < .1).astype(np.uint8)
    return R, W, bh, bv, v0


def run_gibbs(ops, v0, W, bh, bv, k, given=None, **kw):
    N, D = v0.shape
    p_v = torch.full((N, D), -1.0, device=DEV)
    v_out = torch.full((N, D), 7, device=DEV, dtype=torch.uint8)
    ops.rbm_gibbs(v0, W, bh, bv, k, p_v=p_v, v_out=v_out, given=given, **kw)
    return p_v, v_out


# ------------------------------------------------------------------------------------------------
# 1. kernels vs the checker
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
@pytest.mark.parametrize("k", [0, 1, 10])
@pytest.mark.parametrize("density", [0.3, 1.0])
def test_clamped_gibbs_bit_exact(ops, N, D, Hn, bcast, k, density):
    R, W, bh, bv, v0 = rbm_problem(N, D, Hn, bcast, D + 7 * k)
    codes = random_codes(R, (N, D), density)
    rows = np.arange(500, 500 + N)
    u_h, u_v = G.gibbs_uniforms(11, rows, k, Hn, D, sub0=3)
    p_ref, v_ref = clamped_gibbs(v0, W, bh, bv, k, u_h, u_v, codes)
    args = (dev(v0), dev(W), dev(bh), dev(bv), k)
    p_v, v_out = run_gibbs(ops, *args, given=dev(codes), seed=11, row0=500, sub0=3)
    assert np.array_equal(v_out.cpu().numpy(), v_ref), "clamped Gibbs samples must be bit-exact"
    assert np.array_equal(p_v.cpu().numpy(), p_ref)
    given = codes != FREE
    assert np.array_equal(v_out.cpu().numpy()[given], codes[given])
    if density == 1.0:
        assert np.array_equal(v_out.cpu().numpy(), codes)
    # a step slice of a [N, steps, D] block read in place (ld_given = 3 D), rows through row_ids
    block = np.full((N, 3, D), FREE, np.uint8)
    block[:, 1] = codes
    sl = dev(block)[:, 1]
    assert not sl.is_contiguous() and sl.stride(0) == 3 * D
    p2, v2 = run_gibbs(ops, *args, given=sl, seed=11, row0=0, row_ids=dev(rows.astype(np.int32)), sub0=3)
    assert torch.equal(v2, v_out) and torch.equal(p2, p_v)


# 2. every code free: the unconditioned chain, bit for bit
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
@pytest.mark.parametrize("k", [0, 3])
def test_all_free_codes_equal_unconditioned(ops, N, D, Hn, bcast, k):
    _, W, bh, bv, v0 = rbm_problem(N, D, Hn, bcast, 3 * D)
    args = (dev(v0), dev(W), dev(bh), dev(bv), k)
    p0, v0_ = run_gibbs(ops, *args, seed=5, row0=9, sub0=1)
    p1, v1 = run_gibbs(ops, *args, given=torch.full((N, D), FREE, device=DEV, dtype=torch.uint8), seed=5, row0=9, sub0=1)
    assert torch.equal(v1, v0_) and torch.equal(p1, p0)


# 3. the forms agree
@pytest.mark.parametrize("N,D,Hn,bcast", FORMS)
def test_clamped_gibbs_forms_agree(ops, monkeypatch, N, D, Hn, bcast):
    R, W, bh, bv, v0 = rbm_problem(N, D, Hn, bcast, 5 * D)
    codes = dev(random_codes(R, (N, D), 0.4))
    args = (dev(v0), dev(W), dev(bh), dev(bv), 4)
    res = []
    for env in ({}, {"MNN_RBM_STREAM_W": "1"}, {"MNN_RBM_NO_MFMA": "1"}, {"MNN_RBM_STREAM_W": "1", "MNN_RBM_NO_MFMA": "1"}):
        for key in ("MNN_RBM_STREAM_W", "MNN_RBM_NO_MFMA"):
            monkeypatch.delenv(key, raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        res.append(run_gibbs(ops, *args, given=codes, seed=21, row0=3, sub0=2))
    for key in ("MNN_RBM_STREAM_W", "MNN_RBM_NO_MFMA"):
        monkeypatch.delenv(key, raising=False)
    for p, v in res[1:]:
        assert torch.equal(v, res[0][1]) and torch.equal(p, res[0][0])


# 4. it samples the conditional
def test_clamped_chain_samples_the_conditional(ops):
    """A tiny RBM whose weights couple the visibles strongly: with visibles 0 and 2 clamped, the two free visibles at the end of a 50-step
    chain follow the exact conditional p(v1, v3 | v0 = 1, v2 = 0), computed by enumerating all 2^(4+3) states.  The bound was sized by the
    composed checker chain on the CPU (total variation 0.005 at these draws; the GPU's draws are the same bits); the free chain's marginal is
    0.58 away from the conditional."""
    D, Hn, N, k = 4, 3, 16384, 50
    R = np.random.default_rng(8)
    W = (R.standard_normal((D, Hn)) * 2.5).astype(np.float32)
    bh = (R.standard_normal((1, Hn)) * .5).astype(np.float32)
    bv = (R.standard_normal((1, D)) * .5).astype(np.float32)
    codes = np.tile(np.array([1, FREE, 0, FREE], np.uint8), (N, 1))
    v0 = (R.random((N, D)) < .5).astype(np.uint8)
    P = np.zeros((2,) * D)
    W64, bh64, bv64 = W.astype(np.float64), bh[0].astype(np.float64), bv[0].astype(np.float64)
    for vv in itertools.product((0, 1), repeat=D):
        for hh in itertools.product((0, 1), repeat=Hn):
            a, b = np.array(vv, np.float64), np.array(hh, np.float64)
            P[vv] += np.exp(a @ bv64 + b @ bh64 + a @ W64 @ b)
    P /= P.sum()
    cond = P[1, :, 0, :] / P[1, :, 0, :].sum()
    marg = P.sum((0, 2))

    def tv(v):
        emp = np.array([[np.mean((v[:, 1] == a) & (v[:, 3] == b)) for b in (0, 1)] for a in (0, 1)])
        return 0.5 * np.abs(emp - cond).sum()

    _, v = run_gibbs(ops, dev(v0), dev(W), dev(bh), dev(bv), k, given=dev(codes), seed=7, row0=0, sub0=0)
    v = v.cpu().numpy()
    assert (v[:, 0] == 1).all() and (v[:, 2] == 0).all()
    assert tv(v) < 0.015, tv(v)
    assert 0.5 * np.abs(cond - marg).sum() > 0.5
    _, vf = run_gibbs(ops, dev(v0), dev(W), dev(bh), dev(bv), k, seed=7, row0=0, sub0=0)
    assert tv(vf.cpu().numpy()) > 0.4                       # the unconditioned chain does not sample it


# ------------------------------------------------------------------------------------------------
# 5. RnnRBM.generate with given
def clamped_rnn_rbm_generate(intro, num_steps, p, k, seed, codes, row0=0, internal_bias=True):
    """det.rnn_rbm_generate with the clamped chain per generated step: codes u8 [B, num_steps, D]."""
    B, Ti, D = intro.shape
    Hn = p['W'].shape[1]
    state, h = None, None
    for t in range(Ti):
        h, state = det.lstm_step(intro[:, t], state, p['lstm'])
    bh0 = np.asarray(p['bh'], np.float32).reshape(-1) if internal_bias else None
    bv0 = np.asarray(p['bv'], np.float32).reshape(-1) if internal_bias else None
    rows = np.arange(row0, row0 + B, dtype=np.uint32)
    prev = np.ascontiguousarray(intro[:, -1], np.uint8)
    out = np.empty((B, num_steps, D), np.uint8)
    for s in range(num_steps):
        bh_t, bv_t = det.dense(h, p['Wuh'], bh0), det.dense(h, p['Wuv'], bv0)
        u_h, u_v = G.gibbs_uniforms(seed, rows, k, Hn, D, sub0=s * max(k, 1))
        _, v = clamped_gibbs(prev, p['W'], bh_t, bv_t, k, u_h, u_v, codes[:, s])
        out[:, s] = v
        h, state = det.lstm_step(v, state, p['lstm'])
        prev = v
    return out


@pytest.mark.parametrize("internal_bias", [True, False])
def test_rnn_rbm_generate_with_given(monkeypatch, internal_bias):
    from multinn_amd import RnnRBM
    B, Ti, D, Hn, units, k, steps = 10, 4, 24, 40, [64, 32], 4, 7
    R = np.random.default_rng(26 + internal_bias)
    intro = (R.random((B, Ti, D)) < .3).astype(np.uint8)
    p = G.init_rnn_rbm(27, D, D, Hn, units, np.float32)
    p['bh'] += np.float32(0.1); p['bv'] -= np.float32(0.3)
    gen = RnnRBM(D, Hn, units, k=k, precision="fp32", seed=41, internal_bias=internal_bias)
    gen._materialize(D)
    TM.load_rbm_params(gen, p)
    codes = random_codes(R, (B, steps, D), 0.4)
    ref = clamped_rnn_rbm_generate(intro, steps, p, k, 41, codes, internal_bias=internal_bias)
    out = gen.generate(dev(intro), steps, given=dev(codes))                    # captured scan
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(out.cpu().numpy()[codes != FREE], codes[codes != FREE])
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(dev(intro), steps, given=dev(codes)), out)    # eager
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    # a second given of the same shape replays the same graph, with its own answer
    n_graphs = len(gen._scan_graphs._cache)
    codes2 = random_codes(R, (B, steps, D), 0.7)
    out2 = gen.generate(dev(intro), steps, given=dev(codes2))
    assert len(gen._scan_graphs._cache) == n_graphs
    assert np.array_equal(out2.cpu().numpy(), clamped_rnn_rbm_generate(intro, steps, p, k, 41, codes2, internal_bias=internal_bias))
    # no given: the unconditioned scan
    assert np.array_equal(gen.generate(dev(intro), steps).cpu().numpy(), det.rnn_rbm_generate(intro, steps, p, k, 41, internal_bias=internal_bias))


# ------------------------------------------------------------------------------------------------
# 6. the mode classes
def rbm_mode(mode, P=8, M=3, B=4, Ti=3, Hn=16, seed=14):
    from multinn_amd import MultINN
    x = (np.random.default_rng(seed).random((B, Ti, P, M)) < 0.3).astype(np.uint8)
    m = MultINN(TM.config(P, TM.TRACKS5[:M]), TM.params(mode, gen="RBM", Hn=Hn, units=(32, 32)), mode=mode, precision="fp32")
    m.build(dev(x), lengths=None, is_train=False, mode="generate")
    return m, x


def masks(R, B, steps, P, M):
    return (torch.tensor([False, True, False]), torch.from_numpy(R.random((P, M)) < 0.5), torch.from_numpy(R.random((B, steps, P, M)) < 0.4))


@pytest.mark.parametrize("mode", ["jamming", "joint"])
def test_rbm_mode_conditional_generation(mode):
    m, x = rbm_mode(mode)
    steps = 5
    base = m.generate(steps)
    B, _, P, M = base.shape
    R = np.random.default_rng(7)
    given = dev((R.random((B, steps, P, M)) < 0.3).astype(np.uint8))
    for mask in masks(R, B, steps, P, M):
        out = m.generate(steps, given=given, given_mask=mask)
        full = mask.to(DEV).expand(B, steps, P, M)
        assert torch.equal(out[full], given[full]), mode
        assert not torch.equal(out, base)
    assert torch.equal(m.generate(steps), base)                          # no given: today's bits, before and after
    d = m._config["data"]
    n = d["beat_resolution"] * (d["pitch_range"]["highest"] - d["pitch_range"]["lowest"]) // m._num_dims
    g2 = dev((R.random((B, n, P, M)) < 0.3).astype(np.uint8))
    pm = torch.zeros(P, M, dtype=torch.bool)
    pm[:P // 2, 0] = True
    out = m.sampler(1, given=g2, given_mask=pm)
    assert torch.equal(out[:, :, :P // 2, 0], g2[:, :, :P // 2, 0])


def test_joint_rbm_conditional_bit_exact():
    """Joint mode's one RBM over the stacked tracks (codes in p M + m order) against the clamped restatement."""
    from multinn_amd.common import given_codes
    m, x = rbm_mode("joint", P=6, M=3, B=5, Ti=3, Hn=20)
    g = m.generators[0]
    B, Ti, P, M = x.shape
    p = G.init_rnn_rbm(33, P * M, P * M, 20, [32, 32], np.float32)
    p['bv'] -= np.float32(0.5)
    TM.load_rbm_params(g, p)
    steps = 6
    R = np.random.default_rng(2)
    given = dev((R.random((B, steps, P, M)) < 0.3).astype(np.uint8))
    mask = torch.from_numpy(R.random((P, M)) < 0.5)
    out = m.generate(steps, given=given, given_mask=mask).cpu().numpy()
    codes = given_codes(given, mask).reshape(B, steps, P * M).cpu().numpy()
    intro = np.concatenate([np.zeros((B, 1, P * M), np.uint8), x.reshape(B, Ti, P * M)], 1)
    ref = clamped_rnn_rbm_generate(intro, steps, p, g.k, g.seed, codes, row0=g.row0, internal_bias=g.internal_bias)
    assert np.array_equal(out, ref.reshape(B, steps, P, M))


def test_feedback_rbm_partial_mask_still_refused():
    from multinn_amd import MultINN
    m = MultINN(TM.config(8, TM.TRACKS5[:3]), TM.params("feedback", gen="RBM", Hn=16, units=(32, 32), feedback=[32]), mode="feedback",
                precision="fp32")
    pm = torch.zeros(8, 3, dtype=torch.bool)
    pm[:4, 0] = True
    with pytest.raises(NotImplementedError):
        m.generate(4, given=torch.zeros(2, 4, 8, 3, dtype=torch.uint8, device=DEV), given_mask=pm)
