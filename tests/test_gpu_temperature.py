"""Sampling temperature on the device, scalar or per track, from the kernels to the mode classes.

The checker (oracle/det_ref.c) has a scalar NADE temperature and nothing else.  Everything it lacks -- a temperature per visible index, the
tempered RBM chain, a temperature per track -- is checked against it through one fact: dividing by a power of two is exact in float32, so a
run at T = 2^k must equal, bit for bit, the checker at T = 1 on parameters multiplied by 2^-k (RBM: W, bh, bv -- for a generator also Wuh, Wuv
and the internal biases; NADE: the b_dec columns of the Dense kernel and bias and the w_dec rows of the affected visibles).  Temperatures that
are no power of two are checked against the checker's own scalar temperature (NADE) and a float64 restatement (RBM)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_modes as TM   # noqa: E402
import test_gpu_conditional as TN   # noqa: E402
import test_gpu_conditional_rbm as TC   # noqa: E402
from oracle import det, philox, generators as G   # noqa: E402

DEV = "cuda:0"
FREE = 255
F = np.float32


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def inv(t):
    """1 / t as float32, for a power of two: the factor that multiplies the checker's parameters."""
    s = F(1.0) / F(t)
    assert float(s) * float(t) == 1.0 and np.frexp(float(t))[0] == 0.5, "power-of-two temperatures only"
    return s


SAMPLE_FORMS = ({}, {"MNN_SAMPLE_G8": "1"}, {"MNN_SAMPLE_NO_CHUNK": "1"})      # sixteen visibles per pass, eight, one


def in_every_sample_form(monkeypatch, run):
    """run() under each form of the NADE sampling scan; the results must be the same tensors."""
    res = []
    for env in SAMPLE_FORMS:
        for k in ("MNN_SAMPLE_NO_CHUNK", "MNN_SAMPLE_G8"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res.append(run())
    for k in ("MNN_SAMPLE_NO_CHUNK", "MNN_SAMPLE_G8"):
        monkeypatch.delenv(k, raising=False)
    for r in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, res[0])), "the forms of the sampling scan must agree"
    return res[0]


# ------------------------------------------------------------------------------------------------
# 3. NADE, one temperature per track
@pytest.mark.parametrize("Hn", [256, 48])                      # FULL and not
@pytest.mark.parametrize("with_given", [False, True])
def test_nade_sample_per_track(ops, monkeypatch, Hn, with_given):
    tracks, N, D, temps = 3, 37, 20, (0.5, 1.0, 1.7)           # D = 20: one chunk of sixteen and a tail of four; 37 rows: no multiple of anything
    R = np.random.default_rng(Hn + with_given)
    bias = (R.standard_normal((N, tracks * (Hn + D))) * .5).astype(F)
    we = (R.standard_normal((tracks, D, Hn)) * .3).astype(F)
    wd = (R.standard_normal((tracks, D, Hn)) * .3).astype(F)
    codes = TN.random_codes(R, (N, tracks, D), 0.3) if with_given else np.full((N, tracks, D), FREE, np.uint8)

    def run():
        out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
        nll = torch.zeros((tracks, N), device=DEV)
        ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, temps, seed=77, row0=1000, sub=5, samples=out, nll=nll,
                        given=dev(codes.reshape(N, tracks * D)) if with_given else None)
        return out, nll

    out, nll = in_every_sample_form(monkeypatch, run)
    got = out.cpu().numpy().reshape(N, tracks, D)
    u = philox.uniform_block(77, philox.STREAM_NADE, np.arange(1000, 1000 + N), 5, tracks * D)
    for m in range(tracks):
        s_ref, p_ref = det.nade_sample(bias, we[m], wd[m], tracks, m, D, Hn, temps[m], TN.clamp_u(u[:, m * D:(m + 1) * D], codes[:, m]))
        assert np.array_equal(got[:, m], s_ref), f"track {m}: draws at temperature {temps[m]} must be the checker's"
        # the nll stays the model's own: the T = 1 scoring of the emitted vector (the checker's p is the untempered conditional)
        q = np.where(s_ref > 0, p_ref, F(1.0) - p_ref).astype(np.float64)
        assert TN.rel(nll[m].cpu().numpy(), -np.log(1e-6 + q).sum(1)) < 1e-5
    # the tempered tracks differ from a T = 1 run, the track at 1.0 does not
    base = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, 1.0, seed=77, row0=1000, sub=5, samples=base,
                    given=dev(codes.reshape(N, tracks * D)) if with_given else None)
    base = base.cpu().numpy().reshape(N, tracks, D)
    assert np.array_equal(base[:, 1], got[:, 1]) and not np.array_equal(base[:, 0], got[:, 0]) and not np.array_equal(base[:, 2], got[:, 2])
    # a sequence of equal values is the scalar
    one = torch.zeros_like(out)
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, 1.7, seed=77, row0=1000, sub=5, samples=one)
    seq = torch.zeros_like(out)
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, (1.7, 1.7, 1.7), seed=77, row0=1000, sub=5, samples=seq)
    assert torch.equal(one, seq)


# 4. NADE, the temperature a function of the visible index
@pytest.mark.parametrize("Hn", [256, 48])
@pytest.mark.parametrize("with_given", [False, True])
def test_nade_sample_by_visible(ops, monkeypatch, Hn, with_given):
    N, P, M, temps = 37, 7, 3, (0.5, 2.0, 4.0)
    D = P * M                                                   # 21: a chunk of sixteen and a tail of five; 16 % 3 != 0: the running index wraps
    R = np.random.default_rng(3 * Hn + with_given)
    bias = (R.standard_normal((N, Hn + D)) * .5).astype(F)
    we = (R.standard_normal((1, D, Hn)) * .3).astype(F)
    wd = (R.standard_normal((1, D, Hn)) * .3).astype(F)
    codes = TN.random_codes(R, (N, D), 0.3) if with_given else np.full((N, D), FREE, np.uint8)

    def run():
        out = torch.zeros((N, D), device=DEV, dtype=torch.uint8)
        nll = torch.zeros((1, N), device=DEV)
        ops.nade_sample(dev(bias), dev(we), dev(wd), 1, D, Hn, temps, seed=5, row0=40, sub=2, samples=out, nll=nll, by_visible=True,
                        given=dev(codes) if with_given else None)
        return out, nll

    out, nll = in_every_sample_form(monkeypatch, run)
    s = np.array([inv(temps[i % M]) for i in range(D)], F)
    bias_s, wd_s = bias.copy(), wd.copy()
    bias_s[:, Hn:] *= s[None, :]
    wd_s[0] *= s[:, None]
    u = TN.clamp_u(philox.uniform_block(5, philox.STREAM_NADE, np.arange(40, 40 + N), 2, D), codes)
    s_ref, _ = det.nade_sample(bias_s, we[0], wd_s[0], 1, 0, D, Hn, 1.0, u)
    assert np.array_equal(out.cpu().numpy(), s_ref)
    _, p_ref = det.nade_sample(bias, we[0], wd[0], 1, 0, D, Hn, 1.0, TN.clamp_u(u, s_ref))      # the model's own conditionals of the emitted vector
    q = np.where(s_ref > 0, p_ref, F(1.0) - p_ref).astype(np.float64)
    assert TN.rel(nll[0].cpu().numpy(), -np.log(1e-6 + q).sum(1)) < 1e-5


# ------------------------------------------------------------------------------------------------
# 5. the RBM chain in its three forms
RBM_FORMS = [("lds", 5, {}), ("stream", 13, {"MNN_RBM_STREAM_W": "1", "MNN_RBM_NO_MFMA": "1"}), ("mfma", 2048, {})]


def rbm_problem(N, D, Hn, seed, rows_of_bias=None):
    R = np.random.default_rng(seed)
    W = (R.standard_normal((D, Hn)) * .6).astype(F)
    bh = (R.standard_normal((rows_of_bias or N, Hn)) * .5).astype(F)
    bv = (R.standard_normal((rows_of_bias or N, D)) * .5).astype(F)
    v0 = (R.random((N, D)) < .2).astype(np.uint8)
    return R, W, bh, bv, v0


def set_form(monkeypatch, env):
    for k in ("MNN_RBM_STREAM_W", "MNN_RBM_NO_MFMA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("form,N,env", RBM_FORMS)
@pytest.mark.parametrize("T", [0.5, 2.0])
@pytest.mark.parametrize("with_given", [False, True])
def test_rbm_chain_tempered(ops, monkeypatch, form, N, env, T, with_given):
    D, Hn, k = 20, 24, 3
    R, W, bh, bv, v0 = rbm_problem(N, D, Hn, N + int(4 * T))
    codes = TC.random_codes(R, (N, D), 0.3) if with_given else np.full((N, D), FREE, np.uint8)
    rows = np.arange(500, 500 + N)
    u_h, u_v = G.gibbs_uniforms(11, rows, k, Hn, D, sub0=3)
    s = inv(T)
    p_ref, v_ref = TC.clamped_gibbs(v0, W * s, bh * s, bv * s, k, u_h, u_v, codes)
    set_form(monkeypatch, env)
    args = (dev(v0), dev(W), dev(bh), dev(bv), k)
    p_v, v_out = TC.run_gibbs(ops, *args, given=dev(codes) if with_given else None, seed=11, row0=500, sub0=3, temperature=T)
    p1, v1 = TC.run_gibbs(ops, *args, given=dev(codes) if with_given else None, seed=11, row0=500, sub0=3)
    set_form(monkeypatch, {})
    assert np.array_equal(v_out.cpu().numpy(), v_ref), f"{form}: the tempered chain's samples"
    assert np.array_equal(p_v.cpu().numpy(), p_ref), f"{form}: p_v is the tempered probability the chain drew from"
    assert np.array_equal(v_out.cpu().numpy()[codes != FREE], codes[codes != FREE])
    assert not torch.equal(p1, p_v)                             # (and it is not the chain at temperature 1)
    p_u, v_u = TC.clamped_gibbs(v0, W, bh, bv, k, u_h, u_v, codes)
    assert np.array_equal(v1.cpu().numpy(), v_u) and np.array_equal(p1.cpu().numpy(), p_u)


@pytest.mark.parametrize("form,N,env", RBM_FORMS)
@pytest.mark.parametrize("with_given", [False, True])
def test_rbm_grouped_chain_one_temperature_per_job(ops, monkeypatch, form, N, env, with_given):
    """Three jobs at (0.5, 1, 2) in the strided composer layout: each equals its single launch at its temperature, bit for bit -- and, all
    three being powers of two, the checker on its scaled parameters."""
    D, Hn, k, M, temps, seed = 20, 24, 3, 3, (0.5, 1.0, 2.0), 31
    R = np.random.default_rng(N)
    W = (R.standard_normal((M, D, Hn)) * .6).astype(F)
    ld = -(-(M * (Hn + D)) // 64) * 64
    blk = (R.standard_normal((N, ld)) * .5).astype(F)
    x = (R.random((N, D * M)) < .2).astype(np.uint8)
    codes = TC.random_codes(R, (N, D * M), 0.3) if with_given else None
    W_d, blk_d, x_d = dev(W), dev(blk), dev(x)
    g_d = None if codes is None else dev(codes)
    bh = [blk_d[:, m * Hn:(m + 1) * Hn] for m in range(M)]
    bv = [blk_d[:, M * Hn + m * D:M * Hn + (m + 1) * D] for m in range(M)]
    set_form(monkeypatch, env)
    p_v = torch.full((N, D * M), -1.0, device=DEV)
    v_out = torch.full((N, D * M), 7, device=DEV, dtype=torch.uint8)
    jobs = [dict(v0=x_d[:, m::M], W=W_d[m], bh=bh[m], bv=bv[m], seed=seed + m, p_v=p_v[:, m::M], v_out=v_out[:, m::M],
                 given=None if g_d is None else g_d[:, m::M]) for m in range(M)]
    ops.rbm_gibbs_multi(jobs, k, row0=300, sub0=2, temperature=temps)
    singles = []
    for m in range(M):
        singles.append(TC.run_gibbs(ops, x_d[:, m::M].contiguous(), W_d[m], bh[m].contiguous(), bv[m].contiguous(), k,
                                    given=None if g_d is None else g_d[:, m::M].contiguous(), seed=seed + m, row0=300, sub0=2, temperature=temps[m]))
    set_form(monkeypatch, {})
    rows = np.arange(300, 300 + N)
    for m in range(M):
        assert torch.equal(v_out[:, m::M], singles[m][1]) and torch.equal(p_v[:, m::M], singles[m][0]), (form, m)
        u_h, u_v = G.gibbs_uniforms(seed + m, rows, k, Hn, D, sub0=2)
        s = inv(temps[m])
        c = np.full((N, D), FREE, np.uint8) if codes is None else codes[:, m::M]
        p_ref, v_ref = TC.clamped_gibbs(x[:, m::M], W[m] * s, blk[:, m * Hn:(m + 1) * Hn] * s, blk[:, M * Hn + m * D:M * Hn + (m + 1) * D] * s,
                                        k, u_h, u_v, c)
        assert np.array_equal(v_out[:, m::M].cpu().numpy(), v_ref) and np.array_equal(p_v[:, m::M].cpu().numpy(), p_ref), (form, m)


# 6. temperatures that are no power of two, against a float64 restatement
NP2_SEED = 2           # chosen on the CPU: the float64 restatement alone excludes no row at either temperature (seed 1: one row at T = 1.5)


def f64_tempered_chain(T, seed=NP2_SEED, N=64, D=20, Hn=24):
    """One Gibbs iteration of exp(-E / T) in float64 with the device's uniforms -> (problem, p_v, v, rows with a draw within 1e-4 of a tie)."""
    _, W, bh, bv, v0 = rbm_problem(N, D, Hn, 64)
    u_h, u_v = G.gibbs_uniforms(seed, np.arange(N), 1, Hn, D, sub0=0)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    p_h = sig((v0.astype(np.float64) @ W.astype(np.float64) + bh) / T)
    h = (u_h[0] < p_h).astype(np.float64)
    p_v = sig((h @ W.astype(np.float64).T + bv) / T)
    v = (u_v[0] < p_v).astype(np.uint8)
    near = (np.abs(u_h[0] - p_h) < 1e-4).any(1) | (np.abs(u_v[0] - p_v) < 1e-4).any(1)
    return (W, bh, bv, v0), p_v, v, near


@pytest.mark.parametrize("T", [0.75, 1.5])
def test_rbm_chain_tempered_not_a_power_of_two(ops, T):
    N = 64
    (W, bh, bv, v0), p_ref, v_ref, near = f64_tempered_chain(T)
    p_v, v_out = TC.run_gibbs(ops, dev(v0), dev(W), dev(bh), dev(bv), 1, seed=NP2_SEED, row0=0, sub0=0, temperature=T)
    keep = ~near
    print(f"T = {T}: {int(near.sum())} of {N} rows excluded; max |p_v - p| on the others {np.abs(p_v.cpu().numpy()[keep] - p_ref[keep]).max():.2e}")
    assert near.sum() <= 0.1 * N
    assert np.array_equal(v_out.cpu().numpy()[keep], v_ref[keep])
    assert np.abs(p_v.cpu().numpy()[keep] - p_ref[keep]).max() <= 1e-4


# ------------------------------------------------------------------------------------------------
# generators.  B = 3, a 4-step intro, 6 generated steps
B, TI, STEPS = 3, 4, 6


def nade_generator(tracks, seed=31, E=8, Hn=32, units=(32, 32)):
    from multinn_amd import RnnNade, RnnMultiNADE
    Din = E * tracks if tracks > 1 else E
    p = G.init_rnn_nade(9 + tracks, Din, E, Hn, list(units), F, tracks=tracks)
    p['fc_b'][tracks * Hn:] = F(-0.5)
    gen = RnnNade(E, Hn, list(units), precision="fp32", seed=seed) if tracks == 1 else \
        RnnMultiNADE(E, Hn, list(units), tracks=list("abc")[:tracks], precision="fp32", seed=seed)
    gen._materialize(Din)
    TN.load_nade_params(gen, p)
    intro = (np.random.default_rng(60 + tracks).random((B, TI, Din)) < .3).astype(np.uint8)
    return gen, p, intro


def scale_nade_visibles(p, Hn_total, scale_of_visible, tracks=1):
    """A copy of the parameters with visible i of track m multiplied by scale_of_visible(m, i) in its b_dec column (Dense kernel and bias)
    and its w_dec row."""
    q = copy.deepcopy(p)
    D = p['w_dec'][0].shape[0]
    for m in range(tracks):
        s = np.array([scale_of_visible(m, i) for i in range(D)], F)
        c0 = Hn_total + m * D
        q['fc_k'][:, c0:c0 + D] *= s[None, :]
        q['fc_b'][c0:c0 + D] *= s
        q['w_dec'][m] = q['w_dec'][m] * s[:, None]
    return q


# 7. a scalar through the one-call scan, the captured scan and the eager loop
def test_rnn_nade_generate_scalar(monkeypatch):
    gen, p, intro = nade_generator(1, E=24)
    ref = det.rnn_nade_generate(intro, STEPS, p, 31, temperature=0.8)
    assert np.array_equal(gen._scan_in_one_call(dev(intro), STEPS, None, 0.8).cpu().numpy(), ref)
    out = gen.generate(dev(intro), STEPS, temperature=0.8)                       # captured
    assert np.array_equal(out.cpu().numpy(), ref)
    assert torch.equal(gen.generate(dev(intro), STEPS, temperature=0.8), out)    # replayed
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(dev(intro), STEPS, temperature=0.8), out)    # the eager loop
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    assert torch.equal(gen.generate(dev(intro).float(), STEPS, temperature=0.8), out)      # step by step through sample_single
    assert not np.array_equal(ref, det.rnn_nade_generate(intro, STEPS, p, 31))
    # None: the reference's threshold decoding
    assert np.array_equal(gen.generate(dev(intro), STEPS, temperature=None).cpu().numpy(), det.rnn_nade_generate(intro, STEPS, p, 31, temperature=None))
    # sample_single has the argument, and its nll is the model's own
    state = gen.steps(dev(intro))
    s1, n1 = gen.sample_single(None, state, temperature=0.8)
    assert np.array_equal(s1.cpu().numpy(), ref[:, 0])


# 8. one temperature per track: the MultiNADE, and the joint NADE's visibles p M + m
def test_rnn_multinade_generate_per_track(monkeypatch):
    temps, Hn = (0.5, 1.0, 2.0), 32
    gen, p, intro = nade_generator(3)
    ref = det.rnn_nade_generate(intro, STEPS, scale_nade_visibles(p, 3 * Hn, lambda m, i: inv(temps[m]), tracks=3), 31, tracks=3)
    out = gen.generate(dev(intro), STEPS, temperature=temps)
    assert np.array_equal(out.cpu().numpy(), ref)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(dev(intro), STEPS, temperature=list(temps)), out)
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    assert torch.equal(gen.generate(dev(intro).float(), STEPS, temperature=temps), out)
    plain = det.rnn_nade_generate(intro, STEPS, p, 31, tracks=3)
    assert not np.array_equal(ref, plain)
    assert np.array_equal(gen.generate(dev(intro), STEPS, temperature=(0.8, 0.8, 0.8)).cpu().numpy(),
                          det.rnn_nade_generate(intro, STEPS, p, 31, tracks=3, temperature=0.8))


def test_joint_nade_generate_per_track(monkeypatch):
    temps, Hn, M = (0.5, 2.0, 4.0), 32, 3
    gen, p, intro = nade_generator(1, E=24)                                      # 24 visibles = 8 pitches x 3 tracks, ordered p M + m
    ref = det.rnn_nade_generate(intro, STEPS, scale_nade_visibles(p, Hn, lambda m, i: inv(temps[i % M])), 31)
    out = gen.generate(dev(intro), STEPS, temperature=temps)
    assert np.array_equal(out.cpu().numpy(), ref)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(dev(intro), STEPS, temperature=temps), out)
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    assert torch.equal(gen.generate(dev(intro).float(), STEPS, temperature=temps), out)
    assert not np.array_equal(ref, det.rnn_nade_generate(intro, STEPS, p, 31))


# 9. RBM generators
def test_rnn_rbm_generate_tempered(monkeypatch):
    from multinn_amd import RnnRBM
    D, Hn, units, k = 24, 40, [32, 32], 3
    intro = (np.random.default_rng(26).random((B, TI, D)) < .3).astype(np.uint8)
    p = G.init_rnn_rbm(27, D, D, Hn, units, F)
    p['bh'] += F(0.1); p['bv'] -= F(0.3)
    gen = RnnRBM(D, Hn, units, k=k, precision="fp32", seed=41)
    gen._materialize(D)
    TM.load_rbm_params(gen, p)
    q = dict(p)
    for name in ("W", "bh", "bv", "Wuh", "Wuv"):
        q[name] = p[name] * inv(2.0)
    ref = det.rnn_rbm_generate(intro, STEPS, q, k, 41)
    out = gen.generate(dev(intro), STEPS, temperature=2)
    assert np.array_equal(out.cpu().numpy(), ref)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(dev(intro), STEPS, temperature=2.0), out)
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    assert not np.array_equal(ref, det.rnn_rbm_generate(intro, STEPS, p, k, 41))
    assert np.array_equal(gen.generate(dev(intro), STEPS).cpu().numpy(), det.rnn_rbm_generate(intro, STEPS, p, k, 41))


def test_rnn_multirbm_generate_per_track(monkeypatch):
    import test_gpu_multirbm as TR
    from multinn_amd import RnnMultiRBM
    D, Hn, units, M, k, temps = 8, 12, [32, 32], 3, 3, (0.5, 1.0, 2.0)
    p = TR.init_params(61, D, Hn, units, M, rho=0.2)
    p = dict(lstm=[(det.f32(W), det.f32(b)) for W, b in p['lstm']], W=[det.f32(w) * F(2) for w in p['W']], bh=[det.f32(b) for b in p['bh']],
             bv=[det.f32(b) for b in p['bv']], Wuh=det.f32(p['Wuh']), Wuv=det.f32(p['Wuv']))
    gen = RnnMultiRBM(D, Hn, units, tracks=list("abc"), k=k, precision="fp32", seed=23)
    gen._materialize(D * M)
    TR.load_params(gen, p)
    q = copy.deepcopy(p)
    for m in range(M):
        s = inv(temps[m])
        q['W'][m] *= s; q['bh'][m] *= s; q['bv'][m] *= s
        q['Wuh'][:, m * Hn:(m + 1) * Hn] *= s
        q['Wuv'][:, m * D:(m + 1) * D] *= s
    intro = (np.random.default_rng(7).random((B, TI, D * M)) < 0.2).astype(np.uint8)
    ref = TR.checker_generate(intro, STEPS, q, k, 23)
    out = gen.generate(dev(intro), STEPS, temperature=temps)
    assert np.array_equal(out.cpu().numpy(), ref)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(dev(intro), STEPS, temperature=temps), out)
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    plain = TR.checker_generate(intro, STEPS, p, k, 23)
    assert not np.array_equal(ref, plain)
    assert np.array_equal(gen.generate(dev(intro), STEPS, temperature=(1, 1, 1)).cpu().numpy(), plain)
    # with codes: a clamped cell stays as given at any temperature, the free ones are the checker's clamped tempered chain
    codes = TC.random_codes(np.random.default_rng(3), (B, STEPS, D * M), 0.3)
    got = gen.generate(dev(intro), STEPS, given=dev(codes), temperature=temps).cpu().numpy()
    assert np.array_equal(got, TR.checker_generate(intro, STEPS, q, k, 23, codes=codes))
    assert np.array_equal(got[codes != FREE], codes[codes != FREE])


# 10. the feedback scan: generator m at its own temperature inside the grouped launch
def test_feedback_scan_per_generator(monkeypatch):
    from multinn_amd import RnnNade
    from multinn_amd.feedback import FeedbackRnn, FeedbackRnnSampler
    P, M, Hn, Fb, temps = 8, 3, 16, 32, (0.5, 1.0, 2.0)
    x = (np.random.default_rng(14).random((B, TI, P, M)) < .3).astype(np.uint8)
    fb = FeedbackRnn(P * M, [64, Fb], precision="fp32", seed=40)

    class LaneNade(RnnNade):                                   # not an RnnNade by name: the scan takes its per-lane path (sample_single per generator)
        pass

    gens, lane_gens, gparams, scaled, seeds = [], [], [], [], []
    for i in range(M):
        p = G.init_rnn_nade(60 + i, P + Fb, P, Hn, [32, 32], F)
        p['fc_b'][Hn:] = F(-0.5)
        for cls, lst in ((RnnNade, gens), (LaneNade, lane_gens)):
            g = cls(P, Hn, [32, 32], precision="fp32", seed=50 + i)
            g._materialize(P + Fb)
            TN.load_nade_params(g, p)
            lst.append(g)
        gparams.append(p); seeds.append(50 + i)
        scaled.append(scale_nade_visibles(p, Hn, lambda m, j, i=i: inv(temps[i])))
    fb_layers = [(fb.store[f"feedback/rnn/cell_{l}/kernel"].cpu().numpy(), fb.store[f"feedback/rnn/cell_{l}/bias"].cpu().numpy()) for l in range(2)]
    sampler = FeedbackRnnSampler(gens, fb)
    ref = det.feedback_rnn_generate(x, STEPS, scaled, fb_layers, seeds)
    out = sampler.generate(dev(x), STEPS, temperature=temps)
    assert np.array_equal(out.cpu().numpy(), ref)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(sampler.generate(dev(x), STEPS, temperature=temps), out)
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    assert torch.equal(FeedbackRnnSampler(lane_gens, fb).generate(dev(x), STEPS, temperature=temps), out)      # the per-lane path, captured
    plain = det.feedback_rnn_generate(x, STEPS, gparams, fb_layers, seeds)
    assert not np.array_equal(ref, plain)
    assert np.array_equal(sampler.generate(dev(x), STEPS).cpu().numpy(), plain)


# ------------------------------------------------------------------------------------------------
# 11. every mode
def graphs_of(m):
    """Every captured scan a mode holds: its generators' caches and the feedback sampler's."""
    owners = list(m.generators) + ([m._sampler] if getattr(m, "_sampler", None) is not None else [])
    return sum(len(o._scan_graphs._cache) for o in owners if getattr(o, "_scan_graphs", None) is not None)


MODES = [("joint", "NADE"), ("composer", "NADE"), ("jamming", "NADE"), ("feedback", "NADE"), ("feedback-rnn", "NADE"),
         ("joint", "RBM"), ("jamming", "RBM"), ("composer", "MultiRBM")]


def make_mode(mode, gen):
    if gen == "NADE":
        return TN.make_mode(mode)[0]
    if gen == "RBM":
        return TC.rbm_mode(mode)[0]
    from multinn_amd import MultINN
    x = (np.random.default_rng(14).random((4, 3, 8, 3)) < 0.3).astype(np.uint8)
    m = MultINN(TM.config(8, TM.TRACKS5[:3]), TM.params(mode, gen=gen, Hn=16, units=(32, 32)), mode=mode, precision="fp32")
    m.build(dev(x), lengths=None, is_train=False, mode="generate")
    return m


@pytest.mark.parametrize("mode,gen", MODES)
def test_modes(mode, gen):
    m = make_mode(mode, gen)
    steps, M = 5, 3
    base = m.generate(steps)
    n_graphs = graphs_of(m)
    assert n_graphs >= 1
    per_track = not (mode == "joint" and gen == "RBM")
    # 1.0 and all ones: the bits of the call without the argument, replayed from the scan captured without it
    assert torch.equal(m.generate(steps, temperature=1.0), base)
    assert torch.equal(m.generate(steps, temperature=1), base)
    if per_track:
        assert torch.equal(m.generate(steps, temperature=[1.0] * M), base)
        assert torch.equal(m.generate(steps, temperature=(1, 1, 1)), base)
    assert graphs_of(m) == n_graphs
    # a scalar is the sequence of its copies
    hot = m.generate(steps, temperature=2.0)
    assert not torch.equal(hot, base)
    if per_track:
        assert torch.equal(m.generate(steps, temperature=[2.0] * M), hot)
        mixed = m.generate(steps, temperature=(0.5, 1.0, 2.0))
        assert not torch.equal(mixed, hot) and not torch.equal(mixed, base)
        if mode in ("jamming", "composer"):                    # the tracks of a step are independent given the history (jamming: for good)
            assert torch.equal(mixed[:, 0, :, 1], base[:, 0, :, 1]) and torch.equal(mixed[:, 0, :, 2], hot[:, 0, :, 2])
        if mode == "jamming":
            assert torch.equal(mixed[..., 1], base[..., 1]) and torch.equal(mixed[..., 2], hot[..., 2])
    else:
        with pytest.raises(ValueError):
            m.generate(steps, temperature=(0.5, 1.0, 2.0))
    if gen == "NADE":
        assert m.generate(steps, temperature=None).shape == base.shape
    else:
        with pytest.raises(ValueError):
            m.generate(steps, temperature=None)
    # with conditioning: a clamped cell stays as given at any temperature
    Bm, _, P, _ = base.shape
    R = np.random.default_rng(7)
    given = dev((R.random((Bm, steps, P, M)) < 0.3).astype(np.uint8))
    for mask in (torch.tensor([False, True, False]), torch.from_numpy(R.random((Bm, steps, P, M)) < 0.4)):
        out = m.generate(steps, given=given, given_mask=mask, temperature=2)
        full = mask.to(DEV).expand(Bm, steps, P, M)
        assert torch.equal(out[full], given[full]), mode
        assert torch.equal(m.generate(steps, given=given, given_mask=mask, temperature=1.0), m.generate(steps, given=given, given_mask=mask))
    # the sampler passes it on
    assert torch.equal(m.sampler(1, temperature=2.0), m.generate(m.sampler(1).shape[1], temperature=2.0))
    assert torch.equal(m.generate(steps), base)


# ------------------------------------------------------------------------------------------------
# 12. the direction of the effect: with every p < 0.5 a hotter chain plays more notes
def density(gen, intro, T):
    return float(gen.generate(dev(intro), 8, temperature=T).float().mean())


def test_note_density_grows_with_temperature():
    from multinn_amd import RnnNade, RnnRBM
    Bn, D, Hn, units = 16, 24, 32, [32, 32]
    intro = (np.random.default_rng(1).random((Bn, TI, D)) < .1).astype(np.uint8)
    p = G.init_rnn_nade(4, D, D, Hn, units, F)
    p['fc_b'][Hn:] = F(-2.0)                                   # strongly negative decoder biases, small decoder weights: every p < 0.5
    p['w_dec'] = [w * F(0.1) for w in p['w_dec']]
    p['fc_k'][:, Hn:] *= F(0.1)
    nade = RnnNade(D, Hn, units, precision="fp32", seed=3)
    nade._materialize(D)
    TN.load_nade_params(nade, p)
    q = G.init_rnn_rbm(5, D, D, Hn, units, F)
    q['bv'] -= F(2.0)
    q['W'] *= F(0.1); q['Wuv'] *= F(0.1)
    rbm = RnnRBM(D, Hn, units, k=3, precision="fp32", seed=6)
    rbm._materialize(D)
    TM.load_rbm_params(rbm, q)
    for gen in (nade, rbm):
        cold, mid, hot = density(gen, intro, 0.5), density(gen, intro, 1.0), density(gen, intro, 2.0)
        print(type(gen).__name__, "note density at T = 0.5 / 1 / 2:", cold, mid, hot)
        assert cold < mid < hot, (type(gen).__name__, cold, mid, hot)
        assert hot < 0.5
