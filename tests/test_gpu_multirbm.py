"""The composer-mode LSTM-RBM (generators.RnnMultiRBM) and the grouped RBM launches it runs on.

Kernels: every job of ops.rbm_gibbs_multi equals its single launch (ops.rbm_gibbs on contiguous copies) bit for bit -- in every kernel form,
for both addressings (element stride 1: de-interleaved planes; element stride M: composer layout in place), with codes, row ids and the
device-side step -- and the deterministic checker; ops.rbm_free_energy_multi equals ops.rbm_free_energy per job and float64.
Model: forward / backward against a float64 restatement (shared LSTM, one Dense whose gradient sums over the tracks' blocks), the captured
step, generation and conditional generation bit-exact against a step-by-step checker, the AIS likelihood against enumeration, and the
composer mode end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_modes as TM   # noqa: E402
import test_gpu_conditional_rbm as TC   # noqa: E402
from oracle import det, generators as G, lstm as OL, rbm as ORBM   # noqa: E402

DEV = "cuda:0"
FREE = 255


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ================================================================================================
# kernels
def multi_problem(N, D, Hn, M, bcast, seed):
    """M RBMs of one shape behind one Dense-output block [N, ld] = [bh_0 .. bh_{M-1} | bv_0 .. bv_{M-1} | padding] (bcast: one row), chains
    starting from a composer-layout batch [N, D * M] (feature d * M + m)."""
    R = np.random.default_rng(seed)
    W = (R.standard_normal((M, D, Hn)) * .3).astype(np.float32)
    ld = -(-(M * (Hn + D)) // 64) * 64
    out = (R.standard_normal((1 if bcast else N, ld)) * .3).astype(np.float32)
    x = (R.random((N, D * M)) < .1).astype(np.uint8)
    return R, W, out, x


def bias_views(out_d, M, D, Hn):
    return [out_d[:, m * Hn:(m + 1) * Hn] for m in range(M)], [out_d[:, M * Hn + m * D:M * Hn + (m + 1) * D] for m in range(M)]


def single_launches(ops, x_d, W_d, bh, bv, k, seed, given=None, **kw):
    """The reference of the invariant: one ops.rbm_gibbs per job on contiguous copies, seeds seed + m -> (p_v [M,N,D], v [M,N,D])."""
    M = W_d.shape[0]
    N, D = x_d.shape[0], x_d.shape[1] // M
    ps, vs = [], []
    for m in range(M):
        p_v = torch.full((N, D), -1.0, device=DEV)
        v_out = torch.full((N, D), 7, device=DEV, dtype=torch.uint8)
        g = None if given is None else given[:, m::M].contiguous()
        ops.rbm_gibbs(x_d[:, m::M].contiguous(), W_d[m], bh[m].contiguous(), bv[m].contiguous(), k, seed + m, p_v=p_v, v_out=v_out, given=g, **kw)
        ps.append(p_v); vs.append(v_out)
    return torch.stack(ps), torch.stack(vs)


def grouped_launch(ops, x_d, W_d, bh, bv, k, seed, es, given=None, **kw):
    """ONE grouped launch -> (p_v [M,N,D], v [M,N,D]).  es = M: the composer-layout batch is read, and composer-layout outputs are written,
    in place; es = 1: de-interleaved track planes."""
    M = W_d.shape[0]
    N, D = x_d.shape[0], x_d.shape[1] // M
    if es == 1:
        v0 = x_d.view(N, D, M).permute(2, 0, 1).contiguous()
        gv = None if given is None else given.view(N, D, M).permute(2, 0, 1).contiguous()
        p_v = torch.full((M, N, D), -1.0, device=DEV)
        v_out = torch.full((M, N, D), 7, device=DEV, dtype=torch.uint8)
        jobs = [dict(v0=v0[m], W=W_d[m], bh=bh[m], bv=bv[m], seed=seed + m, p_v=p_v[m], v_out=v_out[m], given=None if gv is None else gv[m])
                for m in range(M)]
        ops.rbm_gibbs_multi(jobs, k, **kw)
        return p_v, v_out
    p_v = torch.full((N, D * M), -1.0, device=DEV)
    v_out = torch.full((N, D * M), 7, device=DEV, dtype=torch.uint8)
    jobs = [dict(v0=x_d[:, m::M], W=W_d[m], bh=bh[m], bv=bv[m], seed=seed + m, p_v=p_v[:, m::M], v_out=v_out[:, m::M],
                 given=None if given is None else given[:, m::M]) for m in range(M)]
    ops.rbm_gibbs_multi(jobs, k, **kw)
    return p_v.view(N, D, M).permute(2, 0, 1).contiguous(), v_out.view(N, D, M).permute(2, 0, 1).contiguous()


def check_grouped(ops, N, D, Hn, M, bcast, k, seed):
    R, W, out, x = multi_problem(N, D, Hn, M, bcast, seed)
    W_d, out_d, x_d = dev(W), dev(out), dev(x)
    bh, bv = bias_views(out_d, M, D, Hn)
    rows = dev((R.permutation(4 * N)[:N] + 1000).astype(np.int32))
    codes = dev(TC.random_codes(R, (N, D * M), 0.4))
    step = torch.tensor([5], device=DEV, dtype=torch.int32)
    for kw, given in ((dict(row0=500, sub0=3), None), (dict(row_ids=rows, sub0=1), None), (dict(row0=9, sub0=2), codes),
                      (dict(row_ids=rows, sub0=0), codes), (dict(row_ids=rows, sub0=0, seed_step=step), None)):
        p_ref, v_ref = single_launches(ops, x_d, W_d, bh, bv, k, seed, given=given, **kw)
        for es in (1, M):
            p_v, v = grouped_launch(ops, x_d, W_d, bh, bv, k, seed, es, given=given, **kw)
            assert torch.equal(v, v_ref), (es, sorted(kw), given is not None)
            assert torch.equal(p_v, p_ref), (es, sorted(kw), given is not None)
        if given is not None:
            g = given.view(N, D, M).permute(2, 0, 1)
            assert torch.equal(v_ref[g != FREE], g[g != FREE])


@pytest.mark.parametrize("N,D,Hn,bcast", TC.FORMS)
@pytest.mark.parametrize("k", [0, 1, 10])
def test_grouped_gibbs_equals_single_launches_in_every_form(ops, N, D, Hn, bcast, k):
    check_grouped(ops, N, D, Hn, 3, bcast, k, seed=D + 11 * k)


@pytest.mark.parametrize("N", [72, 2048, 2117])
@pytest.mark.parametrize("M", [1, 3, 5])
@pytest.mark.parametrize("k", [0, 1, 10])
def test_grouped_gibbs_equals_single_launches_at_real_widths(ops, N, M, k):
    check_grouped(ops, N, 88, 256, M, False, k, seed=N + M)


def test_grouped_gibbs_against_the_checker(ops):
    N, D, Hn, M, k, seed = 21, 88, 256, 3, 4, 31
    R, W, out, x = multi_problem(N, D, Hn, M, False, 77)
    W_d, out_d, x_d = dev(W), dev(out), dev(x)
    bh, bv = bias_views(out_d, M, D, Hn)
    rows = np.arange(300, 300 + N)
    p_v, v = grouped_launch(ops, x_d, W_d, bh, bv, k, seed, M, row0=300, sub0=2)
    for m in range(M):
        u_h, u_v = G.gibbs_uniforms(seed + m, rows, k, Hn, D, sub0=2)
        p_ref, v_ref = det.rbm_gibbs(x[:, m::M], W[m], out[:, m * Hn:(m + 1) * Hn], out[:, M * Hn + m * D:M * Hn + (m + 1) * D], k, u_h, u_v)
        assert np.array_equal(v[m].cpu().numpy(), v_ref), m
        assert np.array_equal(p_v[m].cpu().numpy(), p_ref), m


@pytest.mark.parametrize("N,D,Hn,M,bcast", [(72, 88, 256, 5, False), (2117, 88, 256, 3, False), (9, 30, 20, 8, True), (33, 300, 100, 2, False)])
def test_grouped_free_energy(ops, N, D, Hn, M, bcast):
    R, W, out, x = multi_problem(N, D, Hn, M, bcast, N + D)
    W_d, out_d = dev(W), dev(out)
    bh, bv = bias_views(out_d, M, D, Hn)
    v = dev(np.ascontiguousarray(x.reshape(N, D, M).transpose(2, 0, 1)))
    F = torch.full((M, N), 7.0, device=DEV)
    p_h = torch.full((M, N, Hn), 7.0, device=DEV)
    ops.rbm_free_energy_multi([dict(v=v[m], W=W_d[m], bh=bh[m], bv=bv[m], F=F[m], p_h=p_h[m]) for m in range(M)])
    F2 = torch.full((M, N), 7.0, device=DEV)
    ops.rbm_free_energy_multi([dict(v=v[m], W=W_d[m], bh=bh[m], bv=bv[m], F=F2[m]) for m in range(M)])
    assert torch.equal(F2, F)
    for m in range(M):
        F1, p1 = torch.empty(N, device=DEV), torch.empty((N, Hn), device=DEV)
        ops.rbm_free_energy(v[m], W_d[m], bh[m].contiguous(), bv[m].contiguous(), F1, p_h=p1)
        assert torch.equal(F[m], F1) and torch.equal(p_h[m], p1), m
        ref = ORBM.free_energy(v[m].cpu().numpy().astype(np.float64), W[m].astype(np.float64), out[:, m * Hn:(m + 1) * Hn].astype(np.float64),
                               out[:, M * Hn + m * D:M * Hn + (m + 1) * D].astype(np.float64))
        assert np.abs(F[m].cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max(), m


# ================================================================================================
# model: the float64 restatement
import test_gpu_state0 as TS   # noqa: E402
import test_gpu_ais as TA   # noqa: E402
from test_gpu_realmodes import FWD_TOL, GRAD_TOL   # noqa: E402


def glorot(rng, a, b):
    lim = np.sqrt(6.0 / (a + b))
    return rng.uniform(-lim, lim, (a, b))


def init_params(seed, D, Hn, units, M, rho=0.05):
    """float64 parameters of an RnnMultiRBM over M * D inputs: lstm, per-track W / bh [1,Hn] / bv [1,D], Wuh [R, M Hn], Wuv [R, M D]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = dict(lstm=G.init_lstm(rng, M * D, units, np.float64))
    p['W'] = [glorot(rng, D, Hn) for _ in range(M)]
    p['bh'] = [np.full((1, Hn), 0.05 * m) for m in range(M)]
    p['bv'] = [np.full((1, D), np.log(rho / (1 - rho))) + 0.01 * m for m in range(M)]
    p['Wuh'], p['Wuv'] = glorot(rng, units[-1], M * Hn), glorot(rng, units[-1], M * D)
    return p


def load_params(gen, p, c0=None):
    s = gen.store
    f = lambda a: TM.dev(np.asarray(a, np.float32))
    with torch.no_grad():
        for l, (W, b) in enumerate(p['lstm']):
            s[f"rnn/cell_{l}/kernel"].copy_(f(W)); s[f"rnn/cell_{l}/bias"].copy_(f(b))
            if c0 is not None:
                s[f"rnn/cell_{l}/c0"].copy_(f(c0[l]))
        for m in range(len(p['W'])):
            s[f"rbm_{m}/W"].copy_(f(p['W'][m])); s[f"rbm_{m}/bh"].copy_(f(p['bh'][m])); s[f"rbm_{m}/bv"].copy_(f(p['bv'][m]))
        s["Wuh"].copy_(f(p['Wuh'])); s["Wuv"].copy_(f(p['Wuv']))
    gen._packed_step = -1


def multirbm_oracle(inp, tgt, p, k, seed, keep_prob, units, lengths=None, c0=None, internal_bias=True, bias_mode="conditional", v_samples=None):
    """The model in float64: ONE shared LSTM, one Dense [bh_0 .. | bv_0 ..] (+ the concatenated internal biases), per track a CD-k chain
    with the Philox uniforms of seed + m and cost_m = F_m(target_m) - F_m(v_s,m); loss = mean over tracks of the row-weighted costs.
    v_samples (per track, API rows): chain ends to take instead of the float64 chain's -- costs and gradients on identical samples.
    Returns (fw, grads by variable name)."""
    B, T, _ = inp.shape
    M, (D, Hn) = len(p['W']), p['W'][0].shape
    init = TS.state_of(c0, B) if c0 is not None else None
    du = G.dropout_uniforms(seed, B, T, units)
    y, _, cache = OL.seq_fwd(inp, p['lstm'], keep_prob, du, lengths, 'decode' if c0 is not None else 'dynamic_rnn', init_state=init)
    valid = np.ones((B, T), bool) if lengths is None else (np.arange(T)[None, :] < np.asarray(lengths)[:, None])
    yf = y[valid]
    N = yf.shape[0]
    ib = 1.0 if internal_bias else 0.0
    out_h = yf @ p['Wuh'] + ib * np.concatenate(p['bh'], 1)
    out_v = yf @ p['Wuv'] + ib * np.concatenate(p['bv'], 1)
    rows = (np.arange(T)[None, :] * 65536 + np.arange(B)[:, None])[valid]
    rw = G.row_weights(lengths, B, T, np.float64)
    assert rw.shape[0] == N
    v0s, tgs = inp[valid].reshape(N, D, M), tgt[valid].reshape(N, D, M)
    fw = dict(F=[], cost=[], v_s=[], agree=1.0)
    g = {}
    d_h, d_v = np.zeros((N, M * Hn)), np.zeros((N, M * D))
    for m in range(M):
        bh_t, bv_t = out_h[:, m * Hn:(m + 1) * Hn], out_v[:, m * D:(m + 1) * D]
        u_h, u_v = G.gibbs_uniforms(seed + m, rows, k, Hn, D)
        _, v_s = ORBM.gibbs(v0s[..., m], p['W'][m], bh_t, bv_t, k, u_h, u_v)
        if v_samples is not None:
            fw['agree'] = min(fw['agree'], float((v_samples[m] == v_s).all(1).mean()))
            v_s = v_samples[m].astype(np.float64)
        if bias_mode == "conditional":
            bh_u, bv_u = bh_t, bv_t
        else:
            bh_u, bv_u = np.broadcast_to(p['bh'][m], bh_t.shape), np.broadcast_to(p['bv'][m], bv_t.shape)
        cost, F = ORBM.free_energy_cost(tgs[..., m], v_s, p['W'][m], bh_u, bv_u)
        dW, dbh, dbv = ORBM.free_energy_cost_bwd(tgs[..., m], v_s, p['W'][m], bh_u, bv_u, rw / M)
        fw['F'].append(F); fw['cost'].append(cost); fw['v_s'].append(v_s)
        reaches = internal_bias or bias_mode != "conditional"
        g[f"rbm_{m}/W"], g[f"rbm_{m}/bh"], g[f"rbm_{m}/bv"] = dW, dbh.sum(0, keepdims=True) * reaches, dbv.sum(0, keepdims=True) * reaches
        d_h[:, m * Hn:(m + 1) * Hn], d_v[:, m * D:(m + 1) * D] = dbh, dbv
    fw['loss'] = float(np.mean([(rw * c).sum() for c in fw['cost']]))
    fw['free_energy'] = float(np.mean([(rw * F).sum() for F in fw['F']]))
    if bias_mode == "conditional":
        g['Wuh'], g['Wuv'] = yf.T @ d_h, yf.T @ d_v                      # the Dense gradient sums over the tracks' blocks
        dy = np.zeros((B, T, yf.shape[1]))
        dy[valid] = d_h @ p['Wuh'].T + d_v @ p['Wuv'].T
        _, lg = OL.seq_bwd(dy, cache)
        c0g = TS.state_grads(cache, dy, c0)[1] if c0 is not None else None
    else:
        g['Wuh'], g['Wuv'] = np.zeros_like(p['Wuh']), np.zeros_like(p['Wuv'])
        lg = [(np.zeros_like(W), np.zeros_like(b)) for W, b in p['lstm']]
        c0g = [np.zeros_like(c) for c in c0] if c0 is not None else None
    for l, (dW, db) in enumerate(lg):
        g[f"rnn/cell_{l}/kernel"], g[f"rnn/cell_{l}/bias"] = dW, db
        if c0g is not None:
            g[f"rnn/cell_{l}/c0"] = c0g[l]
    return fw, g


def compare(gen, inp, tgt, p, k, units, keep_prob, lengths=None, c0=None, internal_bias=True, bias_mode="conditional"):
    """Device forward (already built in train mode) and backward against the restatement, on the device's own chain ends.
    -> dict(free_energy, loss, agree, grads: name -> rel err)."""
    vs = [v.cpu().numpy() for v in gen._outputs]
    fw, g = multirbm_oracle(inp, tgt, p, k, gen.seed, keep_prob, units, lengths, c0, internal_bias, bias_mode, v_samples=vs)
    res = dict(agree=fw['agree'])
    res['free_energy'] = max(TM.rel(F.cpu().numpy(), fw['F'][m]) for m, F in enumerate(gen.free_energy))
    res['cost'] = max(np.abs(c.cpu().numpy() - fw['cost'][m]).max() / max(1.0, np.abs(fw['cost'][m]).max()) for m, c in enumerate(gen.cost))
    res['loss'] = abs(float(gen.metrics["batch/loss"]) - fw['loss']) / max(1.0, abs(fw['loss']))
    res['fe_metric'] = abs(float(gen.metrics["free_energy"]) - fw['free_energy']) / max(1.0, abs(fw['free_energy']))
    gen.backward()
    gen.check()
    assert sorted(g) == sorted(gen.store.names())
    res['grads'] = {n: TM.rel(gen.store.gviews[n].cpu().numpy().reshape(g[n].shape), g[n]) if np.abs(g[n]).max() > 0
                    else float(gen.store.gviews[n].abs().max()) for n in gen.store.names()}
    return res


P, M5, HN, UNITS = 88, 5, 256, [512, 256]


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_composer_multirbm_real_widths(precision):
    """P = 88, M = 5, Hn = 256, LSTM [512, 256], CD-10, B = 16, T = 8, keep_prob 0.9 through the composer mode, by the method and bounds of
    test_gpu_realmodes.py::test_c3_jamming_real_widths."""
    from multinn_amd import MultINN
    B, T, k = 16, 8, 10
    x = TM.batch(B, T, P, M5, 8, rho=0.05)
    m = MultINN(TM.config(P, TM.TRACKS5), TM.params("composer", gen="MultiRBM", Hn=HN, units=UNITS), mode="composer", precision=precision)
    m.build(TM.dev(x), lengths=None, is_train=True, mode="train")
    g = m.generators[0]
    p = init_params(50, P, HN, UNITS, M5)
    load_params(g, p)
    m.build(TM.dev(x), lengths=None, is_train=True, mode="train")
    inp, tgt = G.joint_inputs(x.astype(np.float64))                     # composer layout: feature p * M + m, one zero step in front
    res = compare(g, inp, tgt, p, k, UNITS, 0.9)
    gerr = max(res['grads'].values())
    print(f"\n[composer MultiRBM {precision}] free energy {res['free_energy']:.2e}  loss {res['loss']:.2e}  rows whose Gibbs chain end equals the "
          f"float64 chain's {res['agree']:.3f}  gradients {gerr:.2e}")
    assert res['agree'] >= 0.99, res
    assert res['free_energy'] < FWD_TOL[precision] and res['loss'] < FWD_TOL[precision] and res['fe_metric'] < FWD_TOL[precision], res
    assert abs(float(m.generator_loss()) - float(g.metrics["batch/loss"])) == 0.0
    assert gerr < GRAD_TOL[precision], res['grads']


@pytest.mark.parametrize("ragged,internal_bias,bias_mode,learned", [(True, True, "conditional", False), (False, False, "conditional", True),
                                                                    (True, True, "internal", False), (False, True, "conditional", True)])
def test_multirbm_small_shapes_fp32(ragged, internal_bias, bias_mode, learned):
    """Ragged lengths, internal_bias both ways, bias_mode both ways, the learned initial state (its c0 gradients against the float64
    autograd restatement of test_gpu_state0, at that file's fp32 bound: 1e-4 like every gradient)."""
    from multinn_amd import RnnMultiRBM
    B, T, D, Hn, units, M, k = 5, 6, 12, 16, [32, 32], 3, 3
    rng = np.random.default_rng(3)
    seq = (rng.random((B, T + 1, D * M)) < 0.2).astype(np.float64)
    inp, tgt = seq[:, :-1], seq[:, 1:]
    lengths = np.array([6, 3, 5, 1, 4]) if ragged else None
    p = init_params(9, D, Hn, units, M, rho=0.2)
    c0 = [np.random.default_rng(5 + l).normal(0, 0.3, (1, u)) for l, u in enumerate(units)] if learned else None
    g = RnnMultiRBM(D, Hn, units, tracks=list("abc"), keep_prob=0.9, internal_bias=internal_bias, k=k, bias_mode=bias_mode, precision="fp32",
                    seed=23, learn_zero_state=learned)
    g._materialize(D * M)
    load_params(g, p, c0)
    g.build(TM.dev(inp.astype(np.uint8)), TM.dev(tgt.astype(np.uint8)), None if lengths is None else torch.from_numpy(lengths).int(), True, "train")
    res = compare(g, inp, tgt, p, k, units, 0.9, lengths, c0, internal_bias, bias_mode)
    print(f"\n[small ragged={ragged} ib={internal_bias} {bias_mode} learned={learned}] {res}")
    n_valid = B * T if lengths is None else int(lengths.sum())
    assert all(len(t) == M and t[0].shape[0] == n_valid for t in (g.cost, g.free_energy, g.cond_probs, g.reconstruction_cost, g._outputs))
    assert res['agree'] >= 0.99
    assert res['free_energy'] < 1e-4 and res['loss'] < 1e-4 and res['cost'] < 1e-4 and res['fe_metric'] < 1e-4, res
    assert max(res['grads'].values()) < 1e-4, res['grads']
    if learned:
        assert all(float(g.store.gviews[f"rnn/cell_{l}/c0"].abs().max()) > 0 for l in range(2))


def test_multirbm_captured_step_equals_eager():
    """graphed_build_train: replays are steps 3, 4, 5 of the eager trajectory (dropout masks, the M chains' uniforms and Adam's step follow
    the device step counter); the bounds of test_gpu_generators.py::test_graphed_build_train_matches_eager."""
    from multinn_amd import RnnMultiRBM, AdamOptimizer
    B, T, E, M = 8, 6, 12, 3
    R = np.random.default_rng(4)
    seq = (R.random((B, T + 1, E * M)) < .25).astype(np.float32)
    x, y = TM.dev(seq[:, :-1]), TM.dev(seq[:, 1:])
    make = lambda: RnnMultiRBM(E, 20, [128, 128], tracks=list("abc"), keep_prob=0.9, k=3, precision="bf16", seed=3)
    a, b = make(), make()
    a._materialize(E * M); b._materialize(E * M)
    b.store.theta.copy_(a.store.theta)
    opt = AdamOptimizer(0.01)

    def eager_step():
        a.build(x, y, None, True, "train")
        a.train(opt, 0.01)
        return float(a._loss)

    run = b.graphed_build_train(x, y, opt, 0.01, warmup=2)
    la = [eager_step() for _ in range(5)]
    lb = [float(run()) for _ in range(3)]
    assert np.allclose(lb, la[2:], rtol=5e-3, atol=1e-4), (la, lb)
    assert len(set(np.round(lb, 6))) == 3                      # every replay is a different step
    assert b.store.step == 5 and int(b.store.step_dev) == 5
    assert torch.allclose(a.store.theta, b.store.theta, atol=3e-3)


# ------------------------------------------------------------------------------------------------
# generation: the step-by-step checker
def f32p(p):
    return dict(lstm=[(det.f32(W), det.f32(b)) for W, b in p['lstm']], W=[det.f32(w) for w in p['W']], Wuh=det.f32(p['Wuh']), Wuv=det.f32(p['Wuv']),
                bh=det.f32(np.concatenate(p['bh'], 1).reshape(-1)), bv=det.f32(np.concatenate(p['bv'], 1).reshape(-1)))


def checker_generate(intro, num_steps, p, k, seed, internal_bias=True, state0=None, codes=None):
    """RnnMultiRBM.generate in the deterministic float32 arithmetic: intro pass through the shared LSTM (from state0), then per step the two
    Dense products, per track a k-step (clamped) chain from its slice of the previous row with the uniforms of seed + m (row = batch index,
    sub = step * k + iteration), and an LSTM step on the composer-layout row.  intro u8 [B, Ti, D * M] -> u8 [B, num_steps, D * M]."""
    q = f32p(p)
    B, Ti, DM = intro.shape
    M, (D, Hn) = len(q['W']), q['W'][0].shape
    state, h = state0, None
    for t in range(Ti):
        h, state = det.lstm_step(intro[:, t], state, q['lstm'])
    rows = np.arange(B, dtype=np.uint32)
    prev = np.ascontiguousarray(intro[:, -1], np.uint8)
    out = np.empty((B, num_steps, DM), np.uint8)
    for s in range(num_steps):
        oh = det.dense(h, q['Wuh'], q['bh'] if internal_bias else None)
        ov = det.dense(h, q['Wuv'], q['bv'] if internal_bias else None)
        row = np.empty((B, D, M), np.uint8)
        for m in range(M):
            u_h, u_v = G.gibbs_uniforms(seed + m, rows, k, Hn, D, sub0=s * max(k, 1))
            bh_t, bv_t = oh[:, m * Hn:(m + 1) * Hn], ov[:, m * D:(m + 1) * D]
            v0 = prev.reshape(B, D, M)[..., m]
            if codes is None:
                _, v = det.rbm_gibbs(v0, q['W'][m], bh_t, bv_t, k, u_h, u_v)
            else:
                _, v = TC.clamped_gibbs(v0, q['W'][m], bh_t, bv_t, k, u_h, u_v, codes[:, s].reshape(B, D, M)[..., m])
            row[..., m] = v
        prev = row.reshape(B, DM)
        out[:, s] = prev
        h, state = det.lstm_step(prev, state, q['lstm'])
    return out


def real_generator(internal_bias=True, learned=False, seed=23):
    from multinn_amd import RnnMultiRBM
    g = RnnMultiRBM(P, HN, UNITS, tracks=TM.TRACKS5, keep_prob=0.9, internal_bias=internal_bias, k=10, precision="fp16", seed=seed,
                    learn_zero_state=learned)
    g._materialize(P * M5)
    p = init_params(61, P, HN, UNITS, M5)
    rng = np.random.default_rng(2)
    p['W'] = [w * 3.0 for w in p['W']]                                   # livelier chains than the glorot start
    c0 = [rng.normal(0, 0.3, (1, u)) for u in UNITS] if learned else None
    load_params(g, p, c0)
    # the checker reads the parameters back from the device (their f32 bits)
    s = g.store
    q = dict(lstm=[(s[f"rnn/cell_{l}/kernel"].cpu().numpy(), s[f"rnn/cell_{l}/bias"].cpu().numpy()) for l in range(2)],
             W=[s[f"rbm_{m}/W"].cpu().numpy() for m in range(M5)], bh=[s[f"rbm_{m}/bh"].cpu().numpy() for m in range(M5)],
             bv=[s[f"rbm_{m}/bv"].cpu().numpy() for m in range(M5)], Wuh=s["Wuh"].cpu().numpy(), Wuv=s["Wuv"].cpu().numpy())
    return g, q


@pytest.fixture(scope="module")
def scan72():
    """72 intros x 16 steps at real widths, shared by the generation and conditional tests: (generator, params, intro, device samples,
    checker samples)."""
    g, q = real_generator()
    intro = (np.random.default_rng(7).random((72, 4, P * M5)) < 0.05).astype(np.uint8)
    dev_s = g.generate(TM.dev(intro), 16).cpu().numpy()
    ref = checker_generate(intro, 16, q, 10, g.seed)
    return g, q, intro, dev_s, ref


def test_generation_bit_exact(scan72):
    g, q, intro, dev_s, ref = scan72
    assert dev_s.shape == (72, 16, P * M5) and dev_s.dtype == np.uint8
    assert 0.001 < ref.mean() < 0.6
    assert np.array_equal(dev_s, ref)
    again = g.generate(TM.dev(intro), 16).cpu().numpy()                  # the captured scan replayed
    assert np.array_equal(again, ref)


@pytest.mark.parametrize("internal_bias,learned", [(False, False), (True, True)])
def test_generation_bit_exact_variants(internal_bias, learned):
    g, q = real_generator(internal_bias, learned, seed=31)
    intro = (np.random.default_rng(8).random((72, 3, P * M5)) < 0.05).astype(np.uint8)
    st0 = TS._device_state(g, 72) if learned else None
    ref = checker_generate(intro, 16, q, 10, g.seed, internal_bias, st0)
    assert np.array_equal(g.generate(TM.dev(intro), 16).cpu().numpy(), ref)


def test_conditional_generation(scan72):
    g, q, intro, free_s, free_ref = scan72
    B, S = 72, 16
    rng = np.random.default_rng(12)
    given = (rng.random((B, S, P, M5)) < 0.08).astype(np.uint8)
    # 1. a whole given track: returned as given, the others equal the checker's with it clamped
    codes = np.full((B, S, P, M5), FREE, np.uint8)
    codes[..., 2] = given[..., 2]
    codes = codes.reshape(B, S, P * M5)
    out = g.generate(TM.dev(intro), S, given=TM.dev(codes)).cpu().numpy()
    assert np.array_equal(out.reshape(B, S, P, M5)[..., 2], given[..., 2])
    assert np.array_equal(out, checker_generate(intro, S, q, 10, g.seed, codes=codes))
    # 2. a partial mask: bit-exact against the checker's clamped chain
    part = np.where(rng.random((B, S, P * M5)) < 0.3, given.reshape(B, S, -1), FREE).astype(np.uint8)
    out = g.generate(TM.dev(intro), S, given=TM.dev(part)).cpu().numpy()
    assert np.array_equal(out[part != FREE], part[part != FREE])
    assert np.array_equal(out, checker_generate(intro, S, q, 10, g.seed, codes=part))
    # 3. all-free codes: the unconditioned samples
    allfree = torch.full((B, S, P * M5), FREE, device=DEV, dtype=torch.uint8)
    assert np.array_equal(g.generate(TM.dev(intro), S, given=allfree).cpu().numpy(), free_s)


# ------------------------------------------------------------------------------------------------
# likelihood
def tiny_multirbm(seed=5):
    from multinn_amd import RnnMultiRBM
    g = RnnMultiRBM(10, 8, [32, 32], tracks=["a", "b"], precision="fp32", seed=seed)
    g._materialize(20)
    R = np.random.default_rng(seed)
    with torch.no_grad():
        for m in range(2):
            g.store[f"rbm_{m}/W"].copy_(TM.dev((R.standard_normal((10, 8)) * 0.5).astype(np.float32)))
        g.store["Wuh"].mul_(3.0)
        g.store["Wuv"].mul_(3.0)
    g._packed_step = -1
    return g


def test_multirbm_estimate_matches_exact_nll():
    """Per-track log Z enumerable (8 hidden units): the estimate within max(0.02, 4 stderr) per row of the exact NLL summed over tracks
    (the bound of test_gpu_ais.py::test_rnn_rbm_estimate_matches_exact_nll)."""
    g = tiny_multirbm()
    M, D, Hn = 2, 10, 8
    x = TM.dev((np.random.default_rng(0).random((3, 5, D * M)) < 0.25).astype(np.uint8))
    est = g.estimate_nll(x, num_chains=256, num_betas=2000)
    out = g._ctx["out"][g._idx()].double().cpu().numpy()
    v = x.reshape(-1, D, M).cpu().numpy().astype(np.float64)              # API order: b-major, then t
    ref = np.zeros(15)
    Fsum = np.zeros(15)
    for m in range(M):
        bh, bv = out[:, m * Hn:(m + 1) * Hn], out[:, M * Hn + m * D:M * Hn + (m + 1) * D]
        W = g.store[f"rbm_{m}/W"].double().cpu().numpy()
        F = -(v[..., m] * bv).sum(1) - TA.softplus(bh + v[..., m] @ W).sum(1)
        Fsum += F
        ref += F + TA.exact_log_z_hidden(W, bh, bv)
    nll = est.nll.cpu().numpy()
    assert nll.shape == (15,) and np.isfinite(est.mean)
    np.testing.assert_allclose(est.free_energy.cpu().numpy(), Fsum, rtol=1e-5, atol=1e-4)
    tol = np.maximum(0.02, 4 * est.row_stderr.cpu().numpy())
    assert np.all(np.abs(nll - ref) <= tol), (np.abs(nll - ref).max(), tol.max())
    assert est.ess > 1 and abs(est.mean - nll.mean()) < 1e-5


# ------------------------------------------------------------------------------------------------
# composer mode end to end
@pytest.mark.parametrize("enc,enc_hidden", [("Pass", None), ("DBN", [14, 10])])
def test_composer_mode_end_to_end(enc, enc_hidden, tmp_path):
    from multinn_amd import MultINN, AdamOptimizer
    from multinn_amd._lib import MnnUnsupported
    Pn, tracks, B, T = 12, ["Drums", "Piano", "Bass"], 6, 8
    cfg = TM.config(Pn, tracks)
    prm = TM.params("composer", enc=enc, enc_hidden=enc_hidden, gen="MultiRBM", Hn=16, units=(32, 32))
    prm["generator"]["k"] = 3
    x = TM.dev(TM.batch(B, T, Pn, 3, 5, rho=0.2))
    m = MultINN(cfg, prm, mode="composer", precision="fp32")
    opt = AdamOptimizer(0.01)
    losses = [float(m.train_step(x, None, opt, 0.01)) for _ in range(3)]
    m.check()
    assert np.all(np.isfinite(losses)) and len(set(np.round(losses, 6))) == 3, losses
    m.build(x, lengths=None, is_train=False, mode="eval")
    ev = m.metrics
    assert np.isfinite(float(m.generator_loss())) and np.isfinite(float(ev["batch/loss"]))
    s1 = m.generate(5)
    assert tuple(s1.shape) == (B, 5, Pn, 3) and s1.dtype == torch.uint8
    assert tuple(m.sampler(1).shape)[0] == B
    m.save(None, str(tmp_path))
    m2 = MultINN(cfg, prm, mode="composer", precision="fp32")
    assert m2.load(None, str(tmp_path))
    m2.build(x, lengths=None, is_train=False, mode="eval")
    assert torch.equal(m2.generate(5), s1)
    # pretraining (one CD-k update per track RBM, the documented 5-tuple) and the captured mode step
    m.build(x, lengths=None, is_train=True, mode="train")
    w_before = [m.generators[0].store[f"rbm_{i}/W"].clone() for i in range(3)]
    ret = m.pretrain_generators(opt, 0.01)
    assert len(ret) == 5 and all(not torch.equal(m.generators[0].store[f"rbm_{i}/W"], w) for i, w in enumerate(w_before))
    assert m.capturable(tuple(x.shape), False)
    run = m.graphed_train_step(x, opt, 0.01, warmup=1)
    captured = [float(run()) for _ in range(2)]
    m.check()
    assert np.all(np.isfinite(captured)) and captured[0] != captured[1], captured
    if enc == "Pass":
        given = (torch.rand((B, 5, Pn, 3), device=DEV) < 0.2).to(torch.uint8)
        for mask in (torch.tensor([True, False, False]), torch.zeros((Pn, 3), dtype=torch.bool).index_fill_(0, torch.arange(4), True),
                     torch.rand((B, 5, Pn, 3)) < 0.3):
            out = m.generate(5, given=given, given_mask=mask.to(DEV))
            mk = mask.to(DEV).expand(B, 5, Pn, 3)
            assert torch.equal(out[mk], given[mk])
        est = m.estimate_nll(x, num_chains=16, num_betas=50)
        assert est.nll.numel() == B * T and np.isfinite(est.mean) and est.stderr > 0
    else:
        with pytest.raises(MnnUnsupported):
            m.estimate_nll(x, num_chains=4, num_betas=10)


def test_driver_epoch_replays_captured_composer_multirbm_steps(monkeypatch):
    """driver.train_epoch on the composer mode with generator type MultiRBM: recurring window shapes -- full-length and ragged (row weights,
    valid-row count and f16 loss scale derived on the device) -- run as replays of the mode's captured step; the loss trajectory of three
    epochs is the eager loop's, at the bound of test_gpu_modes.py::test_driver_epoch_replays_captured_mode_steps."""
    from multinn_amd import MultINN, AdamOptimizer
    from multinn_amd.driver import train_epoch, LossAccumulator, TrainingStats
    R = np.random.default_rng(6)
    Pn, tracks = 8, TM.TRACKS5[:3]
    X = (R.random((16, 12, Pn, len(tracks))) < .2).astype(np.uint8)
    lengths = np.full(16, 12)
    lengths[3] = 7
    ids = np.arange(16)

    def epoch_losses(graph):
        if not graph:
            monkeypatch.setenv("MULTINN_TRAIN_GRAPH", "0")
        m = MultINN(TM.config(Pn, tracks), TM.params("composer", gen="MultiRBM", Hn=32, units=(128, 128)), mode="composer", precision="fp16", seed=23)
        opt = AdamOptimizer(0.01)
        out = []
        for _ in range(3):
            acc = LossAccumulator()
            train_epoch(m, X, lengths, ids, 8, 4, opt, acc, TrainingStats(), lr=0.01, device=DEV)
            out.append(acc.loss())
        if not graph:
            monkeypatch.delenv("MULTINN_TRAIN_GRAPH")
        m.check()
        return out, m

    lg, mg = epoch_losses(True)
    le, me = epoch_losses(False)
    keys = list(mg.__dict__.get("_step_graphs", {}))
    assert any(k[-1] == "ragged" for k in keys) and any(k[-1] == "full" for k in keys), keys
    assert "_step_graphs" not in me.__dict__
    assert np.allclose(lg, le, rtol=2e-2), (lg, le)
