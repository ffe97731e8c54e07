"""RAGGED windows (songs that end inside a window: `lengths`) of the LSTM-RBM and multi-track NADE train steps against the float64 oracle,
which takes `lengths` through flatten_maybe_padded_sequences / sequence_mask (oracle/generators.py; pinned on the CPU by
test_oracle_kats.test_rnn_rbm_ragged_lengths_equal_truncated_sequences_and_fd):

    A  RnnRBM generator, fp32, small shapes: per-row values, metrics, every gradient, one clipped Adam step, then an eval build
    B  jamming mode (5 x LSTM-RBM CD-10) at the reference's widths, fp32 / fp16 / bf16, persistent recurrence
    C  the same mode in lockstep (`group_generators`, B = 256), fp16
    D  the CAPTURED ragged step (`MultINNCore.graphed_train_step(lengths=...)`, `RnnEstimator.ragged_on_device`): three replays on different
       length vectors, each against the oracle at the weights and the step counter read back before it -- RBM and NADE generators
    E  RnnMultiNADE generator: fp32 (padding rows kept) and bf16 / fp16 (rows compacted)

Row ids of a ragged window, API order (b-major, then t): t * 65536 + b.  As in the other RBM tests the oracle's cost, free energy and gradients
are evaluated on the device's own chain ends, after the chains have been compared: at most max(1, ceil(N / 100)) of the N valid rows may end
their Gibbs chain differently from the float64 chain (a draw differs only where a probability sits within f32 rounding of its uniform).
Tolerances: fp32 1e-4 relative (2e-4 absolute on weights after Adam); real widths FWD_TOL / GRAD_TOL of test_gpu_realmodes; E in 16 bits the
6e-2 (gradients: twice that) of test_rnn_nade_joint_train_step.  Every case also asserts that its inputs DISCRIMINATE: the oracle's
full-length loss and W (w_dec) gradient on the same batch miss the ragged reference by at least ten times the tolerance used beside them, so
a device that ignored `lengths` could not pass."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_gpu_modes as TM   # noqa: E402
from test_gpu_realmodes import FWD_TOL, GRAD_TOL, P, M, HN, UNITS   # noqa: E402
from oracle import generators as G, rbm as orbm   # noqa: E402


def row_ids(lengths):
    return np.array([t * 65536 + b for b in range(len(lengths)) for t in range(int(lengths[b]))], np.int64)


def chain_cap(n):
    return max(1, math.ceil(0.01 * n))


def chains_differing(vs, ref):
    return int((vs != ref).any(1).sum())


def on_chain_ends(fw, vs):
    """The oracle's forward record with the device's chain ends in place of its own (a copy: cached records stay as they are)."""
    out = dict(fw)
    out['v_sample'] = vs.astype(np.float64)
    return out


def loud_padding(x, lengths, seed=77):
    """x [B, T, P, M] with the steps behind each sequence's end replaced by dense noise (half the cells set, ten times the music's density):
    whatever the kernels compute on padding rows must not reach a loss, a metric or a gradient -- and a full-length evaluation of the same
    batch then lands far from the ragged one."""
    noise = (np.random.default_rng(seed).random(x.shape) < 0.5).astype(x.dtype)
    for b, n in enumerate(lengths):
        x[b, int(n):] = noise[b, int(n):]
    return x


def full_rows(B, T):
    return row_ids(np.full(B, T))


def assert_discriminates(what, loss_full, loss_ragged, g_full, g_ragged, tol, gtol, unit_floor=True):
    """A device that ignored `lengths` would report loss_full / g_full: both must miss the ragged reference by >= 10 x the tolerance."""
    dl = abs(loss_full - loss_ragged) / (max(1.0, abs(loss_ragged)) if unit_floor else abs(loss_ragged))
    dg = TM.rel(g_full, g_ragged)
    print(f"\n[{what}] full-length oracle against the ragged one: loss {dl:.3f} (needs {10 * tol:.3g}), W gradient {dg:.3f} (needs {10 * gtol:.3g})")
    assert dl >= 10 * tol and dg >= 10 * gtol, (what, dl, dg)


def rbm_zero_grads(p):
    return dict(lstm=[(np.zeros_like(W), np.zeros_like(b)) for W, b in p['lstm']], Wuh=np.zeros_like(p['Wuh']), Wuv=np.zeros_like(p['Wuv']))


def read_rbm_params(gen):
    """The generator's f32 master weights as float64 oracle parameters."""
    s = gen.store
    f = lambda n: s[n].detach().cpu().numpy().astype(np.float64)
    p = dict(lstm=[(f(f"rnn/cell_{l}/kernel"), f(f"rnn/cell_{l}/bias").reshape(-1)) for l in range(len(gen.num_hidden_rnn))])
    p['W'], p['bh'], p['bv'] = f("rbm/W"), f("rbm/bh").reshape(1, -1), f("rbm/bv").reshape(1, -1)
    p['Wuh'], p['Wuv'] = f("Wuh"), f("Wuv")
    return p


def read_nade_params(gen):
    s = gen.store
    f = lambda n: s[n].detach().cpu().numpy().astype(np.float64)
    p = dict(lstm=[(f(f"rnn/cell_{l}/kernel"), f(f"rnn/cell_{l}/bias").reshape(-1)) for l in range(len(gen.num_hidden_rnn))])
    p['w_enc'], p['w_dec'] = list(f("nade/w_enc")), list(f("nade/w_dec"))
    p['fc_k'], p['fc_b'] = f("dense/kernel"), f("dense/bias").reshape(-1)
    return p


# ------------------------------------------------------------------------------------------------------------------------
# A. RnnRBM generator, fp32
def _check_rbm_rows(gen, fw, p, bias_mode, tag):
    """Per-row values (shape, order, value) and the three metrics of a built RnnRBM against the oracle record `fw`; returns the record on the
    device's chain ends."""
    N, D = fw['tgt'].shape
    vs = gen._outputs.cpu().numpy()
    assert vs.shape == (N, D)
    differ = (vs != fw['v_sample']).any(1)
    assert differ.sum() <= chain_cap(N), (tag, int(differ.sum()))
    fd = on_chain_ends(fw, vs)
    bh_u, bv_u = (fw['bh_t'], fw['bv_t']) if bias_mode == "conditional" else (p['bh'], p['bv'])
    cost, F = orbm.free_energy_cost(fw['tgt'], fd['v_sample'], p['W'], bh_u, bv_u)
    got = {k_: getattr(gen, k_).cpu().numpy() for k_ in ("cost", "free_energy", "reconstruction_cost", "cond_probs")}
    assert got["cost"].shape == (N,) and got["free_energy"].shape == (N,) and got["reconstruction_cost"].shape == (N,) and got["cond_probs"].shape == (N, D)
    same = ~differ                                      # rows whose chains agree have the oracle's last conditional too
    recon = fw['recon'].copy()
    recon[differ] = TM.log_loss_rows(fw['tgt'][differ], got["cond_probs"][differ])
    errs = dict(cost=TM.rel(got["cost"], cost), free_energy=TM.rel(got["free_energy"], F),
                cond_probs=float(np.abs(got["cond_probs"][same] - fw['p_v'][same]).max()),
                reconstruction_cost=TM.rel(got["reconstruction_cost"], recon),
                m_loss=abs(float(gen.metrics["batch/loss"]) - cost.mean()) / max(1.0, abs(cost.mean())),
                m_free_energy=abs(float(gen.metrics["free_energy"]) - F.mean()) / abs(F.mean()),
                m_log_likelihood=abs(float(gen.metrics["log_likelihood"]) - recon.mean()) / abs(recon.mean()))
    print(f"\n[A {tag} {bias_mode}] rows whose chain end differs {int(differ.sum())} / {N}  " + "  ".join(f"{k_} {v:.2e}" for k_, v in errs.items()))
    assert errs["cond_probs"] < 1e-5
    assert all(v < 1e-4 for v in errs.values()), errs
    return fd


@pytest.mark.parametrize("bias_mode", ["conditional", "internal"])
def test_rnn_rbm_ragged_train_and_eval_vs_oracle(bias_mode):
    """RnnRBM on a ragged window (one empty sequence, one of length 1, two full ones), keep_prob 0.9: cost / free_energy /
    reconstruction_cost / cond_probs of the sum(lengths) valid rows in API order, the metrics (means over VALID rows), every gradient, the
    global norm and the weights after one clipped Adam step; then the same batch built for evaluation (keep_prob 1, Gibbs seed + 1 step)."""
    from multinn_amd import RnnRBM, AdamOptimizer
    B, T, D, Hn, units, k, kp, seed = 6, 5, 12, 20, [32, 32], 3, 0.9, 13
    lengths = np.array([5, 0, 3, 5, 1, 4], np.int32)
    x = loud_padding(TM.batch(B, T, D, 1, 8), lengths)
    inp, tgt = G.joint_inputs(x)
    i64, t64 = inp.astype(np.float64), tgt.astype(np.float64)
    p = G.init_rnn_rbm(5, D, D, Hn, units, np.float64)
    p['bh'] += 0.1
    p['bv'] -= 0.2
    gen = RnnRBM(D, Hn, units, keep_prob=kp, k=k, precision="fp32", seed=seed, bias_mode=bias_mode)
    gen.build(TM.dev(inp), TM.dev(tgt), TM.dev(lengths), True, "train")
    TM.load_rbm_params(gen, p)
    gen.build(TM.dev(inp), TM.dev(tgt), TM.dev(lengths), True, "train")
    du = G.dropout_uniforms(seed, B, T, units)
    fw = G.rnn_rbm_forward(i64, t64, lengths, p, k, seed, kp, du, bias_mode, row_ids(lengths))
    full = G.rnn_rbm_forward(i64, t64, None, p, k, seed, kp, du, bias_mode, full_rows(B, T))
    assert_discriminates(f"A {bias_mode}", full['loss'], fw['loss'], G.rnn_rbm_backward(full, p)['W'], G.rnn_rbm_backward(fw, p)['W'], 1e-4, 1e-4)
    fd = _check_rbm_rows(gen, fw, p, bias_mode, "train")
    g = G.rnn_rbm_backward(fd, p)
    gen.backward()
    gv = gen.store.gviews
    if bias_mode == "internal":                         # R3, as written: nothing reaches the LSTM / Wuh / Wuv
        assert all(float(gv[n].abs().max()) == 0 for n in gen.store.names() if not n.startswith("rbm/"))
        g.update(rbm_zero_grads(p))
    gerr = {n: TM.rel(gv[n].cpu().numpy().reshape(r.shape), r) for n, r in zip(gen.store.names(), TM.rbm_grad_list(g)) if np.abs(r).max() > 0}
    assert len(gerr) == (len(gen.store.names()) if bias_mode == "conditional" else 3)
    gn = G.apply_clip_adam(TM.rbm_param_list(p), TM.rbm_grad_list(g), G.new_opt(TM.rbm_param_list(p)), lr=0.01)
    gen.train(AdamOptimizer(0.01), None)
    e_gn = abs(float(gen._grad_sumsq.sqrt()) - gn) / gn
    e_w = max(float(np.abs(gen.store[n].cpu().numpy().reshape(r.shape) - r).max()) for n, r in zip(gen.store.names(), TM.rbm_param_list(p)))
    print(f"\n[A {bias_mode}] gradients {max(gerr.values()):.2e}  global norm {e_gn:.2e}  weights after clip + Adam (abs) {e_w:.2e}")
    assert all(v < 1e-4 for v in gerr.values()), gerr
    assert e_gn < 1e-4 and e_w < 2e-4
    # evaluation build of the same batch at the oracle's stepped weights: no dropout, the Gibbs seed follows the step counter
    TM.load_rbm_params(gen, p)
    assert gen.store.step == 1 and int(gen.store.step_dev) == 1
    gen.build(TM.dev(inp), TM.dev(tgt), TM.dev(lengths), False, "eval")
    fe = G.rnn_rbm_forward(i64, t64, lengths, p, k, seed + 1, 1.0, None, bias_mode, row_ids(lengths))
    _check_rbm_rows(gen, fe, p, bias_mode, "eval")


# ------------------------------------------------------------------------------------------------------------------------
# B, C. jamming mode at the reference's widths
def _c3_params():
    ps = [G.init_rnn_rbm(50 + i, P, P, HN, UNITS, np.float64) for i in range(M)]
    for i, p in enumerate(ps):
        p['bh'] += 0.05 * i
        p['bv'] += np.log(0.05 / 0.95)
    return ps


@functools.lru_cache(maxsize=2)
def _jamming_oracle(B, T, xseed, lengths, seeds, k=10):
    """(x, parameters, one oracle forward record per track, discrimination figures of track 0) of a ragged jamming window; computed once
    per window and shared by the precisions (read-only: on_chain_ends copies)."""
    lengths = np.array(lengths, np.int32)
    x = loud_padding(TM.batch(B, T, P, M, xseed, rho=0.05), lengths)
    ps = _c3_params()
    tracks = G.per_track_inputs(x)
    fws = []
    for i in range(M):
        inp, tgt = tracks[i][:, :-1].astype(np.float64), tracks[i][:, 1:].astype(np.float64)
        du = G.dropout_uniforms(seeds[i], B, T, UNITS)
        fws.append(G.rnn_rbm_forward(inp, tgt, lengths, ps[i], k, seeds[i], 0.9, du, row_ids=row_ids(lengths)))
        if i == 0:
            full = G.rnn_rbm_forward(inp, tgt, None, ps[0], k, seeds[0], 0.9, du, row_ids=full_rows(B, T))
            disc = (full['loss'], fws[0]['loss'], G.rnn_rbm_backward(full, ps[0])['W'], G.rnn_rbm_backward(fws[0], ps[0])['W'])
    return x, ps, fws, disc


def _jamming_ragged_vs_oracle(tag, precision, B, T, lengths, xseed, grouped):
    from multinn_amd import MultINN, AdamOptimizer
    m = MultINN(TM.config(P, TM.TRACKS5), TM.params("jamming", gen="RBM", Hn=HN, units=UNITS), mode="jamming", precision=precision)
    if grouped:
        m.group_generators = True
    x, ps, fws, disc = _jamming_oracle(B, T, xseed, tuple(int(n) for n in lengths), tuple(g.seed for g in m.generators))
    ln = TM.dev(lengths.astype(np.int32))
    m.build(TM.dev(x), lengths=ln, is_train=True, mode="train")
    for i, g in enumerate(m.generators):
        TM.load_rbm_params(g, ps[i])
    m.build(TM.dev(x), lengths=ln, is_train=True, mode="train")
    if grouped:
        assert m._built_grouped and all(g._ctx["lstm"][0].get("rowpar") for g in m.generators), "the lockstep `_multi` launches must be the form under test"
    elif precision != "fp32":
        assert all(g._stack._persist(B, T) for g in m.generators), "the persistent recurrence must be the form under test"
    ftol, gtol = FWD_TOL[precision], GRAD_TOL[precision]
    assert_discriminates(f"{tag} {precision}", *disc, ftol, gtol)
    N = int(lengths.sum())
    grads, losses, worst = [], [], {"free_energy": 0.0, "loss": 0.0, "differ": 0}
    for i, g in enumerate(m.generators):
        fe = g.free_energy.cpu().numpy()
        vs = g._outputs.cpu().numpy()
        assert fe.shape == (N,) and vs.shape == (N, P)
        worst["differ"] = max(worst["differ"], chains_differing(vs, fws[i]['v_sample']))
        fd = on_chain_ends(fws[i], vs)
        cost, F = orbm.free_energy_cost(fd['tgt'], fd['v_sample'], ps[i]['W'], fd['bh_t'], fd['bv_t'])
        worst["free_energy"] = max(worst["free_energy"], TM.rel(fe, F))
        worst["loss"] = max(worst["loss"], abs(float(g.metrics["batch/loss"]) - cost.mean()) / max(1.0, abs(cost.mean())))
        losses.append(cost.mean())
        grads.append(G.rnn_rbm_backward(fd, ps[i]))
    e_mean = abs(float(m.generator_loss()) - np.mean(losses)) / max(1.0, abs(np.mean(losses)))
    _, _, metrics, _, _ = m.train_generators(AdamOptimizer(0.01), 0.01)
    m.check()
    e_mean = max(e_mean, abs(float(metrics["batch/loss"]) - np.mean(losses)) / max(1.0, abs(np.mean(losses))))
    gerr = 0.0
    for i, g in enumerate(m.generators):
        for name, ref in zip(g.store.names(), TM.rbm_grad_list(grads[i])):
            gerr = max(gerr, TM.rel(g.store.gviews[name].cpu().numpy().reshape(ref.shape), ref / M))
    print(f"\n[{tag} {precision}, {N} valid rows of {B * T}] free energy {worst['free_energy']:.2e}  loss {worst['loss']:.2e}  mean track loss {e_mean:.2e}  "
          f"rows whose Gibbs chain end differs from the float64 chain's {worst['differ']}  gradients {gerr:.2e}")
    assert worst["differ"] <= chain_cap(N), worst
    assert worst["free_energy"] < ftol and worst["loss"] < ftol and e_mean < ftol
    assert gerr < gtol


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_c3_jamming_ragged_real_widths(precision):
    """test_c3_jamming_real_widths on a RAGGED window (B = 32, T = 8, lengths 1 .. 8 with one full and one single-step sequence): per
    generator free energy, loss and Gibbs chains; for the mode the mean track loss and every gradient against ref / M."""
    B, T = 32, 8
    lengths = np.random.default_rng(3).integers(1, 9, B)
    lengths[0], lengths[1] = 8, 1
    _jamming_ragged_vs_oracle("B", precision, B, T, lengths, 8, grouped=False)


def test_c3_jamming_lockstep_ragged_vs_oracle():
    """The same on the form the C3 benchmark runs (`group_generators`, B = 256, the shortest lockstep window T = 4), lengths 0 .. 4."""
    B, T = 256, 4
    lengths = np.random.default_rng(3).integers(0, 5, B)
    lengths[0], lengths[1], lengths[2] = 4, 1, 0
    _jamming_ragged_vs_oracle("C lockstep", "fp16", B, T, lengths, 9, grouped=True)


# ------------------------------------------------------------------------------------------------------------------------
# D. the captured ragged step
def _replay_lengths(B, T):
    lens = [np.random.default_rng(4).integers(1, T + 1, B).astype(np.int32), np.full(B, T, np.int32), np.ones(B, np.int32)]
    lens[2][0] = 4
    return lens


def test_captured_ragged_jamming_rbm_step_vs_oracle():
    """MultINNCore.graphed_train_step(lengths=...) of a jamming mode with two LSTM-RBM generators at the reference's widths (fp16, keep_prob 1):
    three replays of ONE captured step on different length vectors (random, all full, all 1 but one of 4).  Before each replay every
    generator's f32 weights and device step counter are read back into float64 oracle parameters (the Gibbs seed is seed + step); after it
    the returned loss, each generator's `free_energy` -- read through the public property after EVERY replay, which indexes the kernels' rows
    by the lengths of that replay -- the Gibbs chains and the gradients left in store.gviews are compared with the oracle at those weights."""
    from multinn_amd import MultINN, AdamOptimizer
    B, T, Mt, k, precision = 16, 8, 2, 10, "fp16"
    ftol, gtol = FWD_TOL[precision], GRAD_TOL[precision]
    lens = _replay_lengths(B, T)
    xs = [loud_padding(TM.batch(B, T, P, Mt, 40 + i, rho=0.05), lens[i]) for i in range(3)]
    m = MultINN(TM.config(P, TM.TRACKS5[:Mt]), TM.params("jamming", gen="RBM", Hn=HN, units=UNITS, keep_prob=1.0), mode="jamming",
                precision=precision, seed=23)
    opt = AdamOptimizer(0.01)
    m.build(TM.dev(xs[0]), lengths=TM.dev(lens[0]), is_train=True, mode="train")
    for g, p in zip(m.generators, _c3_params()):
        TM.load_rbm_params(g, p)
    run = m.graphed_train_step(TM.dev(xs[0]), opt, warmup=1, lengths=TM.dev(lens[0]))
    assert run.ragged and all(g.ragged_on_device for g in m.generators)
    for r, (x, ln) in enumerate(zip(xs, lens)):
        N = int(ln.sum())
        ps = [read_rbm_params(g) for g in m.generators]
        steps = [int(g.store.step_dev) for g in m.generators]
        assert steps == [g.store.step for g in m.generators] == [r + 1] * Mt
        tracks = G.per_track_inputs(x)
        fws = [G.rnn_rbm_forward(tracks[i][:, :-1].astype(np.float64), tracks[i][:, 1:].astype(np.float64), ln, ps[i], k, g.seed + steps[i],
                                 row_ids=row_ids(ln)) for i, g in enumerate(m.generators)]
        if r == 0:
            inp, tgt = tracks[0][:, :-1].astype(np.float64), tracks[0][:, 1:].astype(np.float64)
            full = G.rnn_rbm_forward(inp, tgt, None, ps[0], k, m.generators[0].seed + steps[0], row_ids=full_rows(B, T))
            assert_discriminates("D", full['loss'], fws[0]['loss'], G.rnn_rbm_backward(full, ps[0])['W'], G.rnn_rbm_backward(fws[0], ps[0])['W'], ftol, gtol)
        loss = float(run(TM.dev(x), TM.dev(ln)))
        losses, e_fe, differ, gerr = [], 0.0, 0, 0.0
        for i, g in enumerate(m.generators):
            fe = g.free_energy.cpu().numpy()
            assert fe.shape == (N,), (r, i, fe.shape, N)
            vs = g._outputs.cpu().numpy()
            differ = max(differ, chains_differing(vs, fws[i]['v_sample']))
            fd = on_chain_ends(fws[i], vs)
            cost, F = orbm.free_energy_cost(fd['tgt'], fd['v_sample'], ps[i]['W'], fd['bh_t'], fd['bv_t'])
            e_fe = max(e_fe, TM.rel(fe, F))
            losses.append(cost.mean())
            for name, ref in zip(g.store.names(), TM.rbm_grad_list(G.rnn_rbm_backward(fd, ps[i]))):
                gerr = max(gerr, TM.rel(g.store.gviews[name].cpu().numpy().reshape(ref.shape), ref / Mt))
        e_loss = abs(loss - np.mean(losses)) / max(1.0, abs(np.mean(losses)))
        print(f"\n[D replay {r}, {N} valid rows of {B * T}] loss {e_loss:.2e}  free energy {e_fe:.2e}  rows whose chain end differs {differ}  gradients {gerr:.2e}")
        assert differ <= chain_cap(N)
        assert e_loss < ftol and e_fe < ftol and gerr < gtol
    m.check()


def test_captured_ragged_jamming_nade_step_log_probs_vs_oracle():
    """The same captured step with NADE generators (their rows are compacted on the device): `log_probs` read after each of two replays with
    different lengths, and the returned loss, against rnn_nade_forward(..., lengths) at the weights read back before the replay."""
    from multinn_amd import MultINN, AdamOptimizer
    B, T, Mt, precision = 16, 8, 2, "fp16"
    ftol = FWD_TOL[precision]
    lens = _replay_lengths(B, T)[::2]
    xs = [loud_padding(TM.batch(B, T, P, Mt, 50 + i, rho=0.05), lens[i]) for i in range(2)]
    m = MultINN(TM.config(P, TM.TRACKS5[:Mt]), TM.params("jamming", gen="NADE", Hn=HN, units=UNITS, keep_prob=1.0), mode="jamming",
                precision=precision, seed=23)
    opt = AdamOptimizer(0.01)
    m.build(TM.dev(xs[0]), lengths=TM.dev(lens[0]), is_train=True, mode="train")
    for i, g in enumerate(m.generators):
        p = G.init_rnn_nade(60 + i, P, P, HN, UNITS, np.float64)
        p['fc_b'][HN:] = np.log(0.05 / 0.95)
        TM.load_nade_params(g, p)
    run = m.graphed_train_step(TM.dev(xs[0]), opt, warmup=1, lengths=TM.dev(lens[0]))
    assert run.ragged
    for r, (x, ln) in enumerate(zip(xs, lens)):
        N = int(ln.sum())
        ps = [read_nade_params(g) for g in m.generators]
        tracks = G.per_track_inputs(x)
        fws = [G.rnn_nade_forward(tracks[i][:, :-1].astype(np.float64), tracks[i][:, 1:].astype(np.float64), ln, ps[i]) for i in range(Mt)]
        loss = float(run(TM.dev(x), TM.dev(ln)))
        e_nll = 0.0
        for i, g in enumerate(m.generators):
            assert g._ctx["compact"] is not None
            lp = g.log_probs.cpu().numpy()
            assert lp.shape == (N,), (r, i, lp.shape, N)
            e_nll = max(e_nll, TM.rel(lp, fws[i]['nll'][0]))
        ref = np.mean([f['loss'] for f in fws])
        e_loss = abs(loss - ref) / abs(ref)
        print(f"\n[D NADE replay {r}, {N} valid rows of {B * T}] loss {e_loss:.2e}  per-row NLL {e_nll:.2e}")
        assert e_loss < ftol and e_nll < ftol
    m.check()


def test_captured_ragged_rnn_nade_step_log_probs_vs_oracle():
    """RnnNade.graphed_train_step(lengths=...) -- the joint mode's captured piano-roll step keeps its own static lengths -- in the same way:
    `log_probs` and the loss of two replays with different lengths against the oracle at the weights read back before each."""
    from multinn_amd import RnnNade, AdamOptimizer
    B, T, Pp, Mt, Hn, units, precision = 16, 8, 8, 2, 256, [128, 128], "fp16"
    D, ftol = Pp * Mt, FWD_TOL[precision]
    lens = _replay_lengths(B, T)[::2]
    xs = [loud_padding(TM.batch(B, T, Pp, Mt, 60 + i, rho=0.1), lens[i]) for i in range(2)]
    gen = RnnNade(D, Hn, units, keep_prob=1.0, precision=precision, seed=23)
    gen._materialize(D)
    p = G.init_rnn_nade(3, D, D, Hn, units, np.float64)
    p['fc_b'][Hn:] = np.log(0.1 / 0.9)
    TM.load_nade_params(gen, p)
    run = gen.graphed_train_step(TM.dev(xs[0]), AdamOptimizer(0.01), warmup=1, lengths=TM.dev(lens[0]))
    assert run.ragged
    for r, (x, ln) in enumerate(zip(xs, lens)):
        N = int(ln.sum())
        inp, tgt = G.joint_inputs(x.astype(np.float64))
        fw = G.rnn_nade_forward(inp, tgt, ln, read_nade_params(gen))
        loss = float(run(TM.dev(x), TM.dev(ln)))
        lp = gen.log_probs.cpu().numpy()
        assert lp.shape == (N,), (r, lp.shape, N)
        e_loss, e_nll = abs(loss - fw['loss']) / abs(fw['loss']), TM.rel(lp, fw['nll'][0])
        print(f"\n[D RnnNade replay {r}, {N} valid rows of {B * T}] loss {e_loss:.2e}  per-row NLL {e_nll:.2e}")
        assert e_loss < ftol and e_nll < ftol
    gen.check()


# ------------------------------------------------------------------------------------------------------------------------
# E. RnnMultiNADE generator
@functools.lru_cache(maxsize=1)
def _multinade_oracle():
    B, T, E, Mt, Hn, units, seed = 6, 5, 6, 3, 12, [32, 32], 11
    lengths = np.array([5, 2, 4, 5, 1, 3], np.int32)
    enc = (np.random.default_rng(4).random((B, T + 1, E * Mt)) < .1).astype(np.uint8)      # stacked per-track codes, track-minor
    enc[:, 0] = 0
    for b in range(B):
        enc[b, lengths[b] + 1:] = 1                     # the steps behind a sequence's end are loud: they must not reach loss or gradients
    inp, tgt = enc[:, :-1], enc[:, 1:]
    p = G.init_rnn_nade(7, E * Mt, E, Hn, units, np.float64, tracks=Mt)
    p['fc_b'][Mt * Hn:] = np.log(0.1 / 0.9)
    du = G.dropout_uniforms(seed, B, T, units)
    fw = G.rnn_nade_forward(inp.astype(np.float64), tgt.astype(np.float64), lengths, p, 0.9, du, tracks=Mt)
    g = G.rnn_nade_backward(fw, p, tracks=Mt)
    full = G.rnn_nade_forward(inp.astype(np.float64), tgt.astype(np.float64), None, p, 0.9, du, tracks=Mt)
    g_full = G.rnn_nade_backward(full, p, tracks=Mt)
    return (B, T, E, Mt, Hn, units, seed), lengths, inp, tgt, p, fw, g, (full['loss'], fw['loss'], np.stack(g_full['w_dec']), np.stack(g['w_dec']))


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_rnn_multinade_ragged_train_step_vs_oracle(precision):
    """RnnMultiNADE (the composer mode's generator) on a ragged window: fp32 keeps the padding rows (weight 0), bf16 / fp16 run Dense + NADE
    on the compacted valid rows.  Loss, per-track API-order `log_probs[m]` and every gradient against rnn_nade_forward / backward(...,
    lengths, tracks=M).  16-bit bounds: those of test_rnn_nade_joint_train_step (fp16, with three more operand bits, is held to bf16's)."""
    from multinn_amd import RnnMultiNADE
    (B, T, E, Mt, Hn, units, seed), lengths, inp, tgt, p, fw, g, disc = _multinade_oracle()
    tol = 1e-4 if precision == "fp32" else 6e-2
    gtol = tol if precision == "fp32" else 2 * tol
    assert_discriminates(f"E {precision}", *disc, tol, gtol, unit_floor=False)
    gen = RnnMultiNADE(E, Hn, units, tracks=[f"t{m}" for m in range(Mt)], keep_prob=0.9, precision=precision, seed=seed)
    gen.build(TM.dev(inp), TM.dev(tgt), TM.dev(lengths), True, "train")
    TM.load_nade_params(gen, p)
    gen.build(TM.dev(inp), TM.dev(tgt), TM.dev(lengths), True, "train")
    assert (gen._ctx["compact"] is not None) == (precision != "fp32")
    N = int(lengths.sum())
    e_loss = abs(float(gen.metrics['batch/loss']) - fw['loss']) / abs(fw['loss'])
    lps = [t.cpu().numpy() for t in gen.log_probs]
    assert len(lps) == Mt and all(lp.shape == (N,) for lp in lps)
    e_nll = max(TM.rel(lps[m], fw['nll'][m]) for m in range(Mt))
    gen.backward()
    gen.check()
    ref_g = [a for pair in g['lstm'] for a in pair] + [np.stack(g['w_enc']), np.stack(g['w_dec']), g['fc_k'], g['fc_b']]
    gerr = {name: TM.rel(gen.store.gviews[name].cpu().numpy().reshape(ref.shape), ref) for name, ref in zip(gen.store.names(), ref_g)}
    print(f"\n[E {precision}] loss {e_loss:.2e}  per-row NLL {e_nll:.2e}  gradients {max(gerr.values()):.2e}")
    assert len(gerr) == len(gen.store.names()) == len(ref_g)
    assert e_loss < tol and e_nll < tol
    assert all(v < gtol for v in gerr.values()), gerr
