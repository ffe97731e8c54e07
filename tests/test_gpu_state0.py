"""Initial LSTM state on the CU-resident and cluster recurrences, and the learned initial state (`learn_zero_state`, rnn.py:139-143, 166-172)
built on it: kernels against a float64 restatement on the same 16-bit operands (the style and bounds of
test_gpu_kernels.py::test_lstm_resident_recurrence_vs_float64 / ::test_lstm_cluster_recurrence_vs_float64), the stack and the generators
against the float64 oracle (oracle.lstm.seq_fwd(init_state=...) / seq_bwd composed with oracle.nade / oracle.rbm here; state gradients from
a float64 autograd composition of oracle.torch_ref.lstm_cell)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import generators as G, lstm as olstm, nade as onade, torch_ref   # noqa: E402
from oracle.tf_semantics import dense   # noqa: E402

DEV = "cuda:0"
P, M, HN, UNITS = 88, 5, 256, [512, 256]
D = P * M


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / max(1e-300, np.linalg.norm(a) * np.linalg.norm(b)))


def _gate_perm(u):
    """natural TF column g * u + unit -> (unit / 32) * 128 + g * 32 + unit % 32 (DESIGN.md "LSTM layout")"""
    unit = np.arange(u)
    return np.stack([(unit >> 5) * 128 + g * 32 + (unit & 31) for g in range(4)])        # [gate][unit]


# ------------------------------------------------------------------------------------------------ kernels
def _job(u, B, T, keep, tdt, seed, state):
    """Seeded inputs of one layer (host tensors): state = 'random' | 'zeros' | None."""
    rng = np.random.default_rng(seed)
    r16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt)            # noqa: E731
    j = dict(wh_t=r16(rng.normal(0, 0.06 if u == 256 else 0.04, (4 * u, u))), xproj=r16(rng.normal(0, 1.2, (T, B, u, 4))),
             mask=(rng.random((T, B, u)) < keep).astype(np.uint8) if keep < 1.0 else None,
             dh=torch.from_numpy(rng.normal(0, 0.02, (T, B, u)).astype(np.float32)), h0=None, c0=None)
    if state == "random":
        j["h0"], j["c0"] = r16(rng.normal(0, 0.5, (B, u))), torch.from_numpy(rng.normal(0, 0.5, (B, u)).astype(np.float32))
    elif state == "zeros":
        j["h0"], j["c0"] = torch.zeros((B, u), dtype=tdt), torch.zeros((B, u))
    return j


SENTINEL = 0.375          # what column block 0 of h^T holds before the launch: the caller's h0^T, which the launch must leave alone


def _launch(ops, kind, j, B, T, keep, tdt, kb, want_dc0=True):
    """Forward + backward of one layer on the device; returns every output."""
    u = j["wh_t"].shape[1]
    N = T * B
    d = lambda t_: None if t_ is None else t_.to(DEV)                               # noqa: E731
    o = dict(gates=torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt), c=torch.zeros((T, B, u), device=DEV), h=torch.zeros((T, B, u), device=DEV, dtype=tdt),
             y=torch.zeros((T, B, u), device=DEV, dtype=tdt) if keep < 1.0 else None, hT=torch.full((u, N), SENTINEL, device=DEV, dtype=tdt),
             yT=torch.zeros((u, N), device=DEV, dtype=tdt), dzc=torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt),
             dzT=torch.zeros((N // 32, 4 * u, 32), device=DEV, dtype=tdt) if kb else torch.zeros((4 * u, N), device=DEV, dtype=tdt),
             db=torch.zeros(4 * u, device=DEV), dc0=torch.full((B, u), 7.0, device=DEV) if (want_dc0 and j["c0"] is not None) else None,
             ws=ops.lstm_rowpar_workspace(T, B, u, DEV) if kind == "cluster" else None)
    # (the descriptors hold raw pointers: every device tensor they name stays alive in `o`)
    md = o["mask_d"] = d(torch.from_numpy(j["mask"])) if j["mask"] is not None else None
    o["xproj_d"], o["wh_t_d"], o["h0_d"], o["c0_d"], o["dh_d"] = d(j["xproj"]).view(T, B, 4 * u), d(j["wh_t"]), d(j["h0"]), d(j["c0"]), d(j["dh"])
    o["L"] = ops.lstm2_fwd_layer(o["xproj_d"], o["wh_t_d"], o["h0_d"], o["c0_d"], o["gates"], o["c"], o["h"], o["hT"], o["y"], md,
                                 yT=o["yT"], gates_dtype=tdt, xproj_dtype=tdt)
    o["wh_p"] = j["wh_t"].t().contiguous().to(DEV)
    o["bws"] = ops.lstm_seq_bwd_workspace(B, u, DEV)
    o["E"] = ops.lstm2_bwd_layer(o["dh_d"], o["wh_p"], o["gates"], o["c"], o["c0_d"], o["dzc"], o["bws"], o["dzT"], o["db"], md, gates_dtype=tdt)
    return o


def _run_single(ops, kind, o, B, T, keep):
    if kind == "resident":
        ops.lstm_resident_fwd(T, B, o["L"], keep)
        ops.lstm_resident_bwd(T, B, o["E"], keep, o["dc0"])
    else:
        ops.lstm_cluster_fwd(T, B, o["L"], keep, o["ws"])
        torch.cuda.synchronize()
        ops.lstm_rowpar_check(o["ws"])
        ops.lstm_cluster_bwd(T, B, o["E"], keep, o["ws"], o["dc0"])
    torch.cuda.synchronize()
    if o["ws"] is not None:
        ops.lstm_rowpar_check(o["ws"])


def _check_vs_float64(ops, j, o, B, T, keep, tdt, eps, kb):
    """The float64 restatement of rnn.py:104-145 on the same 16-bit operands, started from (c0, h0)."""
    u = j["wh_t"].shape[1]
    N = T * B
    r16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt)            # noqa: E731
    perm = _gate_perm(u)
    W = j["wh_t"].double().numpy()                                                   # z[n] += sum_k h[k] W[n][k]
    X = j["xproj"].double().numpy()
    mask = j["mask"]
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))                                        # noqa: E731
    h, c, y, gates = o["h"], o["c"], o["y"], o["gates"]
    hp, cp = j["h0"].double().numpy(), j["c0"].double().numpy()
    ref = dict(g=np.zeros((T, B, u, 4)), c=np.zeros((T, B, u)), h=np.zeros((T, B, u)))
    for t in range(T):
        z = np.stack([X[t, :, :, g] + hp @ W[perm[g]].T for g in range(4)], -1)     # [B, u, 4]
        gi, gg, gf, go = sig(z[..., 0]), np.tanh(z[..., 1]), sig(z[..., 2]), sig(z[..., 3])
        cp = gg * gi + cp * gf
        hv = np.tanh(cp) * go
        ref["g"][t], ref["c"][t], ref["h"][t] = np.stack([gi, gg, gf, go], -1), cp, hv
        hp = h[t].double().cpu().numpy() if (mask is None or t + 1 == T) else r16(hv).double().numpy()     # the 16-bit state the kernel feeds back
    got_c = c.cpu().numpy()
    assert np.abs(got_c - ref["c"]).max() < 4 * eps, np.abs(got_c - ref["c"]).max()
    if mask is None:
        assert np.abs(h.double().cpu().numpy() - ref["h"]).max() < 2 * eps
        out16 = h
    else:
        assert np.abs(h[-1].double().cpu().numpy() - ref["h"][-1]).max() < 2 * eps          # only the final state leaves through h
        yref = r16(ref["h"]).double().numpy() / keep * mask
        assert np.abs(y.double().cpu().numpy() - yref).max() < 3 * eps
        out16 = y
    assert np.abs(gates.double().cpu().numpy().reshape(T, B, u, 4) - ref["g"]).max() < 2 * eps
    hT, yT = o["hT"], o["yT"]
    assert torch.equal(yT.view(u, T, B), out16.permute(2, 0, 1))
    hh = r16(ref["h"]).double().numpy()
    assert np.abs(hT.view(u, T, B)[:, 1:].double().cpu().numpy() - np.transpose(hh, (2, 0, 1))[:, :-1]).max() < 2 * eps
    assert bool((hT.view(u, T, B)[:, 0] == SENTINEL).all()), "column block 0 of h^T is the caller's (h0^T)"
    # ---- backward on the kernel's own saved tensors ----
    dzc, dzT, db, dh = o["dzc"], o["dzT"], o["db"], j["dh"]
    Gs = gates.double().cpu().numpy().reshape(T, B, u, 4)
    Cs = c.double().cpu().numpy()
    dz_ref = np.zeros((T, B, 4 * u))
    dcv, dz_next = np.zeros((B, u)), np.zeros((B, 4 * u))
    for t in range(T - 1, -1, -1):
        gi, gg, gf, go = (Gs[t, :, :, k] for k in range(4))
        dhv = dh[t].double().numpy() * (mask[t] / keep if mask is not None else 1.0) + dz_next @ W      # sum_n dz[n] W[n][k]
        tc = np.tanh(Cs[t])
        d_o = dhv * tc
        d_c = dhv * go * (1 - tc * tc) + dcv
        cprev = Cs[t - 1] if t > 0 else j["c0"].double().numpy()
        dzs = [d_c * gg * gi * (1 - gi), d_c * gi * (1 - gg * gg), d_c * cprev * gf * (1 - gf), d_o * go * (1 - go)]
        dcv = d_c * gf
        for g in range(4):
            dz_ref[t][:, perm[g]] = dzs[g]
        dz_next = dzc[t].double().cpu().numpy()                                      # the 16-bit values the kernel feeds back
    scale = np.abs(dz_ref).max()
    got = dzc.double().cpu().numpy()
    assert np.abs(got - dz_ref).max() < 3 * eps * scale, (np.abs(got - dz_ref).max(), scale)
    flat = dzc.view(N, 4 * u)
    if kb:
        assert torch.equal(dzT.permute(0, 2, 1).reshape(N, 4 * u), flat)
    else:
        assert torch.equal(dzT[:, :N].t(), flat)
    db_ref = flat.double().sum(0).cpu().numpy()
    assert np.abs(db.cpu().numpy() - db_ref).max() < 1e-5 * max(1.0, np.abs(db_ref).max()) + 1e-6
    # ---- the state gradients: dc0 = d_c . f of step 0 (out of the launch); dh0 = dz[0] . Wh^T through the op the stack uses (one GEMM over
    # the kernel's own 16-bit dz[0]) ----
    e_c = np.abs(o["dc0"].double().cpu().numpy() - dcv).max()
    print(f"    dc0 err {e_c:.3e} (bound {3 * eps * np.abs(dcv).max():.3e})")
    assert e_c < 3 * eps * np.abs(dcv).max(), (e_c, np.abs(dcv).max())
    dh0 = ops.gemm_tn(dzc[0], o["wh_p"], torch.empty((B, u), device=DEV))
    dh0_ref = dzc[0].double().cpu().numpy() @ W
    e_h = np.abs(dh0.double().cpu().numpy() - dh0_ref).max()
    print(f"    dh0 err {e_h:.3e} (bound {3 * eps * np.abs(dh0_ref).max():.3e})")
    assert e_h < 3 * eps * np.abs(dh0_ref).max(), (e_h, np.abs(dh0_ref).max())


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("B,T,keep", [(8, 6, 0.9), (64, 5, 1.0), (2048, 2, 0.9)])
def test_lstm_resident_recurrence_with_initial_state_vs_float64(ops, B, T, keep, dt):
    """mnn_lstm_resident_fwd with L->h0 / L->c0 and mnn_lstm_resident_bwd_state (c0 in, dc0 out): h0 = r16(N(0, 0.5)), c0 = N(0, 0.5)."""
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    eps = 2.0 ** -10 if dt == "fp16" else 2.0 ** -7
    kb = B % 32 == 0
    j = _job(256, B, T, keep, tdt, 11, "random")
    o = _launch(ops, "resident", j, B, T, keep, tdt, kb)
    _run_single(ops, "resident", o, B, T, keep)
    _check_vs_float64(ops, j, o, B, T, keep, tdt, eps, kb)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("T,nolocal", [(4, False), (6, False), (4, True), (6, True)])
def test_lstm_cluster_recurrence_with_initial_state_vs_float64(ops, monkeypatch, T, nolocal, dt):
    """mnn_lstm_cluster_fwd with L->h0 / L->c0 and mnn_lstm_cluster_bwd_state, B = 256 (eight clusters), both hand-off policies of the
    forward (MNN_PERSIST_NO_LOCAL as test_lstm_cluster_recurrence_vs_float64 switches it); the status word is read after every launch."""
    if nolocal:
        monkeypatch.setenv("MNN_PERSIST_NO_LOCAL", "1")
    B, keep = 256, 0.9
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    eps = 2.0 ** -10 if dt == "fp16" else 2.0 ** -7
    j = _job(512, B, T, keep, tdt, 13, "random")
    o = _launch(ops, "cluster", j, B, T, keep, tdt, True)
    _run_single(ops, "cluster", o, B, T, keep)
    _check_vs_float64(ops, j, o, B, T, keep, tdt, eps, True)


@pytest.mark.parametrize("kind,B,T,keep", [("resident", 64, 5, 0.9), ("resident", 8, 3, 1.0), ("cluster", 256, 5, 0.9), ("cluster", 256, 4, 1.0)])
def test_all_zero_initial_state_is_bit_identical_to_the_null_launch(ops, kind, B, T, keep):
    """All-zero h0 / c0 arrays take the state path of the kernels and must give the bits of the NULL launch: forward h, c, gates, hT, yT (and
    y), backward dz (both layouts) and db."""
    tdt = torch.float16
    u = 256 if kind == "resident" else 512
    kb = B % 32 == 0
    outs = []
    for state in (None, "zeros"):
        j = _job(u, B, T, keep, tdt, 5, state)
        o = _launch(ops, kind, j, B, T, keep, tdt, kb)
        _run_single(ops, kind, o, B, T, keep)
        outs.append(o)
    a, b = outs
    for k in ("h", "c", "gates", "hT", "yT", "y", "dzc", "dzT", "db"):
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k
    assert float(a["dzc"].float().abs().max()) > 0 and float(b["dc0"].abs().max()) > 0 and bool((b["dc0"] != 7.0).all())


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kind,B,T,keep", [("resident", 64, 5, 0.9), ("cluster", 256, 6, 0.9)])
def test_multi_job_launch_with_different_states_equals_single_launches(ops, kind, B, T, keep, mixed):
    """Three jobs with three different initial states in ONE launch of the _multi / _state_multi entries equal three single launches bit for
    bit, dc0 included.  mixed: the third job has no state (the header allows jobs with and without one in a launch: the test is per workgroup)."""
    tdt = torch.float16
    u = 256 if kind == "resident" else 512
    jobs = [_job(u, B, T, keep, tdt, 20 + i, "random" if (i < 2 or not mixed) else None) for i in range(3)]
    if kind == "cluster":       # 3 x 8 clusters: a multiple of 8
        assert ops.lstm_cluster_bwd_multi_ok(B, u, 3)
    single = [_launch(ops, kind, j, B, T, keep, tdt, True) for j in jobs]
    multi = [_launch(ops, kind, j, B, T, keep, tdt, True) for j in jobs]
    for o in single:
        _run_single(ops, kind, o, B, T, keep)
    wss = [o["ws"] for o in multi] if kind == "cluster" else None
    ops.lstm_recurrence_multi(kind + "_fwd", T, B, [o["L"] for o in multi], keep, wss)
    torch.cuda.synchronize()
    for o in multi:
        if o["ws"] is not None:
            ops.lstm_rowpar_check(o["ws"])
    ops.lstm_recurrence_multi(kind + "_bwd", T, B, [o["E"] for o in multi], keep, wss, [o["dc0"] for o in multi])
    torch.cuda.synchronize()
    for o in multi:
        if o["ws"] is not None:
            ops.lstm_rowpar_check(o["ws"])
    for a, b in zip(single, multi):
        for k in ("gates", "c", "h", "y", "hT", "yT", "dzc", "dzT", "db", "dc0"):
            if a[k] is not None:
                assert torch.equal(a[k], b[k]), k
    assert not torch.equal(single[0]["dc0"], single[1]["dc0"])
    if mixed:
        assert single[2]["dc0"] is None
    else:
        assert not torch.equal(single[1]["dc0"], single[2]["dc0"]) and not torch.equal(single[0]["dc0"], single[2]["dc0"])


# ------------------------------------------------------------------------------------------------ stack and models
def synth(B, T, seed, rho):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.random((B, T, P, M)) < rho).astype(np.uint8)


def load(gen, p, c0):
    s = gen.store
    for l, (W, b) in enumerate(p['lstm']):
        s[f"rnn/cell_{l}/kernel"].copy_(dev(W.astype(np.float32))); s[f"rnn/cell_{l}/bias"].copy_(dev(b.astype(np.float32)))
        s[f"rnn/cell_{l}/c0"].copy_(dev(c0[l].astype(np.float32)))
    s["nade/w_enc"].copy_(dev(np.stack(p['w_enc']).astype(np.float32)))
    s["nade/w_dec"].copy_(dev(np.stack(p['w_dec']).astype(np.float32)))
    s["dense/kernel"].copy_(dev(p['fc_k'].astype(np.float32)))
    s["dense/bias"].copy_(dev(p['fc_b'].astype(np.float32)))
    gen._packed_step = -1


def state_of(c0, B):
    """zero_state of rnn.py:166-172 in float64: [(c0 tiled, tanh(c0) tiled)]."""
    return [(np.tile(c, (B, 1)), np.tile(np.tanh(c), (B, 1))) for c in c0]


def state_grads(cache, dy, c0):
    """float64 autograd composition of oracle.torch_ref.lstm_cell over the oracle forward's inputs and keep masks: the gradient of
    sum(y * dy) wrt the per-row initial state [(dc0, dh0) [B, u]] per layer, and wrt the c0 variables [1, u] (through h0 = tanh(c0))."""
    x = torch.from_numpy(np.asarray(cache['x'], np.float64))
    B, T, _ = x.shape
    kp = cache['keep_prob']
    layers = [(torch.from_numpy(W), torch.from_numpy(b)) for W, b in cache['layers']]
    cv = [torch.from_numpy(np.asarray(c, np.float64)).clone().requires_grad_(True) for c in c0]
    st = []
    for c in cv:
        cb, hb = c.expand(B, -1).clone(), torch.tanh(c).expand(B, -1).clone()
        cb.retain_grad(); hb.retain_grad()
        st.append((cb, hb))
    leaves = list(st)
    ys = []
    for t in range(T):
        inp = x[:, t]
        for l, (W, b) in enumerate(layers):
            c_, h_ = st[l]
            h2, c2 = torch_ref.lstm_cell(inp, c_, h_, W, b)
            st[l] = (c2, h2)
            inp = h2 / kp * torch.from_numpy(np.asarray(cache['keep'][l][t], np.float64)) if kp < 1.0 else h2
        ys.append(inp)
    (torch.stack(ys, 1) * torch.from_numpy(dy)).sum().backward()
    return [(cb.grad.numpy(), hb.grad.numpy()) for cb, hb in leaves], [c.grad.numpy() for c in cv]


def nade_oracle(x, p, c0, keep_prob, lengths=None):
    """oracle.generators.rnn_nade_forward / _backward restated with an initial state (those two take none), joint piano-roll plumbing."""
    inp, tgt = G.joint_inputs(x.astype(np.float64))
    return nade_oracle_xy(inp, tgt, p, c0, keep_prob, lengths)


def nade_oracle_xy(inp, tgt, p, c0, keep_prob, lengths=None, tracks=1, seed=23, units=UNITS):
    """Forward dict, gradients (the LSTM's from oracle.lstm.seq_bwd, whose xh.T @ dz holds the h0 term), the c0 gradients and the per-row
    state gradients of an LSTM-(Multi)NADE started from zero_state(c0)."""
    B, T = inp.shape[0], inp.shape[1]
    Hn, Dd = p['w_enc'][0].shape[1], p['w_enc'][0].shape[0]
    y, _, cache = olstm.seq_fwd(inp, p['lstm'], keep_prob, G.dropout_uniforms(seed, B, T, units), lengths, 'decode', init_state=state_of(c0, B))
    valid = np.ones((B, T), bool) if lengths is None else (np.arange(T)[None, :] < np.asarray(lengths)[:, None])
    yf, tf_ = y[valid], tgt[valid]
    out = dense(yf, p['fc_k'], p['fc_b'])
    b_enc, b_dec = G.split_biases(out, Hn, Dd, tracks)
    tg = [tf_] if tracks == 1 else [tf_.reshape(-1, Dd, tracks)[..., m] for m in range(tracks)]
    rw = G.row_weights(lengths, B, T, np.float64) / tracks
    assert rw.shape[0] == yf.shape[0]
    nll, cond, g = [], [], dict(w_enc=[], w_dec=[])
    d_out = np.zeros((yf.shape[0], p['fc_k'].shape[1]))
    for m in range(tracks):
        n_, c_ = onade.log_prob(tg[m], b_enc[m], b_dec[m], p['w_enc'][m], p['w_dec'][m])
        nll.append(n_); cond.append(c_)
        dbe, dbd, dwe, dwd = onade.log_prob_bwd(tg[m], b_enc[m], b_dec[m], p['w_enc'][m], p['w_dec'][m], rw)
        d_out[:, m * Hn:(m + 1) * Hn] = dbe
        d_out[:, tracks * Hn + m * Dd:tracks * Hn + (m + 1) * Dd] = dbd
        g['w_enc'].append(dwe); g['w_dec'].append(dwd)
    g['fc_k'], g['fc_b'] = yf.T @ d_out, d_out.sum(0)
    dy = np.zeros((B, T, yf.shape[1]))
    dy[valid] = d_out @ p['fc_k'].T
    _, g['lstm'] = olstm.seq_bwd(dy, cache)
    rows, g['c0'] = state_grads(cache, dy, c0)
    fw = dict(loss=float(np.mean([n_.mean() for n_ in nll])), nll=nll[0] if tracks == 1 else nll, cond_p=cond[0] if tracks == 1 else cond, valid=valid)
    return fw, g, rows, dy


def oracle_grads(g):
    out = []
    for W, b in g['lstm']:
        out += [W, b]
    return out + list(g['c0']) + [np.stack(g['w_enc']), np.stack(g['w_dec']), g['fc_k'], g['fc_b']]


def params(seed, rho, c0_std=0.3):
    p = G.init_rnn_nade(seed, D, D, HN, UNITS, np.float64)
    for W, b in p['lstm']:
        b += 0.05
    p['fc_b'][HN:] += np.log(rho / (1 - rho))
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    return p, [rng.normal(0, c0_std, (1, u)) for u in UNITS]


class Calls:
    """Counts the recurrence launches that go through multinn_amd.ops."""
    NAMES = ("lstm_resident_fwd", "lstm_resident_bwd", "lstm_cluster_fwd", "lstm_cluster_bwd", "lstm_rowpar_fwd", "lstm_rowpar_bwd", "lstm_seq_fwd",
             "lstm_seq_bwd", "lstm2_persist_fwd", "lstm2_persist_bwd", "lstm_recurrence_multi")

    def __init__(self, monkeypatch):
        from multinn_amd import ops as o
        self.n = {k: 0 for k in self.NAMES}
        self.kinds = []
        for k in self.NAMES:
            monkeypatch.setattr(o, k, self._wrap(k, getattr(o, k)))

    def _wrap(self, k, fn):
        def f(*a, **kw):
            self.n[k] += 1
            if k == "lstm_recurrence_multi":
                self.kinds.append(a[0])
            return fn(*a, **kw)
        return f


def _compare(gen, fw, g, title):
    loss = float(gen.metrics["batch/loss"])
    nll = gen.log_probs.cpu().numpy()
    cp_err = np.abs(gen.cond_probs.cpu().numpy() - fw['cond_p']).max()
    gen.backward()
    gen._stack.check()
    errs = {"loss": abs(loss - fw['loss']) / abs(fw['loss'])}
    if fw.get("api_nll") is not None:
        errs["nll"] = rel(nll, fw["api_nll"])
    cosv = {}
    names = gen.store.names()
    assert names[4:6] == ["rnn/cell_0/c0", "rnn/cell_1/c0"]
    for name, ref in zip(names, oracle_grads(g)):
        got = gen.store.gviews[name].cpu().numpy().reshape(ref.shape)
        errs[name] = rel(got, ref)
        cosv[name] = cosine(got, ref)
    print(f"\n[{title}] relative error vs float64 oracle:")
    for k, v in errs.items():
        print(f"    {k:24s} {v:.3e}" + (f"   cos {cosv[k]:.6f}" if k in cosv else ""))
    print(f"    {'cond_probs (abs)':24s} {cp_err:.3e}")
    return errs, cosv, cp_err


def test_timed_cluster_kernels_with_learned_state_vs_oracle(monkeypatch):
    """The stateful twin of test_gpu_realdims.py::test_timed_cluster_kernels_long_sequence_vs_oracle: the flag-on model on the cluster
    (layer 1) and CU-resident (layer 2) kernels, forward and backward, c0 ~ N(0, 0.3) so that h0 != 0 and the tanh' factor is exercised;
    that test's bounds, the two c0 gradients included (held like rnn/cell_l/bias: a column sum over the batch from the same backward)."""
    from multinn_amd import RnnNade
    B, T, rho = 256, 8, 0.03
    x = synth(B, T, 37, rho)
    p, c0 = params(41, rho)
    fw, g, _, _ = nade_oracle(x, p, c0, 0.9)
    fw["api_nll"] = fw["nll"]
    gen = RnnNade(D, HN, UNITS, keep_prob=0.9, precision="fp16", seed=23, learn_zero_state=True)
    gen._materialize(D)
    load(gen, p, c0)
    gen._stack.rowpar_min_batch = 32
    calls = Calls(monkeypatch)
    gen.build_pianoroll(dev(x), None, is_train=True, mode="train")
    assert gen._stack._rowpar_state0(B, T) and gen._ctx["lstm"][0].get("rowpar") and gen._nade_mfma() and gen._nade_exact()
    assert gen._stack._cluster(0, B, T) and gen._stack._cluster_bwd(0, B, T) and gen._stack._resident(1, B, T) and not gen._stack._resident(0, B, T)
    assert gen._ctx["lstm"][0]["c0"] is not None and gen._ctx["lstm"][1]["h0"] is not None
    errs, cosv, cp_err = _compare(gen, fw, g, f"learned state, cluster kernels fp16 B={B} T={T} rho={rho}")
    assert calls.n["lstm_cluster_fwd"] == 1 and calls.n["lstm_resident_fwd"] == 1 and calls.n["lstm_cluster_bwd"] == 1 and calls.n["lstm_resident_bwd"] == 1
    assert calls.n["lstm_seq_fwd"] == calls.n["lstm_seq_bwd"] == calls.n["lstm_rowpar_fwd"] == calls.n["lstm_rowpar_bwd"] == calls.n["lstm2_persist_fwd"] == 0
    assert errs["loss"] < 1e-4 and errs["nll"] < 1e-4 and cp_err < 1e-4, (errs, cp_err)
    assert all(v < 3e-3 for v in errs.values()), errs
    assert all(c > 0.99999 for c in cosv.values()), cosv


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_stack_state_gradients_vs_autograd(precision):
    """LstmStack.backward(need_dstate=True) at the same shape: the per-row dc0, dh0 of both layers against the float64 autograd values,
    below the gradient bound test_joint_lstm_nade_step_at_real_widths_vs_oracle uses for the precision."""
    from multinn_amd import RnnNade
    B, T, rho = 256, 8, 0.03
    x = synth(B, T, 37, rho)
    p, c0 = params(41, rho)
    _, _, rows, dy = nade_oracle(x, p, c0, 0.9)
    gen = RnnNade(D, HN, UNITS, keep_prob=0.9, precision=precision, seed=23, learn_zero_state=True)
    gen._materialize(D)
    load(gen, p, c0)
    gen._stack.rowpar_min_batch = 32
    gen._ensure_packed()
    gen._rnn.build_cell(True)
    stack = gen._stack
    inp, _ = G.joint_inputs(x.astype(np.float64))
    x_tm = gen._to_time_major_inputs(dev(inp.astype(np.float32)))
    assert stack._rowpar_state0(B, T)
    gen.store.grad.zero_()
    y, ctx, _ = stack.forward(x_tm, 0.9, gen.seed, 0, save=True, state0=gen._state0(B), step_dev=gen.store.step_dev, state_grad=True)
    assert ctx[0].get("rowpar")
    scale = 4096.0 if precision == "fp16" else 1.0          # (a power of two: the f16 backward works on a scaled seed, as the generators do)
    dyd = dev((np.transpose(dy, (1, 0, 2)) * scale).astype(np.float32)).contiguous()
    _, dstate = stack.backward(dyd, ctx, 0.9, gen.seed, 0, step_dev=gen.store.step_dev, need_dstate=True)
    torch.cuda.synchronize()
    stack.check()
    bound = 3e-3 if precision == "fp16" else 2e-2
    for l, ((dc0, dh0), (rc, rh)) in enumerate(zip(dstate, rows)):
        ec, eh = rel(dc0.cpu().numpy() / scale, rc), rel(dh0.cpu().numpy() / scale, rh)
        print(f"    [{precision}] layer {l}: dc0 rel {ec:.3e}  dh0 rel {eh:.3e}")
        assert ec < bound and eh < bound, (l, ec, eh)


def test_launch_per_timestep_path_fp32_vs_oracle_and_optimiser_step():
    """The same model at precision fp32, B = 16, T = 5 (no resident / cluster form: mnn_lstm_seq_fwd / _bwd with h0 / c0 in and dh0 / dc0
    out): everything within 1e-4, and one train_step moves both c0 by what clip 5.0 + TF-Adam give for the oracle's gradient."""
    from multinn_amd import RnnNade, AdamOptimizer
    B, T, rho = 16, 5, 0.03
    x = synth(B, T, 37, rho)
    p, c0 = params(41, rho)
    fw, g, _, _ = nade_oracle(x, p, c0, 0.9)
    fw["api_nll"] = fw["nll"]
    gen = RnnNade(D, HN, UNITS, keep_prob=0.9, precision="fp32", seed=23, learn_zero_state=True)
    gen._materialize(D)
    load(gen, p, c0)
    gen.build_pianoroll(dev(x), None, is_train=True, mode="train")
    assert not gen._ctx["lstm"][0].get("rowpar") and not gen._ctx["lstm"][0].get("persist")
    errs, cosv, cp_err = _compare(gen, fw, g, f"learned state, fp32 B={B} T={T}")
    assert all(v < 1e-4 for v in errs.values()), errs
    assert cp_err < 2e-5
    # ---- the optimiser step (the check of test_real_width_optimiser_step_fp32_vs_oracle, with the new variables) ----
    load(gen, p, c0)
    before = {n: gen.store[n].clone() for n in gen.store.names()}
    gen.train_step(dev(x), None, AdamOptimizer(0.01))
    flat_p = [a.copy() for pair in p['lstm'] for a in pair] + [c.copy() for c in c0] + [np.stack(p['w_enc']), np.stack(p['w_dec']), p['fc_k'].copy(), p['fc_b'].copy()]
    ref_before = [a.copy() for a in flat_p]
    gn = G.apply_clip_adam(flat_p, oracle_grads(g), G.new_opt(flat_p), lr=0.01)
    assert abs(float(gen._grad_sumsq.sqrt()) - gn) < 1e-4 * gn
    for name, ra, rb in zip(gen.store.names(), flat_p, ref_before):
        upd = (gen.store[name] - before[name]).cpu().numpy().reshape(ra.shape)
        assert np.abs(upd - (ra - rb)).max() < 2e-4, name
    for l in range(2):
        assert float((gen.store[f"rnn/cell_{l}/c0"] - before[f"rnn/cell_{l}/c0"]).abs().max()) > 1e-3


def test_launch_per_timestep_path_fp16_small_batch_vs_oracle(monkeypatch):
    """What the README says of small batches in 16 bits: with the flag a training window takes the launch-per-timestep kernels (the two-layer
    persistent form, which such a batch runs on otherwise, has no state gradient) -- mnn_lstm_seq_fwd / _bwd with h0 / c0 in and dh0 / dc0 out
    on loss-scaled f16 operands.  B = 32, T = 8 against the oracle at the fp16 bounds of test_joint_lstm_nade_step_at_real_widths_vs_oracle
    (forward quantities 1e-4, gradients 3e-3), the c0 gradients included."""
    from multinn_amd import RnnNade
    B, T, rho = 32, 8, 0.03
    x = synth(B, T, 37, rho)
    p, c0 = params(41, rho)
    fw, g, _, _ = nade_oracle(x, p, c0, 0.9)
    fw["api_nll"] = fw["nll"]
    gen = RnnNade(D, HN, UNITS, keep_prob=0.9, precision="fp16", seed=23, learn_zero_state=True)
    gen._materialize(D)
    load(gen, p, c0)
    calls = Calls(monkeypatch)
    gen.build_pianoroll(dev(x), None, is_train=True, mode="train")
    assert gen._stack._persist(B, T) and not gen._ctx["lstm"][0].get("rowpar") and not gen._ctx["lstm"][0].get("persist")
    errs, cosv, cp_err = _compare(gen, fw, g, f"learned state, launch per timestep fp16 B={B} T={T}")
    assert calls.n["lstm2_persist_fwd"] == 0 and calls.n["lstm2_persist_bwd"] == 0 and calls.n["lstm_seq_bwd"] >= 2
    assert errs["loss"] < 1e-4 and errs["nll"] < 1e-4 and cp_err < 1e-4, (errs, cp_err)
    assert all(v < 3e-3 for v in errs.values()), errs


def test_ragged_window_with_learned_state_vs_oracle():
    """A ragged window (lengths ~ U{T/2..T}, seed 24) at fp16, B = 256: loss and gradients against the oracle composition with row weights
    (oracle.generators.row_weights); every row is valid at t = 0, so all B rows contribute to the c0 gradients."""
    from multinn_amd import RnnNade
    B, T, rho = 256, 8, 0.03
    x = synth(B, T, 37, rho)
    lengths = np.random.Generator(np.random.PCG64(24)).integers(T // 2, T + 1, B)
    p, c0 = params(41, rho)
    fw, g, _, _ = nade_oracle(x, p, c0, 0.9, lengths)
    gen = RnnNade(D, HN, UNITS, keep_prob=0.9, precision="fp16", seed=23, learn_zero_state=True)
    gen._materialize(D)
    load(gen, p, c0)
    gen._stack.rowpar_min_batch = 32
    gen.build_pianoroll(dev(x), torch.from_numpy(lengths.astype(np.int32)), is_train=True, mode="train")
    assert gen._ctx["lstm"][0].get("rowpar") and gen._ctx["lstm"][0]["c0"] is not None
    fw["api_nll"] = fw["nll"]                               # b-major then t over the valid rows: the order of y[valid]
    errs, cosv, cp_err = _compare(gen, fw, g, f"learned state, ragged fp16 B={B} T={T}")
    assert errs["loss"] < 1e-4 and errs["nll"] < 1e-4 and cp_err < 1e-4, (errs, cp_err)
    assert all(v < 3e-3 for v in errs.values()), errs
    assert all(c > 0.99999 for c in cosv.values()), cosv


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_evaluation_and_estimate_nll_start_from_the_learned_state(precision):
    """An evaluation build at a small batch (fp16: the two-layer persistent forward, which takes a state; fp32: launch per timestep) and
    estimate_nll start from zero_state too: loss and per-row NLL against the oracle forward with keep_prob 1."""
    from multinn_amd import RnnNade
    B, T, rho = 32, 8, 0.03
    x = synth(B, T, 37, rho)
    p, c0 = params(41, rho)
    fw, _, _, _ = nade_oracle(x, p, c0, 1.0)
    gen = RnnNade(D, HN, UNITS, keep_prob=0.9, precision=precision, seed=23, learn_zero_state=True)
    gen._materialize(D)
    load(gen, p, c0)
    gen.build_pianoroll(dev(x), None, is_train=False, mode="eval")
    if precision == "fp16":
        assert gen._stack._persist(B, T)
    e_loss = abs(float(gen.metrics["batch/loss"]) - fw['loss']) / abs(fw['loss'])
    e_nll = rel(gen.log_probs.cpu().numpy(), fw['nll'])
    est = gen.estimate_nll(dev(x).view(B, T, D))
    print(f"\n[eval {precision}] loss {e_loss:.2e}  per-row NLL {e_nll:.2e}  estimate_nll mean {est.mean:.6f} (oracle {fw['loss']:.6f})")
    assert e_loss < 1e-4 and e_nll < 1e-4
    assert abs(est.mean - fw['loss']) < 1e-4 * abs(fw['loss'])
    # ... and the check sees the state: the same weights from the zero state miss the tolerance above (else it would show nothing)
    for l in range(2):
        gen.store[f"rnn/cell_{l}/c0"].zero_()
    gen.build_pianoroll(dev(x), None, is_train=False, mode="eval")
    assert abs(float(gen.metrics["batch/loss"]) - fw['loss']) > 1e-4 * abs(fw['loss'])
    assert rel(gen.log_probs.cpu().numpy(), fw['nll']) > 1e-4


def test_graphed_train_step_with_learned_state_matches_eager():
    """Two replays of graphed_train_step equal two eager train_steps (the check of test_gpu_generators.py::
    test_graphed_train_step_matches_eager) and c0 differs after each: the tiling of zero_state runs inside the graph."""
    from multinn_amd import RnnNade, AdamOptimizer
    B, T, rho = 256, 8, 0.1
    xs = [dev(synth(B, T, 50 + i, rho)) for i in range(2)]
    gens = []
    for _ in range(2):
        gen = RnnNade(D, HN, UNITS, keep_prob=0.9, precision="fp16", seed=23, learn_zero_state=True)
        gen._materialize(D)
        gen._stack.rowpar_min_batch = 32
        for l, u in enumerate(UNITS):
            gen.store[f"rnn/cell_{l}/c0"].copy_(torch.linspace(-0.3, 0.3, u, device=DEV).view(1, u))
        gens.append(gen)
    ge, gg = gens
    opt_e, opt_g = AdamOptimizer(0.01), AdamOptimizer(0.01)
    c0_seen = [gg.store["rnn/cell_0/c0"].clone()]
    run = gg.graphed_train_step(xs[0], opt_g, warmup=0)
    assert gg._ctx["lstm"][0].get("rowpar") and gg._ctx["lstm"][0]["c0"] is not None
    for x in xs:
        le = float(ge.train_step(x, None, opt_e))
        lg = float(run(x))
        assert abs(le - lg) < 1e-5 * abs(le) + 1e-6, (le, lg)
        c0_seen.append(gg.store["rnn/cell_0/c0"].clone())
        assert not torch.equal(c0_seen[-1], c0_seen[-2])
    for n in ge.store.names():
        a, b = ge.store[n], gg.store[n]
        assert float((a - b).abs().max()) < 1e-4 * max(1.0, float(a.abs().max())), n
    ge.check(); gg.check()


def test_multinade_with_learned_state_vs_oracle():
    """RnnMultiNADE (one LSTM, three NADEs) with the flag, fp16, B = 256 on the cluster / CU-resident kernels through build(x, y)."""
    from multinn_amd import RnnMultiNADE
    B, T, E, tracks = 256, 6, 24, 3
    Dm = E * tracks
    rng = np.random.default_rng(4)
    seq = (rng.random((B, T + 1, Dm)) < 0.1).astype(np.float64)
    p = G.init_rnn_nade(7, Dm, E, 64, UNITS, np.float64, tracks=tracks)
    for W, b in p['lstm']:
        b += 0.05
    c0 = [rng.normal(0, 0.3, (1, u)) for u in UNITS]
    fw, g, _, _ = nade_oracle_xy(seq[:, :-1], seq[:, 1:], p, c0, 0.9, tracks=tracks)
    gen = RnnMultiNADE(E, 64, UNITS, tracks=list("abc"), keep_prob=0.9, precision="fp16", seed=23, learn_zero_state=True)
    gen._materialize(Dm)
    load(gen, p, c0)
    gen._stack.rowpar_min_batch = 32
    gen.build(dev(seq[:, :-1].astype(np.float32)), dev(seq[:, 1:].astype(np.float32)), None, True, "train")
    assert gen._ctx["lstm"][0].get("rowpar") and gen._ctx["lstm"][0]["c0"] is not None
    e_loss = abs(float(gen.metrics["batch/loss"]) - fw['loss']) / fw['loss']
    e_nll = max(rel(gen.log_probs[t].cpu().numpy(), fw['nll'][t]) for t in range(tracks))
    gen.backward()
    gen._stack.check()
    errs = {name: rel(gen.store.gviews[name].cpu().numpy().reshape(ref.shape), ref) for name, ref in zip(gen.store.names(), oracle_grads(g))}
    print(f"\n[MultiNADE learned state fp16] loss {e_loss:.2e}  per-row NLL {e_nll:.2e}  gradients {errs}")
    assert e_loss < 1e-4 and e_nll < 1e-4                 # FWD_TOL / GRAD_TOL of test_gpu_realmodes.py for fp16
    assert all(v < 3e-3 for v in errs.values()), errs


def rbm_oracle(inp, tgt, p, c0, k, seed, v_sample, keep_prob=0.9, units=UNITS):
    """oracle.generators.rnn_rbm_forward / _backward (conditional bias mode, full-length rows) restated with an initial state, cost and
    gradients on the given chain ends (the device's own: test_gpu_realmodes.py::test_c3_jamming_real_widths does the same)."""
    from oracle import rbm as orbm
    B, T, _ = inp.shape
    y, _, cache = olstm.seq_fwd(inp, p['lstm'], keep_prob, G.dropout_uniforms(seed, B, T, units), None, 'dynamic_rnn', init_state=state_of(c0, B))
    yf = y.reshape(B * T, -1)
    bh_t, bv_t = p['bh'] + yf @ p['Wuh'], p['bv'] + yf @ p['Wuv']
    tg = tgt.reshape(B * T, -1)
    rows = np.array([t * 65536 + b for b in range(B) for t in range(T)])
    u_h, u_v = G.gibbs_uniforms(seed, rows, k, p['W'].shape[1], p['W'].shape[0])
    _, v_own = orbm.gibbs(inp.reshape(B * T, -1), p['W'], bh_t, bv_t, k, u_h, u_v)
    vs = v_own if v_sample is None else v_sample
    cost, F = orbm.free_energy_cost(tg, vs, p['W'], bh_t, bv_t)
    rw = np.full(B * T, 1.0 / (B * T))
    dW, dbh, dbv = orbm.free_energy_cost_bwd(tg, vs, p['W'], bh_t, bv_t, rw)
    g = dict(W=dW, bh=dbh.sum(0, keepdims=True), bv=dbv.sum(0, keepdims=True), Wuh=yf.T @ dbh, Wuv=yf.T @ dbv)
    dy = (dbh @ p['Wuh'].T + dbv @ p['Wuv'].T).reshape(B, T, -1)
    _, g['lstm'] = olstm.seq_bwd(dy, cache)
    _, g['c0'] = state_grads(cache, dy, c0)
    return dict(cost=cost, F=F, agree=float((v_own == vs).all(1).mean())), g


def rbm_grad_list(g):
    """Order of RnnRBM's variables with the flag: rbm [W, bv, bh], rnn (cells, then the c0s), Wuh, Wuv."""
    out = [g['W'], g['bv'], g['bh']]
    for W, b in g['lstm']:
        out += [W, b]
    return out + list(g['c0']) + [g['Wuh'], g['Wuv']]


def load_rbm(gen, p, c0):
    s = gen.store
    for l, (W, b) in enumerate(p['lstm']):
        s[f"rnn/cell_{l}/kernel"].copy_(dev(W.astype(np.float32))); s[f"rnn/cell_{l}/bias"].copy_(dev(b.astype(np.float32)))
        s[f"rnn/cell_{l}/c0"].copy_(dev(c0[l].astype(np.float32)))
    for kk in ("W", "bh", "bv"):
        s[f"rbm/{kk}"].copy_(dev(p[kk].astype(np.float32)))
    s["Wuh"].copy_(dev(p['Wuh'].astype(np.float32))); s["Wuv"].copy_(dev(p['Wuv'].astype(np.float32)))
    gen._packed_step = -1


def _rbm_params(seed, i=0):
    p = G.init_rnn_rbm(seed, P, P, HN, UNITS, np.float64)
    p['bh'] += 0.05 * i
    p['bv'] += np.log(0.05 / 0.95)
    rng = np.random.Generator(np.random.PCG64(seed + 7))
    return p, [rng.normal(0, 0.3, (1, u)) for u in UNITS]


def test_rnn_rbm_with_learned_state_vs_oracle():
    """RnnRBM(88, 256, [512, 256], learn_zero_state=True), conditional bias mode, fp16, B = 256: cost / free energy and gradients at the
    bounds of test_gpu_realmodes.py::test_c3_jamming_real_widths for the precision (1e-4 / 3e-3), the c0 gradients held like the bias gradients."""
    from multinn_amd import RnnRBM
    B, T, k = 256, 8, 10
    rng = np.random.default_rng(8)
    seq = (rng.random((B, T + 1, P)) < 0.05).astype(np.float64)
    inp, tgt = seq[:, :-1], seq[:, 1:]
    p, c0 = _rbm_params(50)
    gen = RnnRBM(P, HN, UNITS, keep_prob=0.9, k=k, precision="fp16", seed=23, learn_zero_state=True)
    gen._materialize(P)
    load_rbm(gen, p, c0)
    gen._stack.rowpar_min_batch = 32
    gen.build(dev(inp.astype(np.float32)), dev(tgt.astype(np.float32)), None, True, "train")
    assert gen._ctx["lstm"][0].get("rowpar") and gen._ctx["lstm"][0]["c0"] is not None and gen.bias_mode == "conditional"
    vs = gen._outputs.cpu().numpy()
    fw, g = rbm_oracle(inp, tgt, p, c0, k, gen.seed, vs.astype(np.float64))
    e_F = rel(gen.free_energy.cpu().numpy(), fw['F'])
    e_loss = abs(float(gen.metrics["batch/loss"]) - fw['cost'].mean()) / max(1.0, abs(fw['cost'].mean()))
    gen.backward()
    gen._stack.check()
    errs = {name: rel(gen.store.gviews[name].cpu().numpy().reshape(ref.shape), ref) for name, ref in zip(gen.store.names(), rbm_grad_list(g))}
    print(f"\n[RnnRBM learned state fp16] free energy {e_F:.2e}  loss {e_loss:.2e}  chain ends equal {fw['agree']:.3f}  gradients {errs}")
    assert gen.store.names()[7:9] == ["rnn/cell_0/c0", "rnn/cell_1/c0"]
    assert fw['agree'] >= 0.99 and e_F < 1e-4 and e_loss < 1e-4
    assert all(v < 3e-3 for v in errs.values()), errs


def test_jamming_mode_with_learned_state_in_lockstep(monkeypatch):
    """The jamming mode with generator.learn_zero_state, B = 256: the five generators run in lockstep (the _multi / _state_multi launches are
    asserted) and agree with the same model running them one after the other (launch-per-timestep kernels at this batch size) as
    test_gpu_realmodes.py::test_c3_jamming_generators_in_lockstep_equal_one_after_the_other compares them; track 0's c0 gradients against the
    oracle composition on the device's chain ends (bias-gradient bound)."""
    import test_gpu_modes as TM
    from multinn_amd import MultINN, AdamOptimizer
    B, T, k = 256, 6, 10
    xh = TM.batch(B, T, P, M, 9, rho=0.05)
    x = TM.dev(xh)
    prm = TM.params("jamming", gen="RBM", Hn=HN, units=UNITS)
    prm["generator"]["learn_zero_state"] = True
    res = []
    for grouped in (True, False):
        m = MultINN(TM.config(P, TM.TRACKS5), prm, mode="jamming", precision="fp16", seed=23)
        m.group_generators = grouped
        m.build(x, lengths=None, is_train=True, mode="train")
        ps = [_rbm_params(50 + i, i) for i in range(M)]
        for g_, (p_, c0_) in zip(m.generators, ps):
            load_rbm(g_, p_, c0_)
        calls = Calls(monkeypatch)
        m.build(x, lengths=None, is_train=True, mode="train")
        assert bool(getattr(m, "_built_grouped", False)) == grouped and all(g_.learn_zero_state for g_ in m.generators)
        fe = [g_.free_energy.clone() for g_ in m.generators]
        vs0 = m.generators[0]._outputs.cpu().numpy().astype(np.float64)
        m.train_generators(AdamOptimizer(0.01), 0.01)
        m.check()
        if grouped:
            assert all(g_._ctx["lstm"][0].get("rowpar") and g_._ctx["lstm"][0]["c0"] is not None for g_ in m.generators)
            assert sorted(calls.kinds) == ["cluster_bwd", "cluster_fwd", "resident_bwd", "resident_fwd"], calls.kinds
            assert calls.n["lstm_seq_fwd"] == 0 and calls.n["lstm_seq_bwd"] == 0
            tr = G.per_track_inputs(xh)[0]
            _, g0 = rbm_oracle(tr[:, :-1].astype(np.float64), tr[:, 1:].astype(np.float64), ps[0][0], ps[0][1], k, m.generators[0].seed, vs0)
            for l in range(2):
                e = rel(m.generators[0].store.gviews[f"rnn/cell_{l}/c0"].cpu().numpy(), g0['c0'][l] / M)
                print(f"    jamming track 0 c0 gradient layer {l}: rel {e:.3e}")
                assert e < 3e-3, (l, e)
        else:
            assert calls.kinds == [] and calls.n["lstm_seq_fwd"] > 0 and calls.n["lstm_seq_bwd"] > 0
        monkeypatch.undo()
        res.append((fe, [g_.store.grad.clone() for g_ in m.generators], float(m.generator_loss())))
    (fa, ga, la), (fb, gb, lb) = res
    for a, b in zip(fa, fb):
        assert float((a - b).abs().max()) < 2e-3 * float(b.abs().max())
    assert abs(la - lb) < 2e-2 * max(1.0, abs(lb)), (la, lb)
    for a, b in zip(ga, gb):
        assert bool(torch.isfinite(a).all()) and float(torch.nn.functional.cosine_similarity(a, b, dim=0)) > 0.98


# ------------------------------------------------------------------------------------------------ generation
GU = [128, 64]


def _small(cls, learn, **kw):
    gen = cls(P, 64, GU, precision="fp16", seed=23, learn_zero_state=learn, **kw)
    gen._materialize(P)
    return gen


def _set_c0(gen):
    for l, u in enumerate(GU):
        gen.store[f"rnn/cell_{l}/c0"].copy_(torch.linspace(-1.5, 1.5, u, device=DEV).view(1, u))
    gen._packed_step = -1


def _device_state(gen, B):
    """(c0, h0) as the device formed them (f32, tiled): the checker starts from the same bits."""
    return [(c.cpu().numpy(), h.cpu().numpy()) for c, h in gen._rnn.zero_state(B, torch.float32)]


def _lstm_params(gen):
    n = lambda k: gen.store[k].cpu().numpy()          # noqa: E731
    return [(n(f"rnn/cell_{l}/kernel"), n(f"rnn/cell_{l}/bias")) for l in range(len(GU))]


@pytest.mark.parametrize("kind", ["nade", "rbm"])
def test_generate_with_zero_c0_equals_the_flag_off_model(kind, monkeypatch):
    """With c0 = 0 the samples of a flag-on model equal the flag-off model's bit for bit (same seed: zeros_init draws nothing, so every other
    weight is the same); with c0 != 0 they differ, and the eager loop (MULTINN_GENERATE_GRAPH=0) equals the captured scan."""
    from multinn_amd import RnnNade, RnnRBM
    cls, kw = (RnnNade, {}) if kind == "nade" else (RnnRBM, dict(k=3))
    g_off, g_on = _small(cls, False, **kw), _small(cls, True, **kw)
    for n in g_off.store.names():
        assert torch.equal(g_off.store[n], g_on.store[n]), n
    intro = dev((np.random.default_rng(3).random((6, 4, P)) < 0.1).astype(np.uint8))
    a, b = g_off.generate(intro, 8), g_on.generate(intro, 8)
    assert torch.equal(a, b)
    _set_c0(g_on)
    c = g_on.generate(intro, 8)
    assert not torch.equal(b, c)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(g_on.generate(intro, 8), c)


def test_nade_generate_from_learned_state_equals_the_step_by_step_checker(monkeypatch):
    """generate() (the captured one-call scan, mnn_generate_scan_state with c0 / h0 as input arrays) of an LSTM-NADE with c0 != 0 against
    oracle/det started from the (c0, h0) read back from the device: 72 intros x 32 steps, every cell."""
    from multinn_amd import RnnNade, ops as o
    from oracle import det, philox
    gen = _small(RnnNade, True)
    _set_c0(gen)
    B, Ti, steps = 72, 4, 32
    intro = (np.random.default_rng(5).random((B, Ti, P)) < 0.1).astype(np.uint8)
    seen, real = [], o.generate_scan

    def spy(*a, **kw):
        seen.append(kw.get("state0"))
        return real(*a, **kw)
    monkeypatch.setattr(o, "generate_scan", spy)
    got = gen.generate(dev(intro), steps).cpu().numpy()
    assert seen and all(st is not None and tuple(st[0][1].shape) == (B, GU[0]) and st[0][1].dtype == torch.float32 for st in seen)
    n = lambda k: gen.store[k].cpu().numpy()          # noqa: E731
    layers = _lstm_params(gen)
    state, h = _device_state(gen, B), None
    for t in range(Ti):
        h, state = det.lstm_step(intro[:, t], state, layers)
    out = det.dense(h, n("dense/kernel"), n("dense/bias"))
    rows = np.arange(0, B, dtype=np.uint32)
    ref = np.empty((B, steps, P), np.uint8)
    for s_ in range(steps):
        u = philox.uniform_block(gen.seed, philox.STREAM_NADE, rows, s_, P)
        step = det.nade_sample(out, n("nade/w_enc")[0], n("nade/w_dec")[0], 1, 0, P, 64, 1.0, u)[0]
        ref[:, s_] = step
        h, state = det.lstm_step(step, state, layers)
        out = det.dense(h, n("dense/kernel"), n("dense/bias"))
    assert got.shape == ref.shape and int((got != ref).sum()) == 0, int((got != ref).sum())
    assert 0 < int(got.sum()) < got.size


def test_rbm_generate_from_learned_state_equals_the_step_by_step_checker():
    """The same for an LSTM-RBM (k = 3 Gibbs steps per generated step)."""
    from multinn_amd import RnnRBM
    from oracle import det
    k = 3
    gen = _small(RnnRBM, True, k=k)
    _set_c0(gen)
    B, Ti, steps = 24, 4, 12
    intro = (np.random.default_rng(6).random((B, Ti, P)) < 0.1).astype(np.uint8)
    got = gen.generate(dev(intro), steps).cpu().numpy()
    n = lambda k_: gen.store[k_].cpu().numpy()         # noqa: E731
    layers = _lstm_params(gen)
    pre = gen._rbm.prefix
    state, h = _device_state(gen, B), None
    for t in range(Ti):
        h, state = det.lstm_step(intro[:, t], state, layers)
    bh0, bv0 = n(f"{pre}/bh").reshape(-1), n(f"{pre}/bv").reshape(-1)
    rows = np.arange(0, B, dtype=np.uint32)
    prev = np.ascontiguousarray(intro[:, -1], np.uint8)
    ref = np.empty((B, steps, P), np.uint8)
    for s_ in range(steps):
        bh_t, bv_t = det.dense(h, n("Wuh"), bh0), det.dense(h, n("Wuv"), bv0)
        u_h, u_v = G.gibbs_uniforms(gen.seed, rows, k, 64, P, sub0=s_ * k)
        _, v = det.rbm_gibbs(prev, n(f"{pre}/W"), bh_t, bv_t, k, u_h, u_v)
        ref[:, s_] = v
        h, state = det.lstm_step(v, state, layers)
        prev = v
    assert got.shape == ref.shape and int((got != ref).sum()) == 0, int((got != ref).sum())
