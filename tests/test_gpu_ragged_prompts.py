"""Ragged prompts on the GPU.  The statement under test (DESIGN.md section 4 "Ragged prompts"): row b of a call with `lengths` is, bit for
bit, the one-row call on x[b:b+1, :lengths[b]] with row0 + b.  The kernel (mnn_lstm_step_det_ragged) against the plain step and the
deterministic checker; the scan and every generator against the checker called per row (a row is independent, so that IS the reference)
or, where the checker has no form (given, per-track temperature, caps, particles, RnnMultiRBM, float inputs), against the generator's own
one-row calls; padding insensitivity; the graph cache; sessions; the joint, jamming and composer modes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import generators as G, det   # noqa: E402
from test_gpu_session import dev, load_nade_params, load_rbm_params, multirbm_gen as _multirbm_gen, chunks, random_codes, DEV, FREE, ABC   # noqa: E402

E, HN, UNITS, TI, STEPS = 8, 16, [32, 32], 5, 4
LENS5 = (5, 1, 3, 5, 2)


def lens_of(B):
    """B = 5: the issue's lengths.  B = 35: rows 32..34 (the second tile) all have length 1, so that tile is finished from t = 1 on, and
    tile 0 holds every length."""
    if B == 5:
        return LENS5
    return tuple(int(v) for v in np.random.default_rng(35).integers(1, TI + 1, 32)) + (1, 1, 1)


def intro_of(B, Din, seed=6):
    return (np.random.default_rng(seed).random((B, TI, Din)) < .3).astype(np.uint8)


# The generators of tests/test_gpu_session.py with their recurrent and Dense weights scaled up: at the initialisers' scale the conditionals
# of these tiny models barely move with the LSTM state, and a scan that ignored the lengths would still emit nearly the same cells.  With
# them the padded call differs from the ragged one in many cells (asserted below), so the bit-exact comparisons can tell the two apart.
def nade_gen(tracks, E, Hn, units, seed=31):
    from multinn_amd import RnnNade, RnnMultiNADE
    Din = E * tracks
    gen = RnnNade(E, Hn, units, precision="fp32", seed=seed) if tracks == 1 else RnnMultiNADE(E, Hn, units, tracks=ABC[:tracks], precision="fp32", seed=seed)
    gen._materialize(Din)
    p = G.init_rnn_nade(9, Din, E, Hn, units, np.float32, tracks=tracks)
    p['lstm'] = [((W * np.float32(3)).astype(np.float32), b) for W, b in p['lstm']]
    p['fc_k'] = (p['fc_k'] * np.float32(6)).astype(np.float32)
    load_nade_params(gen, p)
    return gen, p


def rbm_gen(D, Hn, units, k, seed=41):
    from multinn_amd import RnnRBM
    p = G.init_rnn_rbm(27, D, D, Hn, units, np.float32)
    p['bh'] += np.float32(0.1); p['bv'] -= np.float32(0.3)
    p['lstm'] = [((W * np.float32(3)).astype(np.float32), b) for W, b in p['lstm']]
    p['Wuh'], p['Wuv'] = (p['Wuh'] * np.float32(6)).astype(np.float32), (p['Wuv'] * np.float32(6)).astype(np.float32)
    gen = RnnRBM(D, Hn, units, k=k, precision="fp16", seed=seed)
    gen._materialize(D)
    load_rbm_params(gen, p)
    return gen, p


def multirbm_gen(D, Hn, units, k, M=3):
    gen = _multirbm_gen(D, Hn, units, k, M)
    gen.store.theta.mul_(3.0)
    gen._packed_step = -1
    return gen


def differing_rows(a, b):
    return sorted(set(torch.nonzero(a != b)[:, 0].tolist()))


# ------------------------------------------------------------------------------------------------
# 1. the kernel
B_K = 40                                                             # rows 32..39: a second tile of 32
GUARD = 8
SENTINEL = 7777.0


def _kernel_problem():
    R = np.random.default_rng(3)
    jobs = []
    for n_x, n_x2, u, u8 in ((11, 0, 32, True), (32, 5, 64, False)):          # u8 with an odd K (the pad column); f32 with a second block
        K = n_x + n_x2 + u
        x = (R.random((B_K, n_x)) < .4).astype(np.uint8) if u8 else R.standard_normal((B_K, n_x)).astype(np.float32)
        jobs.append(dict(x=x, x2=R.standard_normal((B_K, n_x2)).astype(np.float32) if n_x2 else None,
                         W=(R.standard_normal((K, 4 * u)) * .3).astype(np.float32), b=(R.standard_normal(4 * u) * .1).astype(np.float32),
                         c=R.standard_normal((B_K, u)).astype(np.float32), h=np.tanh(R.standard_normal((B_K, u))).astype(np.float32), u=u))
    return jobs


def _launch(prob, packed, lengths=None, t=0, state=True, nan_rows=None):
    """Both jobs in ONE launch -> [(c_out, h_out) with GUARD rows behind B], and the reference of every row as if it were live."""
    from multinn_amd import ops
    jobs, outs, refs = [], [], []
    for j in prob:
        x = j["x"].copy()
        if nan_rows is not None and x.dtype == np.float32:
            x[nan_rows] = np.nan                                     # what a frozen row stages must reach no other row
        c_out, h_out = (torch.full((B_K + GUARD, j["u"]), SENTINEL, device=DEV) for _ in range(2))
        W = dev(j["W"])
        jobs.append(dict(x=dev(x), x2=None if j["x2"] is None else dev(j["x2"]), W=W, bias=dev(j["b"]), c_out=c_out[:B_K], h_out=h_out[:B_K],
                         c_prev=dev(j["c"]) if state else None, h_prev=dev(j["h"]) if state else None,
                         Wp=ops.det_lstm_pack(W, j["u"]) if packed else None))
        outs.append((c_out, h_out))
        xin = j["x"].astype(np.float32) if j["x2"] is None else np.concatenate([j["x"].astype(np.float32), j["x2"]], 1)
        _, new = det.lstm_step(xin, [(j["c"], j["h"])] if state else None, [(j["W"], j["b"])])
        refs.append(new[0])
    if lengths is None:
        ops.lstm_step_det(jobs)
    else:
        ops.lstm_step_det(jobs, lengths=lengths, t=t)
    torch.cuda.synchronize()
    return [(c.cpu().numpy(), h.cpu().numpy()) for c, h in outs], refs


@pytest.mark.parametrize("packed", [False, True], ids=["tf_layout", "packed"])
def test_step_freezes_finished_rows_and_leaves_live_rows_alone(packed):
    """(a) at t = 2 tile 0 is mixed and tile 1 wholly frozen (the short cut): live rows = mnn_lstm_step_det's bits = the checker's, frozen
    rows = their previous state, bit for bit -- zeros without one --, guard rows untouched.  (b) all rows live: the plain launch, byte
    for byte."""
    prob = _kernel_problem()
    t = 2
    lens = np.array([(1, 2, 3, 4, 5)[r % 5] for r in range(32)] + [1, 2] * 4, np.int32)
    live = lens > t
    assert live[:32].any() and not live[:32].all() and not live[32:].any()
    plain, refs = _launch(prob, packed)
    got, _ = _launch(prob, packed, lengths=dev(lens), t=t, nan_rows=~live)
    for j, ((c, h), (pc, ph), (rc, rh)) in enumerate(zip(got, plain, refs)):
        assert np.array_equal(pc[:B_K], rc) and np.array_equal(ph[:B_K], rh), "the plain step against the checker"
        assert np.array_equal(c[:B_K][live], pc[:B_K][live]) and np.array_equal(h[:B_K][live], ph[:B_K][live]), j
        assert np.array_equal(c[:B_K][~live], prob[j]["c"][~live]) and np.array_equal(h[:B_K][~live], prob[j]["h"][~live]), j
        assert np.all(c[B_K:] == SENTINEL) and np.all(h[B_K:] == SENTINEL), "rows behind B"
    # no previous state: a frozen row is the zero state
    got0, refs0 = _launch(prob, packed, lengths=dev(lens), t=t, state=False)
    for (c, h), (rc, rh) in zip(got0, refs0):
        assert np.array_equal(c[:B_K][live], rc[live]) and np.array_equal(h[:B_K][live], rh[live])
        assert not c[:B_K][~live].any() and not h[:B_K][~live].any()
        assert np.all(c[B_K:] == SENTINEL) and np.all(h[B_K:] == SENTINEL)
    # (b) every row live
    full, _ = _launch(prob, packed, lengths=dev(np.full(B_K, 5, np.int32)), t=t)
    for (c, h), (pc, ph) in zip(full, plain):
        assert c.tobytes() == pc.tobytes() and h.tobytes() == ph.tobytes()


def test_no_length_indexes_anything():
    """Lengths outside 1..Ti are the caller's error, but never an index: huge, zero and negative values only decide live or frozen."""
    prob = _kernel_problem()
    lens = np.array([2 ** 31 - 1, 0, -5, -2 ** 31] * 10, np.int32)
    live = lens > 3
    plain, _ = _launch(prob, True)
    got, _ = _launch(prob, True, lengths=dev(lens), t=3)
    for j, ((c, h), (pc, ph)) in enumerate(zip(got, plain)):
        assert np.array_equal(c[:B_K][live], pc[:B_K][live]) and np.array_equal(c[:B_K][~live], prob[j]["c"][~live])
        assert np.array_equal(h[:B_K][live], ph[:B_K][live]) and np.array_equal(h[:B_K][~live], prob[j]["h"][~live])
        assert np.all(c[B_K:] == SENTINEL) and np.all(h[B_K:] == SENTINEL)


def test_ops_refuse_bad_lengths_arguments():
    prob = _kernel_problem()
    for bad in (torch.ones(B_K, dtype=torch.int64, device=DEV), torch.ones(B_K - 1, dtype=torch.int32, device=DEV), torch.ones(B_K, dtype=torch.int32), [1] * B_K):
        with pytest.raises(ValueError, match="lengths int32"):
            _launch(prob, False, lengths=bad, t=0)


# ------------------------------------------------------------------------------------------------
# 2. the scan and the generators, row by row
_refs = {}


def nade_case(tracks, B):
    """(gen, x, lengths, the checker's rows), the reference computed once per process."""
    gen, p = nade_gen(tracks, E, HN, UNITS)
    x, lens = intro_of(B, E * tracks), lens_of(B)
    if (tracks, B) not in _refs:
        _refs[tracks, B] = np.concatenate([det.rnn_nade_generate(x[b:b + 1, :n], STEPS, p, gen.seed, row0=b, tracks=tracks) for b, n in enumerate(lens)])
    return gen, x, lens, _refs[tracks, B]


def one_row_calls(gen, x, lens, after=None, **kw):
    """The generator's own one-row calls: row b on x[b:b+1, :lens[b]] with row0 + b (given sliced with the row)."""
    rows, extra, row0 = [], [], gen.row0
    given = kw.pop("given", None)
    try:
        for b, n in enumerate(lens):
            gen.row0 = row0 + b
            rows.append(gen.generate(x[b:b + 1, :n].contiguous(), STEPS, given=None if given is None else given[b:b + 1].contiguous(), **kw))
            if after is not None:
                extra.append(after(gen))
    finally:
        gen.row0 = row0
    return torch.cat(rows), extra


@pytest.mark.parametrize("B", [5, 35])
@pytest.mark.parametrize("tracks", [1, 3])
def test_nade_rows_equal_the_checker_on_each_prompt(tracks, B):
    gen, x, lens, ref = nade_case(tracks, B)
    out = gen.generate(dev(x), STEPS, lengths=lens)
    assert out.shape == (B, STEPS, E * tracks) and out.dtype == torch.uint8
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), f"rows {sorted(set(np.argwhere(got != ref)[:, 0].tolist()))} differ"
    short = [b for b, n in enumerate(lens) if n < TI]
    padded = differing_rows(out, gen.generate(dev(x), STEPS))
    assert padded and set(padded) <= set(short), ("the padded call is another piece, in short rows only", padded)
    # the same through every accepted form of the argument, and the step-loop path (float inputs)
    for form in (list(lens), np.array(lens), torch.tensor(lens)):
        assert torch.equal(gen.generate(dev(x), STEPS, lengths=form), out)
    assert torch.equal(gen.generate(dev(x).float(), STEPS, lengths=lens), out)


def test_steps_returns_every_rows_own_state():
    gen, x, lens, _ = nade_case(1, 5)
    st = gen.steps(dev(x), lengths=lens)
    for b, n in enumerate(lens):
        one = gen.steps(dev(x[b:b + 1, :n]))
        for (c, h), (c1, h1) in zip(st.rnn_state, one.rnn_state):
            assert torch.equal(c[b:b + 1], c1) and torch.equal(h[b:b + 1], h1), b
    full = gen.steps(dev(x), lengths=[TI] * 5)
    for (c, h), (c1, h1) in zip(full.rnn_state, gen.steps(dev(x)).rnn_state):
        assert torch.equal(c, c1) and torch.equal(h, h1)


def test_rbm_rows_equal_the_checker_on_each_prompt():
    D, k, B = 8, 3, 5
    gen, p = rbm_gen(D, HN, UNITS, k)
    x = intro_of(B, D, seed=26)
    out = gen.generate(dev(x), STEPS, lengths=LENS5).cpu().numpy()
    ref = np.concatenate([det.rnn_rbm_generate(x[b:b + 1, :n], STEPS, p, k, gen.seed, row0=b) for b, n in enumerate(LENS5)])
    assert np.array_equal(out, ref), f"rows {sorted(set(np.argwhere(out != ref)[:, 0].tolist()))} differ"
    assert 0.02 < out.mean() < 0.98
    padded = gen.generate(dev(x), STEPS).cpu().numpy()
    assert np.array_equal(padded[[0, 3]], out[[0, 3]]) and not np.array_equal(padded, out), "the padded call is another piece in the short rows only"


def test_multirbm_and_float_inputs_equal_their_own_one_row_calls():
    D, k, M, B = 8, 3, 3, 5
    gen = multirbm_gen(D, HN, UNITS, k, M)
    x = dev(intro_of(B, D * M, seed=27))
    out = gen.generate(x, STEPS, lengths=LENS5)
    assert torch.equal(out, one_row_calls(gen, x, LENS5)[0])
    assert differing_rows(out, gen.generate(x, STEPS)), "the padded call is another piece"
    for tracks in (1, 3):
        gen, xn, lens, ref = nade_case(tracks, 5)
        xf = dev(xn).float()
        assert gen._scan_in_one_call(xf, STEPS) is None              # the step loop: steps(lengths=) and the gathered last rows
        assert torch.equal(gen.generate(xf, STEPS, lengths=lens), one_row_calls(gen, xf, lens)[0])


@pytest.mark.parametrize("case", ["given", "temperature", "max_notes_redraws", "particles"])
def test_nade_options_compose_row_by_row(case):
    """One case each of given, a per-track temperature, max_notes with redraws, and particles -- with their statistics."""
    tracks, B = 3, 5
    gen, x, lens, _ = nade_case(tracks, B)
    x = dev(x)
    R = np.random.default_rng(12)
    codes = dev(random_codes(R, (B, STEPS, E * tracks)))
    if case == "given":
        kw, after = dict(given=codes), None
    elif case == "temperature":
        kw, after = dict(temperature=(0.6, 1.0, 1.7)), None
    elif case == "max_notes_redraws":
        kw, after = dict(max_notes=(1, None, 2), redraws=3), lambda g: g.redraw_counts()
    else:
        kw, after = dict(given=codes, particles=8), lambda g: (g.particle_ess(), g.particle_picks())
    out = gen.generate(x, STEPS, lengths=lens, **kw)
    stats = after(gen) if after is not None else None
    rows, row_stats = one_row_calls(gen, x, lens, after=after, **dict(kw))
    assert torch.equal(out, rows), (case, int((out != rows).sum()))
    if case == "given":
        free = codes == FREE
        assert torch.equal(out[~free], codes[~free])
    if case == "max_notes_redraws":
        assert stats == (sum(s[0] for s in row_stats), sum(s[1] for s in row_stats)), (stats, row_stats)
        notes = out.reshape(B, STEPS, E, tracks).sum(2)
        assert int(notes[..., 0].max()) <= 1 and int(notes[..., 2].max()) <= 2
    if case == "particles":
        ess, picks = stats
        assert ess.shape == (B, STEPS, tracks)
        for b in range(B):
            assert torch.equal(ess[b:b + 1], row_stats[b][0]) and torch.equal(picks[b:b + 1], row_stats[b][1]), b
        assert float(ess.min()) >= 1.0 and float(ess.max()) <= 8.0


@pytest.mark.parametrize("kind", ["nade_u8", "nade_f32", "rbm_u8"])
def test_no_cell_behind_a_prompt_changes_an_output_bit(kind):
    """Every cell of x behind a row's length set to 1 (u8) or NaN (float inputs)."""
    if kind == "rbm_u8":
        gen, _ = rbm_gen(8, HN, UNITS, 3)
        x = dev(intro_of(5, 8, seed=26))
    else:
        gen, xn, _, _ = nade_case(3, 5)
        x = dev(xn)
    x = x.float() if kind == "nade_f32" else x
    pad = x.clone()
    for b, n in enumerate(LENS5):
        pad[b, n:] = float("nan") if kind == "nade_f32" else 1
    assert not torch.equal(pad[:, -1].nan_to_num(7.0), x[:, -1])
    assert torch.equal(gen.generate(pad, STEPS, lengths=LENS5), gen.generate(x, STEPS, lengths=LENS5))


# ------------------------------------------------------------------------------------------------
# 3. graphs
@pytest.mark.parametrize("kind", ["nade", "rbm"])
def test_full_lengths_are_the_call_without_them(kind):
    if kind == "nade":
        gen, xn, _, _ = nade_case(3, 5)
    else:
        gen, _ = rbm_gen(8, HN, UNITS, 3)
        xn = intro_of(5, 8, seed=26)
    x = dev(xn)
    plain = gen.generate(x, STEPS)
    n = len(gen._scan_graphs._cache)
    keys = list(gen._scan_graphs._cache)
    assert torch.equal(gen.generate(x, STEPS, lengths=[TI] * 5), plain)
    assert len(gen._scan_graphs._cache) == n and list(gen._scan_graphs._cache) == keys, "no graph entry of its own"


@pytest.mark.parametrize("kind", ["nade", "nade_f32", "rbm"])
def test_captured_and_eager_agree_and_new_lengths_replay_the_same_graph(monkeypatch, kind):
    if kind == "rbm":
        gen, p = rbm_gen(8, HN, UNITS, 3)
        xn = intro_of(5, 8, seed=26)
        ref = lambda lens: np.concatenate([det.rnn_rbm_generate(xn[b:b + 1, :n], STEPS, p, 3, gen.seed, row0=b) for b, n in enumerate(lens)])
    else:
        gen, p = nade_gen(3, E, HN, UNITS)
        xn = intro_of(5, E * 3)
        ref = lambda lens: np.concatenate([det.rnn_nade_generate(xn[b:b + 1, :n], STEPS, p, gen.seed, row0=b, tracks=3) for b, n in enumerate(lens)])
    x = dev(xn).float() if kind == "nade_f32" else dev(xn)
    other = (2, 5, 5, 1, 4)

    def eager(lens):
        monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
        out = gen.generate(x, STEPS, lengths=lens)
        monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
        return out

    first = gen.generate(x, STEPS, lengths=LENS5)
    n = len(gen._scan_graphs._cache)
    assert n == 1 and "lengths" in list(gen._scan_graphs._cache)[0]
    second = gen.generate(x, STEPS, lengths=other)                   # lengths baked into the nodes would give `first` again
    assert len(gen._scan_graphs._cache) == n
    assert np.array_equal(first.cpu().numpy(), ref(LENS5)) and np.array_equal(second.cpu().numpy(), ref(other))
    assert not torch.equal(first, second)
    assert torch.equal(first, eager(LENS5)) and torch.equal(second, eager(other))
    assert len(gen._scan_graphs._cache) == n


# ------------------------------------------------------------------------------------------------
# 4. sessions
@pytest.mark.parametrize("kind", ["nade", "rbm"])
def test_session_chunks_equal_the_one_call(kind):
    """NADE: the one-call form (mnn_generate_scan_chunk_ragged opens the session); RBM: the step loop (steps(lengths=), the gathered rows)."""
    if kind == "nade":
        gen, xn, _, ref = nade_case(3, 5)
    else:
        gen, _ = rbm_gen(8, HN, UNITS, 3)
        xn, ref = intro_of(5, 8, seed=26), None
    x = dev(xn)
    one = gen.generate(x, STEPS, lengths=LENS5)
    sess = gen.ragged_session(x, LENS5)
    assert sess._scan == (kind == "nade")
    got = chunks(sess, (1, 2, 1))
    assert torch.equal(got, one), int((got != one).sum())
    if ref is not None:
        assert np.array_equal(got.cpu().numpy(), ref)
    full = chunks(gen.ragged_session(x, [TI] * 5), (1, 2, 1))
    assert torch.equal(full, gen.generate(x, STEPS))


# ------------------------------------------------------------------------------------------------
# 5. modes
P, M = 8, 3
TRACKS = ["Drums", "Piano", "Guitar"]
MODE_LENS = (5, 1, 3, 2)


def make_mode(mode, x):
    from multinn_amd import MultINN
    cfg = {"model_name": "t", "data": {"pitch_range": {"lowest": 0, "highest": P}, "instruments": TRACKS, "beat_resolution": 4},
           "training": {"num_pixels": 1, "random_seed": 23}}
    prm = {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
           "generator": {"type": "NADE", "num_hidden": HN, "num_hidden_rnn": UNITS, "feedback": None, "k": 3}}
    m = MultINN(cfg, prm, mode=mode, precision="fp32")
    m.build(dev(x), lengths=None, is_train=False, mode="generate")
    return m


@pytest.mark.parametrize("mode", ["joint", "jamming", "composer"])
def test_modes_row_by_row_and_through_sessions(mode):
    x = (np.random.default_rng(14).random((4, TI, P, M)) < 0.3).astype(np.uint8)
    m = make_mode(mode, x)
    for g in m.generators:                                           # (see nade_gen: conditionals that move with the state)
        g.store.theta.mul_(3.0)
        g._packed_step = -1
    out = m.generate(STEPS, intro_lengths=MODE_LENS)
    assert out.shape == (4, STEPS, P, M) and out.dtype == torch.uint8
    padded = m.generate(STEPS)
    assert differing_rows(out, padded) and 0 not in differing_rows(out, padded), "the padded call is another piece in the short rows only"
    assert torch.equal(m.generate(STEPS, intro_lengths=[TI] * 4), padded)
    sess = m.ragged_session(MODE_LENS)
    got = torch.cat([sess.generate(n) for n in (1, 2, 1)], 1)
    assert torch.equal(got, out), int((got != out).sum())
    rows = []
    for b, n in enumerate(MODE_LENS):                                # the one-row model call: the same weights, built on the row's prompt
        m.build(dev(x[b:b + 1, :n]), lengths=None, is_train=False, mode="generate")
        for g in m.generators:
            g.row0 = b
        rows.append(m.generate(STEPS))
    rows = torch.cat(rows)
    assert torch.equal(out, rows), (mode, sorted(set(torch.nonzero(out != rows)[:, 0].tolist())))
