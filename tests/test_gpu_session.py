"""Generation sessions on the GPU: the chunks of a session, concatenated, are the one-call scan -- every cell (and the deterministic checker's,
where it applies: no `given`, scalar temperature); captured and eager sessions agree chunk by chunk; the session's graph cache, its
snapshots, row0 and the learned initial state; and the joint, jamming and composer modes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import generators as G, det   # noqa: E402

DEV = "cuda:0"
FREE = 255
ABC = list("abc")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def load_nade_params(gen, p):
    s = gen.store
    for l, (W, b) in enumerate(p['lstm']):
        s[f"rnn/cell_{l}/kernel"].copy_(dev(W.astype(np.float32)))
        s[f"rnn/cell_{l}/bias"].copy_(dev(b.astype(np.float32)))
    s["nade/w_enc"].copy_(dev(np.stack(p['w_enc']).astype(np.float32)))
    s["nade/w_dec"].copy_(dev(np.stack(p['w_dec']).astype(np.float32)))
    s["dense/kernel"].copy_(dev(p['fc_k'].astype(np.float32)))
    s["dense/bias"].copy_(dev(p['fc_b'].astype(np.float32)))


def load_rbm_params(gen, p):
    s = gen.store
    for l, (W, b) in enumerate(p['lstm']):
        s[f"rnn/cell_{l}/kernel"].copy_(dev(W)); s[f"rnn/cell_{l}/bias"].copy_(dev(b))
    for kk in ("W", "bh", "bv"):
        s[f"rbm/{kk}"].copy_(dev(p[kk]))
    s["Wuh"].copy_(dev(p['Wuh'])); s["Wuv"].copy_(dev(p['Wuv']))


def chunks(sess, split, given=None, temperature=1.0):
    """The session's chunks of `split` steps, concatenated; given: the whole block (sliced per chunk), a list with one entry per chunk, or None."""
    out, s = [], 0
    for i, n in enumerate(split):
        g = given[i] if isinstance(given, list) else (None if given is None else given[:, s:s + n].contiguous())
        t = temperature[i] if isinstance(temperature, list) else temperature
        out.append(sess.generate(n, given=g, temperature=t))
        assert out[-1].shape[1] == n and out[-1].dtype == torch.uint8 and sess.steps == s + n
        s += n
    return torch.cat(out, 1)


def random_codes(R, shape, density=0.3):
    vals = (R.random(shape) < 0.3).astype(np.uint8)
    return np.where(R.random(shape) < density, vals, FREE).astype(np.uint8)


def nade_gen(tracks, E, Hn, units, seed=31, precision="fp32", p_seed=9, **kw):
    from multinn_amd import RnnNade, RnnMultiNADE
    Din = E * tracks
    gen = RnnNade(E, Hn, units, precision=precision, seed=seed, **kw) if tracks == 1 else \
        RnnMultiNADE(E, Hn, units, tracks=ABC[:tracks], precision=precision, seed=seed, **kw)
    gen._materialize(Din)
    p = G.init_rnn_nade(p_seed, Din, E, Hn, units, np.float32, tracks=tracks)
    load_nade_params(gen, p)
    return gen, p


def rbm_gen(D, Hn, units, k, seed=41):
    from multinn_amd import RnnRBM
    p = G.init_rnn_rbm(27, D, D, Hn, units, np.float32)
    p['bh'] += np.float32(0.1); p['bv'] -= np.float32(0.3)
    gen = RnnRBM(D, Hn, units, k=k, precision="fp16", seed=seed)
    gen._materialize(D)
    load_rbm_params(gen, p)
    return gen, p


def multirbm_gen(D, Hn, units, k, M=3, seed=43):
    from multinn_amd import RnnMultiRBM
    gen = RnnMultiRBM(D, Hn, units, tracks=ABC[:M], k=k, precision="fp32", seed=seed)
    gen._materialize(D * M)
    g = torch.Generator().manual_seed(5)                      # biases off zero: conditionals that are not coin flips
    for m in range(M):
        gen.store[f"rbm_{m}/bv"].copy_((torch.rand(gen.store[f"rbm_{m}/bv"].shape, generator=g) - 0.8).to(DEV))
    return gen


# ------------------------------------------------------------------------------------------------
# 1. NADE: chunks against the one call and the checker
NADE_CASES = {"small": (5, 8, 16, {}), "full": (3, 24, 256, {}), "no_chunk": (5, 8, 16, {"MNN_SAMPLE_NO_CHUNK": "1"}), "rows130": (130, 8, 16, {})}


@pytest.mark.parametrize("tracks,case", [(t, c) for c in NADE_CASES for t in (1, 3) if (t, c) != (1, "rows130")])
def test_nade_chunks_equal_the_one_call_and_the_checker(monkeypatch, tracks, case):
    """Splits (1, 2, 3) and (3, 1, 2) of six steps (a one-step chunk: the ping-pong parity and the aliased state arrays).  `full`: Hn = 256, the
    FULL instantiations and the speculative kernel; `no_chunk`: the visible-at-a-time kernel; `rows130`: with three tracks N * njobs > 256
    rows, the eight-visible form."""
    B, E, Hn, env = NADE_CASES[case]
    Ti, units, steps = 4, [32, 32], 6
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    intro = (np.random.default_rng(6).random((B, Ti, E * tracks)) < .3).astype(np.uint8)
    gen, p = nade_gen(tracks, E, Hn, units)
    one = gen.generate(dev(intro), steps)
    assert np.array_equal(one.cpu().numpy(), det.rnn_nade_generate(intro, steps, p, 31, tracks=tracks))
    for split in ((1, 2, 3), (3, 1, 2)):
        sess = gen.session(dev(intro))
        assert sess._scan and sess.steps == 0
        got = chunks(sess, split)
        assert torch.equal(got, one), (split, int((got != one).sum()))


# ------------------------------------------------------------------------------------------------
# 2. RBM
@pytest.mark.parametrize("form", ["default", "no_mfma", "stream_w", "k1"])
def test_rbm_chunks_equal_the_one_call_and_the_checker(monkeypatch, form):
    B, Ti, D, Hn, units, steps = 10, 4, 24, 40, [64, 32], 9
    k = 1 if form == "k1" else 4
    if form == "no_mfma":
        monkeypatch.setenv("MNN_RBM_NO_MFMA", "1")
    if form == "stream_w":
        monkeypatch.setenv("MNN_RBM_STREAM_W", "1")
    intro = (np.random.default_rng(26).random((B, Ti, D)) < .3).astype(np.uint8)
    gen, p = rbm_gen(D, Hn, units, k)
    one = gen.generate(dev(intro), steps)
    assert np.array_equal(one.cpu().numpy(), det.rnn_rbm_generate(intro, steps, p, k, 41))
    sess = gen.session(dev(intro))
    assert not sess._scan
    got = chunks(sess, (4, 1, 4))
    assert torch.equal(got, one), int((got != one).sum())


def test_multirbm_chunks_equal_the_one_call():
    B, Ti, D, Hn, units, k, M, steps = 10, 4, 24, 40, [64, 32], 4, 3, 9
    intro = dev((np.random.default_rng(28).random((B, Ti, D * M)) < .3).astype(np.uint8))
    gen = multirbm_gen(D, Hn, units, k, M)
    one = gen.generate(intro, steps)
    assert 0.02 < float(one.float().mean()) < 0.98
    assert torch.equal(chunks(gen.session(intro), (4, 1, 4)), one)
    assert gen._det_bias is None


# ------------------------------------------------------------------------------------------------
# 3. given and temperature
def _cond_gen(kind):
    if kind == "nade":
        return nade_gen(1, 24, 32, [64, 32], seed=37)[0], 24, 0.8
    if kind == "multinade":
        return nade_gen(3, 8, 32, [64, 32], seed=37)[0], 24, (0.8, 1.0, 1.3)
    if kind == "rbm":
        return rbm_gen(24, 40, [64, 32], 4)[0], 24, 0.8
    return multirbm_gen(8, 40, [64, 32], 4), 24, (0.8, 1.0, 1.3)


@pytest.mark.parametrize("kind", ["nade", "multinade", "rbm", "multirbm"])
def test_given_and_temperature_per_chunk(monkeypatch, kind):
    gen, n_out, temp = _cond_gen(kind)
    B, Ti, steps, split = 6, 3, 7, (3, 2, 2)
    R = np.random.default_rng(51)
    intro = dev((R.random((B, Ti, n_out)) < .3).astype(np.uint8))
    codes_np = random_codes(R, (B, steps, n_out))
    codes = dev(codes_np)
    clamped = codes != FREE
    for T in (1.0, temp):
        one = gen.generate(intro, steps, given=codes, temperature=T)
        assert torch.equal(one[clamped], codes[clamped])
        got = chunks(gen.session(intro), split, given=codes, temperature=T)         # the block's slices
        assert torch.equal(got, one), (kind, T, int((got != one).sum()))
        # a chunk without `given` between two conditioned ones: the one call with GIVEN_FREE there
        hole_np = codes_np.copy()
        hole_np[:, 3:5] = FREE
        hole = dev(hole_np)
        one_h = gen.generate(intro, steps, given=hole, temperature=T)
        got_h = chunks(gen.session(intro), split, given=[hole[:, :3].contiguous(), None, hole[:, 5:].contiguous()], temperature=T)
        assert torch.equal(got_h, one_h), (kind, T)
        assert not torch.equal(one_h, one)
    # chunk 1 at T = 1, chunk 2 at T = 1.5: the captured session against the eager one
    cap = chunks(gen.session(intro), (3, 4), given=codes, temperature=[1.0, 1.5])
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    eag = chunks(gen.session(intro), (3, 4), given=codes, temperature=[1.0, 1.5])
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    assert torch.equal(cap, eag)
    assert torch.equal(cap[:, :3], gen.generate(intro, 3, given=codes[:, :3].contiguous()))       # (chunk 1 is the one call's beginning)
    assert not torch.equal(cap, gen.generate(intro, 7, given=codes))


# ------------------------------------------------------------------------------------------------
# 4. graph behaviour
@pytest.mark.parametrize("kind", ["nade", "multinade", "rbm"])
def test_captured_session_equals_eager_session(monkeypatch, kind):
    """As test_generate_graph_replay_equals_eager_scan: captured against eager sessions chunk by chunk; four chunks of one length are ONE
    cached graph; a chunk after the weights moved equals the eager chunk with no new capture; two sessions do not disturb each other."""
    from multinn_amd import RnnNade, RnnMultiNADE, RnnRBM
    B, Ti, E, Hn, units, n = 40, 5, 16, 32, [128, 128], 3
    tracks = 3 if kind == "multinade" else 1
    Din = E * tracks
    R = np.random.default_rng(11)
    xa = dev((R.random((B, Ti, Din)) < .3).astype(np.uint8))
    xb = dev((R.random((B, Ti, Din)) < .3).astype(np.uint8))
    if kind == "nade":
        gen = RnnNade(E, Hn, units, precision="bf16", seed=5)
    elif kind == "multinade":
        gen = RnnMultiNADE(E, Hn, units, tracks=ABC, precision="bf16", seed=5)
    else:
        gen = RnnRBM(E, Hn, units, k=3, precision="bf16", seed=5)
    gen._materialize(Din)

    def eager_session(x):
        monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
        s = gen.session(x)
        monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
        return s

    def eager_chunk(s):
        monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
        out = s.generate(n)
        monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
        return out

    sa, sb, ea, eb = gen.session(xa), gen.session(xb), eager_session(xa), eager_session(xb)
    pa, pb = [], []
    for i in range(4):                                             # the two captured sessions interleaved
        ca, cb = sa.generate(n), sb.generate(n)
        assert torch.equal(ca, eager_chunk(ea)) and torch.equal(cb, eager_chunk(eb)), (kind, i)
        pa.append(ca); pb.append(cb)
    assert not torch.equal(torch.cat(pa, 1), torch.cat(pb, 1))      # (two pieces: the rows share their uniforms, not their intros)
    assert len(sa._graphs) == 1 and len(sb._graphs) == 1 and len(ea._graphs) == 0
    assert torch.equal(gen.session(xa).generate(n), gen.generate(xa, n))
    graph = next(iter(sa._graphs.values()))[0]
    gen.store.theta.mul_(1.5)                                      # "training happened": no recapture, the replay re-packs
    gen.store.step += 1
    ca2 = sa.generate(n)
    assert len(sa._graphs) == 1 and next(iter(sa._graphs.values()))[0] is graph
    assert torch.equal(ca2, eager_chunk(ea))
    assert sa.steps == ea.steps == 5 * n


# ------------------------------------------------------------------------------------------------
# 5. state
@pytest.mark.parametrize("kind", ["nade", "rbm"])
def test_snapshot_restore_and_row0(kind):
    B, Ti = 6, 4
    if kind == "nade":
        gen, _ = nade_gen(3, 8, 16, [32, 32])
        n_out = 24
    else:
        gen, _ = rbm_gen(24, 40, [64, 32], 4)
        n_out = 24
    intro = dev((np.random.default_rng(6).random((B, Ti, n_out)) < .3).astype(np.uint8))
    one = gen.generate(intro, 7)
    sess = gen.session(intro)
    a0 = sess.generate(2)
    snap = sess.snapshot()
    a1, a2 = sess.generate(3), sess.generate(2)
    assert sess.steps == 7 and torch.equal(torch.cat([a0, a1, a2], 1), one)
    sess.restore(snap)
    assert sess.steps == 2
    b1, b2 = sess.generate(3), sess.generate(2)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    sess.restore(snap)                                              # redraw the bar hotter: another piece from the same state
    hot = sess.generate(3, temperature=1.5)
    assert sess.steps == 5 and not torch.equal(hot, a1)
    # row-keyed draws: a session on rows 2: with row0 = 2 reproduces them; row0 is read when the session is opened
    gen.row0 = 2
    sub = gen.session(intro[2:].contiguous())
    gen.row0 = 0
    assert torch.equal(chunks(sub, (2, 3, 2)), one[2:])
    assert gen.row0 == 0


@pytest.mark.parametrize("kind", ["nade", "rbm"])
def test_learned_initial_state(kind):
    from multinn_amd import RnnRBM
    B, Ti, steps = 5, 3, 6
    if kind == "nade":
        gen, _ = nade_gen(1, 24, 16, [32, 32], learn_zero_state=True)
    else:
        gen = RnnRBM(24, 40, [64, 32], k=4, precision="fp32", seed=41, learn_zero_state=True)
        gen._materialize(24)
    g = torch.Generator().manual_seed(3)
    for l in range(2):
        c0 = gen.store[f"rnn/cell_{l}/c0"]
        c0.copy_((torch.randn(c0.shape, generator=g) * 0.7).to(DEV))
    intro = dev((np.random.default_rng(8).random((B, Ti, 24)) < .3).astype(np.uint8))
    one = gen.generate(intro, steps)
    assert torch.equal(chunks(gen.session(intro), (1, 2, 3)), one)
    for l in range(2):
        gen.store[f"rnn/cell_{l}/c0"].zero_()
    assert not torch.equal(gen.generate(intro, steps), one)          # (the state mattered)


# ------------------------------------------------------------------------------------------------
# 6. modes
TRACKS = ["Drums", "Piano", "Guitar"]


def make_mode(mode, gen, P=8, M=3, B=4, Ti=3, seed=14):
    from multinn_amd import MultINN
    cfg = {"model_name": "t", "data": {"pitch_range": {"lowest": 0, "highest": P}, "instruments": TRACKS[:M], "beat_resolution": 4},
           "training": {"num_pixels": 1, "random_seed": 23}}
    prm = {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
           "generator": {"type": gen, "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": None, "k": 3}}
    x = (np.random.default_rng(seed).random((B, Ti, P, M)) < 0.3).astype(np.uint8)
    m = MultINN(cfg, prm, mode=mode, precision="fp32")
    m.build(dev(x), lengths=None, is_train=False, mode="generate")
    return m


MODES = [("joint", "NADE"), ("joint", "RBM"), ("jamming", "NADE"), ("jamming", "RBM"), ("composer", "NADE"), ("composer", "MultiRBM")]


@pytest.mark.parametrize("mode,gen", MODES)
def test_mode_sessions(mode, gen):
    m = make_mode(mode, gen)
    B, steps, P, M = 4, 6, 8, 3
    one = m.generate(steps)
    assert one.shape == (B, steps, P, M) and one.dtype == torch.uint8
    sess = m.session()
    got = torch.cat([sess.generate(n) for n in (2, 1, 3)], 1)
    assert sess.steps == steps and torch.equal(got, one), (mode, gen, int((got != one).sum()))
    # conditioned chunks: some cells of every track, the mask sliced with the block
    R = np.random.default_rng(3)
    given = dev((R.random((B, steps, P, M)) < 0.3).astype(np.uint8))
    mask = torch.from_numpy(R.random((B, steps, P, M)) < 0.3)
    cond = m.generate(steps, given=given, given_mask=mask)
    sess = m.session()
    got = torch.cat([sess.generate(b - a, given=given[:, a:b].contiguous(), given_mask=mask[:, a:b]) for a, b in ((0, 2), (2, 3), (3, 6))], 1)
    assert torch.equal(got, cond), (mode, gen)
    assert torch.equal(got[mask.to(DEV)], given[mask.to(DEV)])
    snap = sess.snapshot()
    nxt = sess.generate(2)
    sess.restore(snap)
    assert sess.steps == steps and torch.equal(sess.generate(2), nxt)


@pytest.mark.parametrize("gen", ["NADE", "RBM"])
def test_jamming_track_given_whole_in_one_chunk_and_free_in_the_next(gen):
    m = make_mode("jamming", gen)
    B, steps, P, M = 4, 6, 8, 3
    given = dev((np.random.default_rng(4).random((B, steps, P, M)) < 0.3).astype(np.uint8))
    mask = torch.zeros((B, steps, P, M), dtype=torch.bool)
    mask[:, :3, :, 0] = True                                        # track 0: the human part for the first chunk, then the model's
    one = m.generate(steps, given=given, given_mask=mask)
    sess = m.session()
    c1 = sess.generate(3, given=given[:, :3].contiguous(), given_mask=torch.tensor([True, False, False]))
    c2 = sess.generate(3)
    got = torch.cat([c1, c2], 1)
    assert torch.equal(got, one), int((got != one).sum())
    assert torch.equal(got[:, :3, :, 0], given[:, :3, :, 0])


# ------------------------------------------------------------------------------------------------
# 7. the draw position is a value (common.DrawAt): a session sets nothing on its generator, and the generator's seed / row0 do not reach it
def _position_case(kind):
    """nade: a byte intro (the one-call chunks); nade_float: the same generator on a float intro (the step loop); rbm: the step loop, k = 4."""
    if kind == "rbm":
        B, Ti, D, steps = 10, 4, 24, 9
        gen, _ = rbm_gen(D, 40, [64, 32], 4)
        return gen, dev((np.random.default_rng(26).random((B, Ti, D)) < .3).astype(np.uint8)), steps, (4, 1, 4)
    B, Ti, E, steps = 5, 4, 8, 6
    gen, _ = nade_gen(1, E, 16, [32, 32])
    x = dev((np.random.default_rng(6).random((B, Ti, E)) < .3).astype(np.uint8))
    return gen, (x.float() if kind == "nade_float" else x), steps, (1, 2, 3)


@pytest.mark.parametrize("graph", ["captured", "eager"])
@pytest.mark.parametrize("kind", ["nade", "nade_float", "rbm"])
def test_session_and_generator_are_independent(monkeypatch, kind, graph):
    if graph == "eager":
        monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    gen, x, steps, split = _position_case(kind)
    one = gen.generate(x, steps)
    sess = gen.session(x)
    assert sess._scan == (kind == "nade")
    mine = (gen.seed + 5, gen.row0 + 3)
    gen.seed, gen.row0 = mine                                       # after the opening: the session keeps the opening's
    other = gen.generate(x, steps)
    assert not torch.equal(other, one)

    def untouched():
        return (gen.seed, gen.row0) == mine and not any(a.startswith("_gen_") for a in dir(gen))
    out = []
    for i, n in enumerate(split):
        if i == 1:                                                  # a chunk that raises leaves the generator, and the session, as they were
            with pytest.raises(ValueError, match="given"):
                sess.generate(n, given=torch.zeros((1, n, 1), dtype=torch.uint8, device=DEV))
            assert untouched() and sess.steps == sum(split[:1])
        out.append(sess.generate(n))
        assert untouched()
    assert torch.equal(torch.cat(out, 1), one)                      # the opening seed / row0
    assert torch.equal(gen.generate(x, steps), other)               # the generator's own, with a session in between
    gen.seed, gen.row0 = mine[0] - 5, mine[1] - 3
    assert torch.equal(gen.generate(x, steps), one)


@pytest.mark.parametrize("kind", ["nade", "rbm"])
def test_sample_single_at_a_position(kind):
    from multinn_amd.common import DrawAt
    gen, x, steps, _ = _position_case(kind)
    one = gen.generate(x, steps)
    out, state, last = gen._scan_steps(gen.steps(x), x[:, -1, :], 3, DrawAt(gen.seed, gen.row0, 0))
    assert torch.equal(out, one[:, :3])
    row, _ = gen.sample_single(last, state, at=DrawAt(gen.seed, gen.row0, 3))
    assert torch.equal(row, one[:, 3])
    seed, row0 = gen.seed, gen.row0
    gen.seed, gen.row0 = seed + 1, row0 + 1                          # the position comes from `at` and from nothing else
    assert torch.equal(gen.sample_single(last, state, at=DrawAt(seed, row0, 3))[0], row)
    assert not torch.equal(gen.sample_single(last, state)[0], row)   # at=None: the generator's own seed and row0, step 0
