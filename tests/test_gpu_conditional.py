"""Conditional generation on the device: sampling kernels with clamped visibles (SampleJob.given) against the deterministic checker, the
kernel forms against one another, the one-call scan, the captured scans and the mode classes.

The checker needs no change: a clamped visible leaves its uniform unused, so det.nade_sample with u = -1 where the given value is 1 and
u = 2 where it is 0 (u < p, p in [0, 1]) is the clamped draw, and every free visible reads the uniform of the unconditioned scan."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nade as onade, philox, det, generators as G   # noqa: E402

DEV = "cuda:0"
FREE = 255


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


def clamp_u(u, codes):
    """The uniforms that make det.nade_sample emit the clamped values."""
    return np.where(codes == 1, np.float32(-1.0), np.where(codes == 0, np.float32(2.0), u)).astype(np.float32)


def random_codes(R, shape, density):
    vals = (R.random(shape) < 0.3).astype(np.uint8)
    return np.where(R.random(shape) < density, vals, FREE).astype(np.uint8)


def load_nade_params(gen, p):
    s = gen.store
    for l, (W, b) in enumerate(p['lstm']):
        s[f"rnn/cell_{l}/kernel"].copy_(dev(W.astype(np.float32)))
        s[f"rnn/cell_{l}/bias"].copy_(dev(b.astype(np.float32)))
    s["nade/w_enc"].copy_(dev(np.stack(p['w_enc']).astype(np.float32)))
    s["nade/w_dec"].copy_(dev(np.stack(p['w_dec']).astype(np.float32)))
    s["dense/kernel"].copy_(dev(p['fc_k'].astype(np.float32)))
    s["dense/bias"].copy_(dev(p['fc_b'].astype(np.float32)))
    gen._packed_step = -1


# ------------------------------------------------------------------------------------------------
# 1. kernels vs the checker
@pytest.mark.parametrize("N,D,Hn,tracks", [(3, 61, 30, 2),          # Hn % 4 != 0: the visible-at-a-time kernel
                                           (4, 7, 256, 2),          # D < one chunk
                                           (5, 333, 256, 3),        # chunks, track offsets and Philox windows that do not line up
                                           (300, 24, 256, 1),       # more rows than CUs: chunks of 8
                                           (72, 440, 256, 1)])      # the joint shape at 72 rows: chunks of 16
@pytest.mark.parametrize("temp", [1.0, 0.7])
@pytest.mark.parametrize("kind", ["density 0.3", "density 1.0", "whole track", "track minor"])
def test_clamped_sample_bit_exact(ops, N, D, Hn, tracks, temp, kind):
    R = np.random.default_rng(N * 31 + D)
    ld = tracks * (Hn + D)
    bias = (R.standard_normal((N, ld)) * .5).astype(np.float32)
    we = (R.standard_normal((tracks, D, Hn)) * .3).astype(np.float32)
    wd = (R.standard_normal((tracks, D, Hn)) * .3).astype(np.float32)
    if kind == "whole track":
        codes = np.full((N, tracks, D), FREE, np.uint8)               # track 0 wholly given (with one track: every visible)
        codes[:, 0] = (R.random((N, D)) < 0.3).astype(np.uint8)
    else:
        codes = random_codes(R, (N, tracks, D), 1.0 if kind == "density 1.0" else 0.3)
    minor = kind == "track minor"
    lay = (lambda a: a.transpose(0, 2, 1).reshape(N, tracks * D)) if minor else (lambda a: a.reshape(N, tracks * D))
    out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
    nll = torch.zeros((tracks, N), device=DEV)
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, temp, seed=77, row0=1000, sub=5, samples=out, nll=nll,
                    track_minor=minor, given=dev(lay(codes)))
    got = out.cpu().numpy()
    got = got.reshape(N, D, tracks).transpose(0, 2, 1) if minor else got.reshape(N, tracks, D)
    u = philox.uniform_block(77, philox.STREAM_NADE, np.arange(1000, 1000 + N), 5, tracks * D)
    for m in range(tracks):
        s_ref, p_ref = det.nade_sample(bias, we[m], wd[m], tracks, m, D, Hn, temp, clamp_u(u[:, m * D:(m + 1) * D], codes[:, m]))
        assert np.array_equal(got[:, m], s_ref), "draws must be bit-exact"
        given = codes[:, m] != FREE
        assert np.array_equal(got[:, m][given], codes[:, m][given])
        # nll of the emitted vector: -sum log(1e-6 + p(emitted value)) with the checker's f32 conditionals -- 1 - p in f32 as in the
        # unconditioned kernels (a visible clamped to 0 against p ~ 1 - 1e-6 makes that term's f32 rounding visible in the sum)
        q = np.where(s_ref > 0, p_ref, np.float32(1.0) - p_ref).astype(np.float64)
        assert rel(nll[m].cpu().numpy(), -np.log(1e-6 + q).sum(1)) < 1e-5
        # and the float64 oracle of the emitted vector
        be = bias[:, m * Hn:(m + 1) * Hn].astype(np.float64)
        bd = bias[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D].astype(np.float64)
        n64, _ = onade.log_prob(s_ref.astype(np.float64), be, bd, we[m].astype(np.float64), wd[m].astype(np.float64))
        assert rel(nll[m].cpu().numpy(), n64) < 2e-4


# 2. the kernel forms agree with given
@pytest.mark.parametrize("scale", [0.3, 3.0])
def test_clamped_sample_kernel_forms_agree(ops, monkeypatch, scale):
    N, D, Hn, tracks = 40, 440, 256, 2
    g = torch.Generator(device=DEV).manual_seed(5)
    ld = tracks * (Hn + D)
    bias = torch.randn((N, ld), device=DEV, generator=g) * 0.5
    if scale < 1:
        bias[:, tracks * Hn:] -= 3.5
    we = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1 * scale
    wd = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1 * scale
    codes = torch.from_numpy(random_codes(np.random.default_rng(3), (N, tracks * D), 0.4)).to(DEV)
    for temp in (1.0, 0.8, None):
        res = []
        for form in ("chunks of 16", "chunks of 8", "visible at a time", "no speculation"):
            for k in ("MNN_SAMPLE_NO_CHUNK", "MNN_SAMPLE_G8", "MNN_SAMPLE_NO_SPEC"):
                monkeypatch.delenv(k, raising=False)
            if form == "chunks of 8":
                monkeypatch.setenv("MNN_SAMPLE_G8", "1")
            elif form == "visible at a time":
                monkeypatch.setenv("MNN_SAMPLE_NO_CHUNK", "1")
            elif form == "no speculation":
                monkeypatch.setenv("MNN_SAMPLE_NO_CHUNK", "1")
                monkeypatch.setenv("MNN_SAMPLE_NO_SPEC", "1")
            out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
            nll = torch.zeros((tracks, N), device=DEV)
            ops.nade_sample(bias, we, wd, tracks, D, Hn, temp, 9, 0, 3, out, nll=nll, given=codes)
            res.append((out, nll))
        for out, nll in res[1:]:
            assert torch.equal(out, res[0][0]) and torch.equal(nll, res[0][1]), temp
        assert torch.equal(res[0][0][codes != FREE], codes[codes != FREE])
    for k in ("MNN_SAMPLE_NO_CHUNK", "MNN_SAMPLE_G8", "MNN_SAMPLE_NO_SPEC"):
        monkeypatch.delenv(k, raising=False)


# 3. invariants
@pytest.mark.parametrize("N,D,Hn,tracks", [(40, 440, 256, 2), (3, 61, 30, 2), (300, 24, 256, 1)])
@pytest.mark.parametrize("temp", [1.0, 0.7, None])
def test_clamped_sample_invariants(ops, N, D, Hn, tracks, temp):
    g = torch.Generator(device=DEV).manual_seed(N + D)
    bias = torch.randn((N, tracks * (Hn + D)), device=DEV, generator=g) * 0.5
    we = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.3
    wd = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.3

    def run(given):
        out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
        nll = torch.zeros((tracks, N), device=DEV)
        ops.nade_sample(bias, we, wd, tracks, D, Hn, temp, 4, 7, 2, out, nll=nll, given=given)
        return out, nll

    base, bnll = run(None)
    out, nll = run(torch.full_like(base, FREE))                            # every visible free: the unconditioned bits
    assert torch.equal(out, base) and torch.equal(nll, bnll)
    out, nll = run(base.clone())                                           # clamped to the unconditioned output: the same bits
    assert torch.equal(out, base) and torch.equal(nll, bnll)
    half = torch.rand(base.shape, device=DEV, generator=g) < 0.5
    out, nll = run(torch.where(half, base, torch.full_like(base, FREE)))
    assert torch.equal(out, base) and torch.equal(nll, bnll)


# 4. several generators in one launch
def test_clamped_sample_multi_equals_separate_calls(ops):
    B, P, M, Hn = 6, 40, 4, 64
    g = torch.Generator(device=DEV).manual_seed(11)
    jobs, refs = [], []
    out = torch.zeros((B, P, M), device=DEV, dtype=torch.uint8)
    codes = torch.from_numpy(random_codes(np.random.default_rng(2), (B, P, M), 0.5)).to(DEV)
    for m in range(M):
        bias = torch.randn((B, Hn + P + 8), device=DEV, generator=g)[:, :Hn + P]
        we = torch.randn((1, P, Hn), device=DEV, generator=g) * 0.3
        wd = torch.randn((1, P, Hn), device=DEV, generator=g) * 0.3
        gv = codes[:, :, m] if m % 2 == 0 else None                       # some jobs clamped, some free
        nll = torch.zeros(B, device=DEV)
        jobs.append(dict(bias=bias, w_enc=we[0], w_dec=wd[0], seed=100 + m, samples=out[:, :, m], nll=nll, given=gv))
        ref = torch.zeros((B, P), device=DEV, dtype=torch.uint8)
        rnll = torch.zeros((1, B), device=DEV)
        ops.nade_sample(bias.contiguous(), we, wd, 1, P, Hn, 1.0, 100 + m, 0, 3, ref, nll=rnll, given=None if gv is None else gv.contiguous())
        refs.append((ref, rnll[0]))
    ops.nade_sample_multi(jobs, P, Hn, 1.0, 0, 3)
    for m in range(M):
        assert torch.equal(out[:, :, m], refs[m][0]) and torch.equal(jobs[m]["nll"], refs[m][1]), m


# ------------------------------------------------------------------------------------------------
# 5. the one-call scan
def clamped_rnn_nade_generate(intro, num_steps, p, seed, codes, tracks=1):
    """det.rnn_nade_generate with clamped visibles: codes u8 [B, num_steps, tracks * D] in the sample layout."""
    B, Ti, _ = intro.shape
    D, Hn = p['w_enc'][0].shape
    state, h = None, None
    for t in range(Ti):
        h, state = det.lstm_step(intro[:, t], state, p['lstm'])
    out = det.dense(h, p['fc_k'], p['fc_b'])
    rows = np.arange(B, dtype=np.uint32)
    samples = np.empty((B, num_steps, tracks * D), np.uint8)
    for s in range(num_steps):
        u = philox.uniform_block(seed, philox.STREAM_NADE, rows, s, tracks * D)
        c = codes[:, s] if tracks == 1 else codes[:, s].reshape(B, D, tracks).transpose(0, 2, 1).reshape(B, tracks * D)   # -> m D + i
        per = [det.nade_sample(out, p['w_enc'][m], p['w_dec'][m], tracks, m, D, Hn, 1.0,
                               clamp_u(u[:, m * D:(m + 1) * D], c[:, m * D:(m + 1) * D]))[0] for m in range(tracks)]
        step = per[0] if tracks == 1 else np.stack(per, axis=2).reshape(B, tracks * D)
        samples[:, s] = step
        h, state = det.lstm_step(step, state, p['lstm'])
        out = det.dense(h, p['fc_k'], p['fc_b'])
    return samples


@pytest.mark.parametrize("tracks", [1, 3])
def test_generate_scan_with_given(ops, monkeypatch, tracks):
    from multinn_amd import RnnNade, RnnMultiNADE
    B, Ti, E, Hn, units, steps = 5, 4, 24, 32, [32, 32], 7
    Din = E * tracks
    R = np.random.default_rng(60 + tracks)
    intro = (R.random((B, Ti, Din)) < .3).astype(np.uint8)
    p = G.init_rnn_nade(9, Din, E, Hn, units, np.float64, tracks=tracks)
    gen = RnnNade(E, Hn, units, precision="fp32", seed=31) if tracks == 1 else \
        RnnMultiNADE(E, Hn, units, tracks=list("abc"), precision="fp32", seed=31)
    gen._materialize(Din)
    load_nade_params(gen, p)
    codes = random_codes(R, (B, steps, Din), 0.4)
    ref = clamped_rnn_nade_generate(intro, steps, p, 31, codes, tracks)
    # the entry point itself
    got = gen._scan_in_one_call(dev(intro), steps, dev(codes))
    assert np.array_equal(got.cpu().numpy(), ref)
    # the captured scan, and the eager one
    out = gen.generate(dev(intro), steps, given=dev(codes))
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(out.cpu().numpy()[codes != FREE], codes[codes != FREE])
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(dev(intro), steps, given=dev(codes)), out)
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    # a second given of the same shape replays the same graph, with its own output
    n_graphs = len(gen._scan_graphs._cache)
    codes2 = random_codes(R, (B, steps, Din), 0.6)
    out2 = gen.generate(dev(intro), steps, given=dev(codes2))
    assert len(gen._scan_graphs._cache) == n_graphs
    assert np.array_equal(out2.cpu().numpy(), clamped_rnn_nade_generate(intro, steps, p, 31, codes2, tracks))
    # the unconditioned scan is unchanged, and has its own graph
    plain = gen.generate(dev(intro), steps)
    assert np.array_equal(plain.cpu().numpy(), det.rnn_nade_generate(intro, steps, p, 31, tracks=tracks))
    # the step-by-step path (float intro: sample_single with given) gives the same bits
    assert torch.equal(gen.generate(dev(intro).float(), steps, given=dev(codes)), out)


# ------------------------------------------------------------------------------------------------
# 6. the mode classes
TRACKS = ["Drums", "Piano", "Guitar"]


def mode_config(P, tracks):
    return {"model_name": "t", "data": {"pitch_range": {"lowest": 0, "highest": P}, "instruments": list(tracks), "beat_resolution": 4},
            "training": {"num_pixels": 1, "random_seed": 23}}


def mode_params(mode, gen="NADE", Hn=16, units=(32, 32), feedback=None):
    return {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
            "generator": {"type": gen, "num_hidden": Hn, "num_hidden_rnn": list(units), "feedback": feedback}}


def make_mode(mode, gen="NADE", P=8, M=3, B=4, Ti=3, seed=14):
    from multinn_amd import MultINN
    x = (np.random.default_rng(seed).random((B, Ti, P, M)) < 0.3).astype(np.uint8)
    fb = [64, 32] if mode == "feedback-rnn" else ([32] if mode == "feedback" else None)
    m = MultINN(mode_config(P, TRACKS[:M]), mode_params(mode, gen=gen, feedback=fb), mode=mode, precision="fp32")
    m.build(dev(x), lengths=None, is_train=False, mode="generate")
    return m, x


@pytest.mark.parametrize("mode", ["joint", "composer", "jamming", "feedback", "feedback-rnn"])
def test_mode_conditional_generation(mode):
    m, x = make_mode(mode)
    steps = 5
    base = m.generate(steps)
    assert torch.equal(base, m.generate(steps))
    B, _, P, M = base.shape
    R = np.random.default_rng(7)
    given = dev((R.random((B, steps, P, M)) < 0.3).astype(np.uint8))
    for mask in (torch.tensor([False, True, False]), torch.from_numpy(R.random((P, M)) < 0.5), torch.from_numpy(R.random((B, steps, P, M)) < 0.4)):
        out = m.generate(steps, given=given, given_mask=mask)
        full = mask.to(DEV).expand(B, steps, P, M)
        assert torch.equal(out[full], given[full]), mode
    # no given: today's bits
    assert torch.equal(m.generate(steps), base)
    # one whole track clamped to its unconditioned output: the whole unconditioned output
    for i in range(M):
        mask = torch.zeros(M, dtype=torch.bool)
        mask[i] = True
        assert torch.equal(m.generate(steps, given=base, given_mask=mask), base), (mode, i)
    # the sampler passes them through
    d = m._config["data"]
    beats = 1
    n = beats * d["beat_resolution"] * (d["pitch_range"]["highest"] - d["pitch_range"]["lowest"]) // m._num_dims
    g2 = dev((R.random((B, n, P, M)) < 0.3).astype(np.uint8))
    assert torch.equal(m.sampler(beats, given=g2, given_mask=torch.tensor([True, False, False]))[..., 0], g2[..., 0])


def test_feedback_grouped_scan_with_given_bit_exact():
    """The grouped NADE path of the feedback scan (nade_sample_multi with given views) against a clamped restatement of
    det.feedback_rnn_generate."""
    from multinn_amd import MultINN
    P, M, Hn, units, fb_units, B, Ti, steps = 8, 3, 16, [32, 32], [64, 32], 4, 3, 6
    x = (np.random.default_rng(14).random((B, Ti, P, M)) < 0.3).astype(np.uint8)
    m = MultINN(mode_config(P, TRACKS[:M]), mode_params("feedback-rnn", Hn=Hn, units=units, feedback=fb_units), mode="feedback-rnn",
                precision="fp32")
    m.build(dev(x), lengths=None, is_train=False, mode="generate")
    gparams = []
    for i, g in enumerate(m.generators):
        p = G.init_rnn_nade(60 + i, P + fb_units[-1], P, Hn, units, np.float64)
        p['fc_b'][Hn:] = np.log(0.15 / 0.85)
        load_nade_params(g, p)
        gparams.append(p)
    fb = m._feedback_layer
    fb_layers = [(fb.store[f"feedback/rnn/cell_{l}/kernel"].cpu().numpy().astype(np.float64),
                  fb.store[f"feedback/rnn/cell_{l}/bias"].cpu().numpy().astype(np.float64)) for l in range(len(fb_units))]
    seeds = [g.seed for g in m.generators]
    R = np.random.default_rng(8)
    given = (R.random((B, steps, P, M)) < 0.3).astype(np.uint8)
    mask = R.random((B, steps, P, M)) < 0.4
    mask[..., 1] = True                                                   # track 1 wholly given, the others in part
    out = m.generate(steps, given=dev(given), given_mask=torch.from_numpy(mask)).cpu().numpy()
    codes = np.where(mask, given, FREE).astype(np.uint8)
    # clamped restatement of det.feedback_rnn_generate
    enc = np.concatenate([np.zeros((B, 1, P, M), np.float32), x.astype(np.float32)], axis=1)
    stack = enc.reshape(B, Ti + 1, P * M)
    fb_state, states, hs = None, [None] * M, [None] * M
    for t in range(Ti + 1):
        f, fb_state = det.lstm_step(stack[:, t], fb_state, fb_layers)
        for i, p in enumerate(gparams):
            hs[i], states[i] = det.lstm_step(np.concatenate([enc[:, t, :, i], f], 1), states[i], p['lstm'])
    outs = [det.dense(hs[i], p['fc_k'], p['fc_b']) for i, p in enumerate(gparams)]
    rows = np.arange(B, dtype=np.uint32)
    ref = np.empty((B, steps, P, M), np.uint8)
    for s in range(steps):
        cur = []
        for i, p in enumerate(gparams):
            u = clamp_u(philox.uniform_block(seeds[i], philox.STREAM_NADE, rows, s, P), codes[:, s, :, i])
            cur.append(det.nade_sample(outs[i], p['w_enc'][0], p['w_dec'][0], 1, 0, P, Hn, 1.0, u)[0])
        st = np.stack(cur, -1)
        ref[:, s] = st
        f, fb_state = det.lstm_step(st.reshape(B, P * M), fb_state, fb_layers)
        for i, p in enumerate(gparams):
            hs[i], states[i] = det.lstm_step(np.concatenate([cur[i].astype(np.float32), f], 1), states[i], p['lstm'])
            outs[i] = det.dense(hs[i], p['fc_k'], p['fc_b'])
    assert np.array_equal(out, ref)
    assert np.array_equal(out[mask], given[mask])


def test_jamming_rbm_generators_whole_given_track():
    m, x = make_mode("jamming", gen="RBM")
    steps = 4
    base = m.generate(steps)
    B, _, P, M = base.shape
    given = dev((np.random.default_rng(3).random((B, steps, P, M)) < 0.3).astype(np.uint8))
    out = m.generate(steps, given=given, given_mask=torch.tensor([False, False, True]))
    assert torch.equal(out[..., 2], given[..., 2])
    assert torch.equal(out[..., :2], base[..., :2])
