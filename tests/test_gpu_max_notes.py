"""The polyphony cap on the device: the capped NADE sampling kernels against the unchanged deterministic checker, the kernel forms against
one another, the identities that make `max_notes=None` today's call, and generate / sample_single_capped / sessions / the mode classes.

The checker needs no change.  A capped visible, like a clamped one, leaves its uniform unused, so det.nade_sample with u = 2 (u < p is false
for every p in [0, 1]) on the free visibles behind a track's cap event is the capped draw.  Where the event lies depends on the draws in
front of it, so the reference is built in rounds: run the checker, settle per row the EARLIEST cap event among the counters not yet settled
(nothing in front of it can change any more), force that counter's later free visibles to 0, run again.  Every round settles one counter of
a row: at most (counters + 1) rounds, two for a track of a MultiNADE.
Threshold decoding (temperature None) ignores the uniforms in the checker, so nothing could be forced there; the same decision is written as
a draw at temperature 1 with u = the largest float below 0.5 on every undecided visible -- u < p is then p >= 0.5 exactly (p is a float32:
p > pred(0.5) and p >= 0.5 are the same set) -- and the uncapped, unclamped case is checked against the checker's own threshold mode."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nade as onade, philox, det, generators as G   # noqa: E402
import test_gpu_conditional as TN                                  # noqa: E402

DEV = "cuda:0"
FREE = 255
F = np.float32
BELOW_HALF = np.nextafter(F(0.5), F(0.0))
dev, rel = TN.dev, TN.rel


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


# ------------------------------------------------------------------------------------------------
# the reference
def checker(bias, we, wd, tracks, m, D, Hn, temp, u):
    """det.nade_sample; threshold decoding as the temperature-1 draw with u = pred(0.5) already written into the undecided visibles of u."""
    return det.nade_sample(bias, we, wd, tracks, m, D, Hn, 1.0 if temp is None else temp, u)


def capped_reference(bias, we, wd, tracks, m, D, Hn, temp, u, codes, counter, caps):
    """One NADE scan (track m of `tracks`) under caps -> (samples, conditionals, rounds).  u [N, D]: the scan's Philox uniforms; codes [N, D];
    counter [D]: the counter a visible counts in; caps: per counter an int or None."""
    N = bias.shape[0]
    free = codes == FREE
    uu = TN.clamp_u(np.full_like(u, BELOW_HALF) if temp is None else u, codes)
    settled = np.zeros((N, len(caps)), bool)
    for c, k in enumerate(caps):
        if k is None:
            settled[:, c] = True
        elif k == 0:                                                # exhausted from the start: no draw in front of the event
            uu[:, counter == c] = np.where(free[:, counter == c], F(2.0), uu[:, counter == c])
            settled[:, c] = True
    rounds = 0
    while True:
        s, p = checker(bias, we, wd, tracks, m, D, Hn, temp, uu)
        rounds += 1
        changed = False
        for n in range(N):
            best = None
            for c in np.flatnonzero(~settled[n]):
                idx = np.flatnonzero(counter == c)
                hit = np.flatnonzero(np.cumsum(s[n, idx]) >= caps[c])
                if hit.size and (best is None or idx[hit[0]] < best[0]):
                    best = (idx[hit[0]], c)
            if best is not None:
                pos, c = best
                uu[n, (counter == c) & (np.arange(D) > pos) & free[n]] = F(2.0)
                settled[n, c] = True
                changed = True
        if not changed:
            return s, p, rounds


def problem(N, D, Hn, tracks):
    """Bias scale 0.5 and weight scale 0.3, as in the clamped tests: about D / 2 ones per row.  (The seed is one at which the condition at the
    end of test_capped_sample_bit_exact -- a property of the checker's outputs alone -- holds in every case: at 4 rows of 7 visibles a cap of
    3 binds on about half of the rows, and the plainest seed leaves it binding on one.)"""
    R = np.random.default_rng(N * 31 + D + 3)
    bias = (R.standard_normal((N, tracks * (Hn + D))) * .5).astype(F)
    we = (R.standard_normal((tracks, D, Hn)) * .3).astype(F)
    wd = (R.standard_normal((tracks, D, Hn)) * .3).astype(F)
    codes = TN.random_codes(R, (N, tracks, D), 0.3)
    codes[0, :, :min(D, 6)] = 1                                     # a row whose given ones alone pass every cap of the cases below
    u = philox.uniform_block(77, philox.STREAM_NADE, np.arange(1000, 1000 + N), 5, tracks * D)
    return bias, we, wd, codes, u


@functools.lru_cache(maxsize=None)
def uncapped_reference(N, D, Hn, tracks, temp, with_given):
    """The checker's scan without caps, per track (computed once per shape / temperature / codes, shared by the cases)."""
    bias, we, wd, codes, u = problem(N, D, Hn, tracks)
    out = []
    for m in range(tracks):
        c = codes[:, m] if with_given else np.full((N, D), FREE, np.uint8)
        um = u[:, m * D:(m + 1) * D]
        s = checker(bias, we[m], wd[m], tracks, m, D, Hn, temp, TN.clamp_u(np.full_like(um, BELOW_HALF) if temp is None else um, c))[0]
        if temp is None and not with_given:                         # the rewriting of the threshold mode is the checker's threshold mode
            assert np.array_equal(s, det.nade_sample(bias, we[m], wd[m], tracks, m, D, Hn, None, um)[0])
        out.append(s)
    return out


PER_TRACK = [(3, 61, 30, 2), (4, 7, 256, 2), (5, 333, 256, 3), (300, 24, 256, 1), (72, 440, 256, 1)]
TABLE = (1, None, 2, 0, 4)
# (N, D, Hn, tracks, max_notes, by_visible): Hn % 4 != 0 is the visible-at-a-time kernel; D = 7 lies below one chunk; 333 x 3: chunks, track
# offsets and Philox windows that do not line up; 300 rows: chunks of 8; 72 rows: chunks of 16
CASES = [(*shape, cap, False) for shape in PER_TRACK for cap in (1, 3)] + [(5, 333, 256, 3, (0, 2, None), False)] + \
        [(72, 440, 256, 1, TABLE, True), (72, 7, 256, 1, TABLE, True)]


# 1. kernels vs the checker
@pytest.mark.parametrize("with_given", [False, True], ids=["free", "given"])
@pytest.mark.parametrize("temp", [1.0, 0.7, None])
@pytest.mark.parametrize("N,D,Hn,tracks,cap,by_visible", CASES)
def test_capped_sample_bit_exact(ops, N, D, Hn, tracks, cap, by_visible, temp, with_given):
    bias, we, wd, codes, u = problem(N, D, Hn, tracks)
    if not with_given:
        codes = np.full_like(codes, FREE)
    out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
    nll = torch.zeros((tracks, N), device=DEV)
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, temp, seed=77, row0=1000, sub=5, samples=out, nll=nll,
                    given=dev(codes.reshape(N, tracks * D)) if with_given else None, by_visible=by_visible, max_notes=cap)
    got = out.cpu().numpy().reshape(N, tracks, D)
    plain = uncapped_reference(N, D, Hn, tracks, temp, with_given)
    differs = np.zeros(N, bool)
    for m in range(tracks):
        if by_visible:
            counter, caps = np.arange(D) % len(cap), list(cap)
        else:
            counter, caps = np.zeros(D, int), [cap[m] if isinstance(cap, tuple) else cap]
        s_ref, p_ref, rounds = capped_reference(bias, we[m], wd[m], tracks, m, D, Hn, temp, u[:, m * D:(m + 1) * D], codes[:, m], counter, caps)
        assert rounds <= len(caps) + 1
        differs |= (s_ref != plain[m]).any(1)
        assert np.array_equal(got[:, m], s_ref), "draws must be bit-exact"
        given = codes[:, m] != FREE
        assert np.array_equal(got[:, m][given], codes[:, m][given]), "a given cell always wins"
        for c, k in enumerate(caps):                                # the free ones of a counter stay within its cap
            if k is not None:
                assert ((got[:, m] * ~given)[:, counter == c].sum(1) <= k).all()
        # nll of the emitted vector: the checker's f32 conditionals (capped visibles keep their logit), and the float64 oracle
        q = np.where(s_ref > 0, p_ref, F(1.0) - p_ref).astype(np.float64)
        assert rel(nll[m].cpu().numpy(), -np.log(1e-6 + q).sum(1)) < 1e-5
        be = bias[:, m * Hn:(m + 1) * Hn].astype(np.float64)
        bd = bias[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D].astype(np.float64)
        n64, _ = onade.log_prob(s_ref.astype(np.float64), be, bd, we[m].astype(np.float64), wd[m].astype(np.float64))
        assert rel(nll[m].cpu().numpy(), n64) < 2e-4
    # against a vacuous test, on the checker's two outputs: the cap changes at least half of the rows
    assert differs.sum() * 2 >= N, f"the cap changed {int(differs.sum())} of {N} rows"


# 2. the kernel forms agree under a cap and codes
@pytest.mark.parametrize("tracks,cap,by_visible", [(2, (3, 60), False), (2, 20, False), (1, TABLE, True)])
def test_capped_sample_kernel_forms_agree(ops, monkeypatch, tracks, cap, by_visible):
    N, D, Hn = 40, 440, 256
    g = torch.Generator(device=DEV).manual_seed(5)
    bias = torch.randn((N, tracks * (Hn + D)), device=DEV, generator=g) * 0.5      # about D / 2 ones at any temperature and in threshold decoding:
    we = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1               # a cap of 60 is reached somewhere in the middle of a row
    wd = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1
    codes = torch.from_numpy(TN.random_codes(np.random.default_rng(3), (N, tracks * D), 0.4)).to(DEV)
    keys = ("MNN_SAMPLE_NO_CHUNK", "MNN_SAMPLE_G8", "MNN_SAMPLE_NO_SPEC")
    for temp in (1.0, 0.8, None):
        res = []
        for form in ({}, {"MNN_SAMPLE_G8": "1"}, {"MNN_SAMPLE_NO_CHUNK": "1"}, {"MNN_SAMPLE_NO_CHUNK": "1", "MNN_SAMPLE_NO_SPEC": "1"}):
            for k in keys:                                          # chunks of 16 | chunks of 8 | visible at a time | no speculation
                monkeypatch.delenv(k, raising=False)
            for k, v in form.items():
                monkeypatch.setenv(k, v)
            out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
            nll = torch.zeros((tracks, N), device=DEV)
            ops.nade_sample(bias, we, wd, tracks, D, Hn, temp, 9, 0, 3, out, nll=nll, given=codes, by_visible=by_visible, max_notes=cap)
            res.append((out, nll))
        for out, nll in res[1:]:
            assert torch.equal(out, res[0][0]) and torch.equal(nll, res[0][1]), temp
        assert torch.equal(res[0][0][codes != FREE], codes[codes != FREE])
        plain = torch.zeros_like(res[0][0])
        ops.nade_sample(bias, we, wd, tracks, D, Hn, temp, 9, 0, 3, plain, given=codes, by_visible=by_visible)
        assert not torch.equal(plain, res[0][0]), "the cap must bind"
    for k in keys:
        monkeypatch.delenv(k, raising=False)


# 3. identity
@pytest.mark.parametrize("N,D,Hn,tracks", [(40, 440, 256, 2), (3, 61, 30, 2), (300, 64, 256, 1)])
@pytest.mark.parametrize("temp", [1.0, 0.7, None])
def test_caps_that_do_not_bind_return_the_uncapped_bits(ops, N, D, Hn, tracks, temp):
    g = torch.Generator(device=DEV).manual_seed(N + D)
    bias = torch.randn((N, tracks * (Hn + D)), device=DEV, generator=g) * 0.5
    we = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.3
    wd = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.3
    codes = torch.from_numpy(TN.random_codes(np.random.default_rng(N), (N, tracks * D), 0.2)).to(DEV)

    def run(b, given, **kw):
        out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
        nll = torch.zeros((tracks, N), device=DEV)
        ops.nade_sample(b, we, wd, tracks, D, Hn, temp, 4, 7, 2, out, nll=nll, given=given, **kw)
        return out, nll

    for given in (None, codes):
        base = run(bias, given)
        for cap in (D, D + 9, (None,) * tracks, (D,) + (None,) * (tracks - 1)):     # the launch without caps
            got = run(bias, given, max_notes=cap)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), cap
    # a cap below D that no row reaches: the capped kernels, the uncapped bits (every drawn visible reads the uniform of the uncapped scan)
    low = bias.clone()
    low[:, tracks * Hn:] -= 6.0
    base = run(low, None)
    assert int(base[0].reshape(N, tracks, D).sum(2).max()) < 50 <= D
    got = run(low, None, max_notes=50)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    if tracks == 1:
        got = run(low, None, max_notes=(50, None, 50, 50), by_visible=True)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


# ------------------------------------------------------------------------------------------------
# 4. end to end, at small models
B, TI, STEPS, P, M, HN, UNITS = 3, 4, 6, 12, 3, 32, (32, 32)
CAPS = (1, None, 0)


def nade_generator(tracks, seed=31):
    from multinn_amd import RnnNade, RnnMultiNADE
    E = P if tracks > 1 else P * M                                  # the MultiNADE: M NADEs of P visibles; the one NADE: P M visibles ordered p M + m
    Din = E * tracks
    p = G.init_rnn_nade(9 + tracks, Din, E, HN, list(UNITS), F, tracks=tracks)
    gen = RnnNade(E, HN, list(UNITS), precision="fp32", seed=seed) if tracks == 1 else \
        RnnMultiNADE(E, HN, list(UNITS), tracks=list("abc")[:tracks], precision="fp32", seed=seed)
    gen._materialize(Din)
    TN.load_nade_params(gen, p)
    intro = (np.random.default_rng(60 + tracks).random((B, TI, Din)) < .3).astype(np.uint8)
    return gen, dev(intro)


def per_track(out):
    """[B, n, P M] in the order p M + m (the joint NADE's and the MultiNADE's) -> ones per step and track [B, n, M]."""
    return out.reshape(out.shape[0], out.shape[1], P, M).sum(2)


def within(out, caps, given=None):
    """Every row of every step within its caps, counting the free ones (a given cell always wins)."""
    free = out if given is None else out * (given == FREE)
    n = per_track(free)
    return all(bool((n[..., m] <= k).all()) for m, k in enumerate(caps) if k is not None)


@pytest.mark.parametrize("tracks", [1, 3])
@pytest.mark.parametrize("cap", [CAPS, 2])
def test_generate_captured_eager_and_step_by_step(monkeypatch, tracks, cap):
    from multinn_amd.common import DrawAt
    gen, x = nade_generator(tracks)
    base = gen.generate(x, STEPS)
    assert len(gen._scan_graphs._cache) == 1
    # caps that cannot bind are the call without one: the same bits, and no new captured scan
    for none in (P * M, (None,) * M, (P, None, P + 3)):
        assert torch.equal(gen.generate(x, STEPS, max_notes=none), base)
    assert len(gen._scan_graphs._cache) == 1
    out = gen.generate(x, STEPS, max_notes=cap)                     # captured: the one-call scan
    assert len(gen._scan_graphs._cache) == 2
    assert torch.equal(gen.generate(x, STEPS, max_notes=cap), out)  # replayed
    assert not torch.equal(out, base)
    if isinstance(cap, tuple) or tracks > 1:
        caps = cap if isinstance(cap, tuple) else (cap,) * M
        assert within(out, caps) and not within(base, caps)
    else:                                                           # one NADE, one integer: the whole step
        assert int(out.sum(2).max()) <= cap < int(base.sum(2).max())
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(x, STEPS, max_notes=cap), out)  # the eager one-call scan
    assert torch.equal(gen.generate(x.float(), STEPS, max_notes=cap), out)      # the step loop
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    state, last, rows = gen.steps(x), x[:, -1], []
    for j in range(STEPS):
        last, _ = gen.sample_single_capped(last, state, max_notes=cap, at=DrawAt(gen.seed, gen.row0, j))
        state = gen.single_step(last, state)
        rows.append(last)
    assert torch.equal(torch.stack(rows, 1), out)
    # with codes: the given cells stay, the free ones stay within the caps
    codes = dev(TN.random_codes(np.random.default_rng(3), (B, STEPS, P * M), 0.3))
    got = gen.generate(x, STEPS, given=codes, max_notes=cap, temperature=0.8)
    assert torch.equal(got[codes != FREE], codes[codes != FREE])
    if isinstance(cap, tuple) or tracks > 1:
        assert within(got, cap if isinstance(cap, tuple) else (cap,) * M, codes)


@pytest.mark.parametrize("tracks", [1, 3])
@pytest.mark.parametrize("byte_intro", [True, False], ids=["one-call chunks", "step loop"])
def test_session_chunks(monkeypatch, tracks, byte_intro):
    gen, x = nade_generator(tracks)
    x = x if byte_intro else x.float()
    whole = gen.generate(x, STEPS, max_notes=CAPS)
    sess = gen.session(x)
    sess.max_notes = CAPS
    assert sess.max_notes == CAPS
    assert torch.equal(torch.cat([sess.generate(n) for n in (1, 2, 3)], 1), whole)
    assert all(("max_notes", CAPS) in key for key in sess._graphs)
    # the cap changes between chunks: captured and eager chunks agree, each chunk keeps its own cap, the first is generate's
    plan = ((1, (0, None, 1)), (2, None), (3, (2, 2, 2)))

    def chunk(sess, n, cap):
        sess.max_notes = cap
        return sess.generate(n)
    sess = gen.session(x)
    captured = [chunk(sess, n, c) for n, c in plan]
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    sess = gen.session(x)
    eager = [chunk(sess, n, c) for n, c in plan]
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))
    assert torch.equal(captured[0], gen.generate(x, 1, max_notes=plan[0][1]))
    assert within(captured[0], plan[0][1]) and within(captured[2], plan[2][1])
    assert not torch.equal(torch.cat(captured, 1), gen.generate(x, STEPS))


@pytest.mark.parametrize("mode", ["joint", "jamming", "composer", "feedback-rnn"])
def test_modes(mode):
    m, _ = TN.make_mode(mode, P=P, M=M, B=B, Ti=TI)
    base = m.generate(STEPS)
    assert tuple(base.shape) == (B, STEPS, P, M)
    graphs = lambda: sum(len(o._scan_graphs._cache) for o in list(m.generators) + [getattr(m, "_sampler", None)]
                         if getattr(o, "_scan_graphs", None) is not None)
    n_graphs = graphs()
    for none in (None, P, (None, None, None), (P, P + 1, None)):    # today's call: the bits and the captured scans of before
        assert torch.equal(m.generate(STEPS, max_notes=none), base)
    assert graphs() == n_graphs
    out = m.generate(STEPS, max_notes=CAPS)
    assert torch.equal(m.generate(STEPS, max_notes=list(CAPS)), out)
    n = out.sum(2)                                                  # notes per step and track [B, STEPS, M]
    assert int(n[..., 0].max()) <= 1 and int(n[..., 2].max()) == 0, "track 0 monophonic, track 2 silent"
    assert int(base.sum(2)[..., 0].max()) > 1 and int(base.sum(2)[..., 2].max()) > 0, "the uncapped model must exceed the caps"
    if mode == "jamming":                                           # independent generators: the uncapped track keeps its bits
        assert torch.equal(out[..., 1], base[..., 1])
    if mode == "composer":                                          # tracks conditionally independent given the history: its first step does
        assert torch.equal(out[:, 0, :, 1], base[:, 0, :, 1])
    assert int(m.generate(STEPS, max_notes=2).sum(2).max()) <= 2
    R = np.random.default_rng(7)
    given = dev((R.random((B, STEPS, P, M)) < 0.3).astype(np.uint8))
    mask = torch.from_numpy(R.random((B, STEPS, P, M)) < 0.4)
    got = m.generate(STEPS, given=given, given_mask=mask, max_notes=CAPS, temperature=(0.8, 1.0, 1.2))
    full = mask.to(DEV)
    assert torch.equal(got[full], given[full]), "a given cell always wins"
    free = (got * ~full).sum(2)
    assert int(free[..., 0].max()) <= 1 and int(free[..., 2].max()) == 0
    if mode in ("joint", "jamming", "composer"):                    # and a session's chunks are the one call
        sess = m.session()
        sess.max_notes = CAPS
        assert torch.equal(torch.cat([sess.generate(k) for k in (2, 4)], 1), out)
