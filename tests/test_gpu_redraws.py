"""The polyphony cap by rejection on the device (`redraws=`): the REDRAW sampling kernels against redraw_reference (the deterministic checker
run attempt by attempt), the kernel forms against one another, the identities that make `redraws=0` and caps that cannot bind today's calls,
the distribution an accepted row is drawn from, and the generate paths.

Problems are sparse (redraw_reference.sparse_problem: about two ones per track), so that at a cap of 1 a row accepts at once, accepts after
a redraw or falls back, each with a share of the rows; the conditions are asserted on the reference's own outputs."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nade as onade                                   # noqa: E402
import test_gpu_conditional as TN                                  # noqa: E402
import test_gpu_max_notes as TM                                    # noqa: E402
import redraw_reference as RR                                      # noqa: E402

DEV = "cuda:0"
FREE = 255
F = np.float32
dev, rel = TN.dev, TN.rel
SEED, ROW0, SUB, R = 77, 1000, 5, 3
FORM_KEYS = ("MNN_SAMPLE_NO_CHUNK", "MNN_SAMPLE_G8", "MNN_SAMPLE_NO_SPEC")


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def stats_cell():
    return torch.zeros(2, device=DEV, dtype=torch.int32)


def track_temp(temp, m):
    return temp[m] if isinstance(temp, tuple) else temp


def counters(cap, by_visible, m, D):
    if by_visible:
        return np.arange(D) % len(cap), list(cap)
    return np.zeros(D, int), [cap[m] if isinstance(cap, tuple) else cap]


@functools.lru_cache(maxsize=None)
def reference(N, D, Hn, tracks, cap, by_visible, temp, with_given, redraws=R):
    """The problem and, per track, redraw_reference's (samples, conditionals, accepted): computed once per case, shared, never written to."""
    bias, we, wd, codes = RR.sparse_problem(N, D, Hn, tracks, 0, temp)
    if not with_given:
        codes = np.full_like(codes, FREE)
    per_track = []
    for m in range(tracks):
        counter, caps = counters(cap, by_visible, m, D)
        per_track.append(RR.redraw_reference(bias, we[m], wd[m], tracks, m, D, Hn, track_temp(temp, m), SEED, np.arange(ROW0, ROW0 + N), SUB,
                                             codes[:, m], counter, caps, redraws))
    return bias, we, wd, codes, per_track


def run(ops, bias, we, wd, codes, tracks, D, Hn, temp, with_given, **kw):
    N = bias.shape[0]
    out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
    nll = torch.zeros((tracks, N), device=DEV)
    stats = stats_cell()
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, temp, seed=SEED, row0=ROW0, sub=SUB, samples=out, nll=nll,
                    given=dev(codes.reshape(N, tracks * D)) if with_given else None, redraw_stats=stats, **kw)
    return out, nll, tuple(int(x) for x in stats.cpu())


# (N, D, Hn, tracks, max_notes, by_visible): the shapes and caps of test_gpu_max_notes -- Hn % 4 != 0 is the visible-at-a-time kernel; D = 7
# lies below one chunk; 333 x 3: chunks, track offsets and Philox windows that do not line up, across attempts; 300 rows: chunks of 8; 72: of 16
CASES = [(*shape, cap, False) for shape in TM.PER_TRACK for cap in (1, 3)] + [(5, 333, 256, 3, (0, 2, None), False)] + \
        [(72, 440, 256, 1, TM.TABLE, True), (72, 7, 256, 1, TM.TABLE, True)]


# 1. kernels vs the reference
@pytest.mark.parametrize("with_given", [False, True], ids=["free", "given"])
@pytest.mark.parametrize("temp", [1.0, 0.7, "per-track"])
@pytest.mark.parametrize("N,D,Hn,tracks,cap,by_visible", CASES)
def test_redraw_sample_bit_exact(ops, N, D, Hn, tracks, cap, by_visible, temp, with_given):
    if temp == "per-track":
        temp = (0.7, 1.0, 1.3)[:tracks]
    bias, we, wd, codes, per_track = reference(N, D, Hn, tracks, cap, by_visible, temp, with_given)
    accepted = np.stack([a for _, _, a in per_track])
    if cap == 1 and (N, D) in ((300, 24), (72, 440)):               # on the reference alone: every outcome of a row occurs
        n0, later, fell = int((accepted == 0).sum()), int((accepted > 0).sum()), int((accepted == RR.FALLBACK).sum())
        print(f"accepted on attempt 0: {n0}, later: {later}, fallback: {fell} of {N}")
        assert n0 > 0 and later > 0 and fell > 0 and 4 * fell <= N
    out, nll, stats = run(ops, bias, we, wd, codes, tracks, D, Hn, temp, with_given, by_visible=by_visible, max_notes=cap, redraws=R)
    got = out.cpu().numpy().reshape(N, tracks, D)
    for m, (s_ref, p_ref, acc) in enumerate(per_track):
        assert np.array_equal(got[:, m], s_ref), "draws must be bit-exact"
        given = codes[:, m] != FREE
        assert np.array_equal(got[:, m][given], codes[:, m][given]), "a given cell always wins"
        counter, caps = counters(cap, by_visible, m, D)
        ok = acc != RR.FALLBACK
        assert not RR.violations(got[:, m][ok], codes[:, m][ok], counter, caps).any(), "an accepted row has no free 1 past a cap"
        q = np.where(s_ref > 0, p_ref, F(1.0) - p_ref).astype(np.float64)
        assert rel(nll[m].cpu().numpy(), -np.log(1e-6 + q).sum(1)) < 1e-5
        be = bias[:, m * Hn:(m + 1) * Hn].astype(np.float64)
        bd = bias[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D].astype(np.float64)
        n64, _ = onade.log_prob(s_ref.astype(np.float64), be, bd, we[m].astype(np.float64), wd[m].astype(np.float64))
        assert rel(nll[m].cpu().numpy(), n64) < 2e-4
    assert stats == RR.stats_of([accepted])


# 2. the kernel forms agree
@pytest.mark.parametrize("tracks,cap,by_visible", [(2, (1, 2), False), (1, TM.TABLE, True)])
def test_redraw_kernel_forms_agree(ops, monkeypatch, tracks, cap, by_visible):
    N, D, Hn = 40, 440, 256
    for temp in (1.0, 0.8):
        bias, we, wd, codes, per_track = reference(N, D, Hn, tracks, cap, by_visible, temp, True)
        res = []
        for form in ({}, {"MNN_SAMPLE_G8": "1"}, {"MNN_SAMPLE_NO_CHUNK": "1"}, {"MNN_SAMPLE_NO_CHUNK": "1", "MNN_SAMPLE_NO_SPEC": "1"}):
            for k in FORM_KEYS:                                     # chunks of 16 | chunks of 8 | visible at a time | no speculation
                monkeypatch.delenv(k, raising=False)
            for k, v in form.items():
                monkeypatch.setenv(k, v)
            res.append(run(ops, bias, we, wd, codes, tracks, D, Hn, temp, True, by_visible=by_visible, max_notes=cap, redraws=R))
        for out, nll, stats in res[1:]:
            assert torch.equal(out, res[0][0]) and torch.equal(nll, res[0][1]) and stats == res[0][2], temp
        assert res[0][2] == RR.stats_of([a for _, _, a in per_track]) and res[0][2][0] > 0
        assert np.array_equal(res[0][0].cpu().numpy().reshape(N, tracks, D), np.stack([s for s, _, _ in per_track], 1))
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)


# 2b. the multi-job launch (the feedback scan's step): job j is the single launch of generator j -- E4 is D rounded up, per job
@pytest.mark.parametrize("temp", [1.0, (0.7, 1.0, 1.3)])
def test_multi_job_launch_equals_single_launches(ops, temp):
    N, D, Hn, J, caps = 40, 22, 256, 3, (1, None, 2)
    probs = [RR.sparse_problem(N, D, Hn, 1, 10 + j, track_temp(temp, j)) for j in range(J)]
    out = torch.zeros((N, D, J), device=DEV, dtype=torch.uint8)     # job j writes track j of a [N, P, M] step: element stride J
    given = dev(np.stack([p[3][:, 0] for p in probs], 2))
    nll = torch.zeros((J, N), device=DEV)
    stats = stats_cell()
    jobs = [dict(bias=dev(p[0]), w_enc=dev(p[1][0]), w_dec=dev(p[2][0]), seed=SEED + j, samples=out[:, :, j], nll=nll[j], given=given[:, :, j])
            for j, p in enumerate(probs)]
    ops.nade_sample_multi(jobs, D, Hn, temp, ROW0, SUB, max_notes=caps, redraws=R, redraw_stats=stats)
    accepted = []
    for j, (bias, we, wd, codes) in enumerate(probs):
        s_ref, p_ref, acc = RR.redraw_reference(bias, we[0], wd[0], 1, 0, D, Hn, track_temp(temp, j), SEED + j, np.arange(ROW0, ROW0 + N), SUB,
                                                codes[:, 0], np.zeros(D, int), [caps[j]], R)
        accepted.append(acc)
        assert np.array_equal(out[:, :, j].cpu().numpy(), s_ref), j
        q = np.where(s_ref > 0, p_ref, F(1.0) - p_ref).astype(np.float64)
        assert rel(nll[j].cpu().numpy(), -np.log(1e-6 + q).sum(1)) < 1e-5
        if caps[j] is not None:                                     # and the single launch of that generator: the same bits and counts
            one, cell = torch.zeros((N, D), device=DEV, dtype=torch.uint8), stats_cell()
            ops.nade_sample(dev(bias), dev(we), dev(wd), 1, D, Hn, track_temp(temp, j), seed=SEED + j, row0=ROW0, sub=SUB, samples=one,
                            given=dev(codes[:, 0]), max_notes=caps[j], redraws=R, redraw_stats=cell)
            assert torch.equal(one, out[:, :, j]) and tuple(int(v) for v in cell.cpu()) == RR.stats_of([acc])
    got = tuple(int(v) for v in stats.cpu())
    assert got == RR.stats_of(accepted) and got[0] > 0


# 3. identity
@pytest.mark.parametrize("N,D,Hn,tracks", [(40, 440, 256, 2), (3, 61, 30, 2), (300, 64, 256, 1)])
@pytest.mark.parametrize("temp", [1.0, 0.7])
def test_nothing_moves_when_it_should_not(ops, N, D, Hn, tracks, temp):
    bias, we, wd, codes = RR.sparse_problem(N, D, Hn, tracks, 1, temp)
    for with_given in (False, True):
        args = (ops, bias, we, wd, codes, tracks, D, Hn, temp, with_given)
        capped, plain = run(*args, max_notes=1), run(*args)
        assert not torch.equal(capped[0], plain[0]), "the cap must bind"
        got = run(*args, max_notes=1, redraws=0)                    # no redraws: the capped call
        assert torch.equal(got[0], capped[0]) and torch.equal(got[1], capped[1]) and got[2] == (0, 0)
        for cap in (None, D, (None,) * tracks):                     # nothing to violate: the plain call
            got = run(*args, max_notes=cap, redraws=R)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and got[2] == (0, 0), cap
        most = int(plain[0].reshape(N, tracks, D).sum(2).max())     # a cap that can bind and that no row reaches: the REDRAW kernels, the plain bits
        assert most < D
        got = run(*args, max_notes=most, redraws=R)
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and got[2] == (0, 0)


# 4. the distribution
@pytest.mark.parametrize("form", [{}, {"MNN_SAMPLE_NO_CHUNK": "1"}], ids=["chunks", "visible-at-a-time"])
def test_accepted_rows_follow_the_restricted_distribution(ops, monkeypatch, form):
    """16384 rows of one model, 8 visibles, at most one note: the counts of the 9 allowed vectors lie within 5 sigma of N pi, pi from a float64
    enumeration; the truncating sampler (redraws = 0) misses that by more than 10 sigma somewhere (arithmetic: about 70) -- the test can tell
    the two apart.  test_redraws_cpu shows both statements for the reference sampler alone."""
    N, D, Hn = RR.DIST_N, RR.DIST_D, RR.DIST_HN
    bias, we, wd = RR.distribution_problem()
    pi = RR.exact_restricted(bias[0], we[0], wd[0])
    assert int((pi > 0).sum()) == 9
    codes = np.full((N, D), FREE, np.uint8)
    _, _, acc = RR.redraw_reference(bias, we[0], wd[0], 1, 0, D, Hn, 1.0, RR.DIST_SEED, np.arange(RR.DIST_ROW0, RR.DIST_ROW0 + N), RR.DIST_SUB,
                                    codes, np.zeros(D, int), [1], RR.DIST_REDRAWS)
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in form.items():
        monkeypatch.setenv(k, v)
    b, e, d = dev(bias), dev(we), dev(wd)

    def draw(redraws):
        out, stats = torch.zeros((N, D), device=DEV, dtype=torch.uint8), stats_cell()
        ops.nade_sample(b, e, d, 1, D, Hn, 1.0, seed=RR.DIST_SEED, row0=RR.DIST_ROW0, sub=RR.DIST_SUB, samples=out, max_notes=1, redraws=redraws,
                        redraw_stats=stats)
        return RR.outcome_counts(out.cpu().numpy()), tuple(int(x) for x in stats.cpu())
    counts, stats = draw(RR.DIST_REDRAWS)
    excess = RR.sigma_excess(counts, pi, N)
    print("counts", counts[pi > 0], "expected", N * pi[pi > 0], "sigmas", excess[pi > 0], "stats", stats)
    assert stats == RR.stats_of([acc])
    assert np.nanmax(excess) <= 5.0
    assert counts[pi == 0].sum() == 0 or stats[1] > 0
    counts0, stats0 = draw(0)
    excess0 = RR.sigma_excess(counts0, pi, N)
    print("truncating sampler: sigmas", excess0[pi > 0])
    assert stats0 == (0, 0) and np.nanmax(excess0) > 10.0
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------
# 5. the generate paths, at the small models of test_gpu_max_notes
B, TI, STEPS, P, M = TM.B, TM.TI, TM.STEPS, TM.P, TM.M
CAPS = (2, None, 1)


def step_by_step(gen, x, cap, redraws, temperature=1.0):
    """sample_single_redrawn + single_step from the intro's state, the statistics of all steps added up in one cell."""
    from multinn_amd.common import DrawAt
    stats = stats_cell()
    state, last, rows = gen.steps(x), x[:, -1], []
    for j in range(STEPS):
        last, _ = gen.sample_single_redrawn(last, state, temperature=temperature, max_notes=cap, redraws=redraws, redraw_stats=stats,
                                            at=DrawAt(gen.seed, gen.row0, j))
        state = gen.single_step(last, state)
        rows.append(last)
    return torch.stack(rows, 1), tuple(int(v) for v in stats.cpu())


@pytest.mark.parametrize("tracks", [1, 3])
@pytest.mark.parametrize("cap", [CAPS, 3])
def test_generate_captured_eager_and_step_by_step(monkeypatch, tracks, cap):
    gen, x = TM.nade_generator(tracks)
    plain, capped = gen.generate(x, STEPS), gen.generate(x, STEPS, max_notes=cap)
    graphs = lambda: len(gen._scan_graphs._cache)
    assert graphs() == 2
    # no redraws, or nothing to violate: the calls, bits and captured scans of before
    assert torch.equal(gen.generate(x, STEPS, max_notes=cap, redraws=0), capped) and gen.redraw_counts() == (0, 0)
    assert torch.equal(gen.generate(x, STEPS, redraws=R), plain) and torch.equal(gen.generate(x, STEPS, max_notes=P * M, redraws=R), plain)
    assert graphs() == 2 and gen.redraw_counts() == (0, 0)
    out = gen.generate(x, STEPS, max_notes=cap, redraws=R)         # captured: the one-call scan, the fill of the statistics a node of it
    counts = gen.redraw_counts()
    assert graphs() == 3 and counts[0] > 0 and counts[0] >= counts[1]
    assert not torch.equal(out, capped) and not torch.equal(out, plain)
    assert torch.equal(gen.generate(x, STEPS, max_notes=cap, redraws=R), out) and gen.redraw_counts() == counts      # replayed: counted from zero again
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(gen.generate(x, STEPS, max_notes=cap, redraws=R), out) and gen.redraw_counts() == counts      # the eager one-call scan
    assert torch.equal(gen.generate(x.float(), STEPS, max_notes=cap, redraws=R), out) and gen.redraw_counts() == counts    # the step loop
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    rows, stats = step_by_step(gen, x, cap, R)
    assert torch.equal(rows, out) and stats == counts               # redraw_counts() is the sum over the steps
    if isinstance(cap, tuple) or tracks > 1:                        # fallbacks truncate: every row stays within the caps
        assert TM.within(out, cap if isinstance(cap, tuple) else (cap,) * M)
    # with codes and another temperature: the given cells stay
    codes = dev(TN.random_codes(np.random.default_rng(3), (B, STEPS, P * M), 0.3))
    got = gen.generate(x, STEPS, given=codes, max_notes=cap, redraws=R, temperature=0.8)
    assert torch.equal(got[codes != FREE], codes[codes != FREE])
    with pytest.raises(ValueError):
        gen.generate(x, STEPS, max_notes=cap, redraws=R, temperature=None)


@pytest.mark.parametrize("tracks", [1, 3])
@pytest.mark.parametrize("byte_intro", [True, False], ids=["one-call chunks", "step loop"])
def test_session_chunks(monkeypatch, tracks, byte_intro):
    gen, x = TM.nade_generator(tracks)
    x = x if byte_intro else x.float()
    whole = gen.generate(x, STEPS, max_notes=CAPS, redraws=R)
    counts = gen.redraw_counts()
    for split in ((1, 2, 3), (4, 2)):                               # every chunk but the first starts at steps > 0: the sub-counter base
        sess = gen.session(x)
        sess.max_notes, sess.redraws = CAPS, R
        assert sess.redraws == R
        chunks, total = [], np.zeros(2, int)
        for n in split:
            chunks.append(sess.generate(n))
            total += sess.redraw_counts()
        assert torch.equal(torch.cat(chunks, 1), whole) and tuple(total) == counts
        assert all(("redraws", R) in key for key in sess._graphs)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    sess = gen.session(x)
    sess.max_notes, sess.redraws = CAPS, R
    assert torch.equal(torch.cat([sess.generate(n) for n in (2, 4)], 1), whole)
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    sess = gen.session(x)                                           # redraws back at 0, and redraws without a cap: the chunks of before
    sess.max_notes, sess.redraws = CAPS, R
    sess.redraws = 0
    assert torch.equal(sess.generate(2), gen.generate(x, 2, max_notes=CAPS)) and sess.redraw_counts() == (0, 0)
    sess = gen.session(x)
    sess.redraws = R
    assert torch.equal(sess.generate(2), gen.generate(x, 2)) and sess.redraw_counts() == (0, 0)


@pytest.mark.parametrize("mode", ["joint", "jamming", "composer", "feedback-rnn"])
def test_modes(monkeypatch, mode):
    m, _ = TN.make_mode(mode, P=P, M=M, B=B, Ti=TI)
    plain, capped = m.generate(STEPS), m.generate(STEPS, max_notes=CAPS)
    graphs = lambda: sum(len(o._scan_graphs._cache) for o in list(m.generators) + [getattr(m, "_sampler", None)]
                         if getattr(o, "_scan_graphs", None) is not None)
    n_graphs = graphs()
    assert torch.equal(m.generate(STEPS, max_notes=CAPS, redraws=0), capped) and torch.equal(m.generate(STEPS, redraws=R), plain)
    assert graphs() == n_graphs and m.redraw_counts() == (0, 0)
    out = m.generate(STEPS, max_notes=CAPS, redraws=R)
    counts = m.redraw_counts()
    assert counts[0] > 0 and not torch.equal(out, capped)
    n = out.sum(2)                                                  # notes per step and track [B, STEPS, M]: fallbacks truncate
    assert int(n[..., 0].max()) <= CAPS[0] and int(n[..., 2].max()) <= CAPS[2]
    assert torch.equal(m.generate(STEPS, max_notes=list(CAPS), redraws=R), out) and m.redraw_counts() == counts
    # a replayed call without redraws reports none, and the replay of the redrawn scan behind it reports its own again
    assert torch.equal(m.generate(STEPS, max_notes=CAPS), capped) and m.redraw_counts() == (0, 0)
    assert torch.equal(m.generate(STEPS, max_notes=CAPS, redraws=R), out) and m.redraw_counts() == counts
    assert torch.equal(m.generate(STEPS), plain) and m.redraw_counts() == (0, 0)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")               # the eager scan: the same launches outside a graph
    assert torch.equal(m.generate(STEPS, max_notes=CAPS, redraws=R), out) and m.redraw_counts() == counts
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    if mode == "jamming":                                           # independent generators: each track is its generator's own scan, step by step
        total = np.zeros(2, int)
        for i, (g, x) in enumerate(zip(m.generators, m._generator_inputs())):
            if CAPS[i] is None:
                assert torch.equal(out[..., i], plain[..., i])
                continue
            rows, stats = step_by_step(g, x, CAPS[i], R)
            assert torch.equal(rows, out[..., i])
            total += stats
        assert tuple(total) == counts
    if mode == "joint":                                             # one NADE over p M + m, caps by visible: its own scan, step by step
        rows, stats = step_by_step(m.generators[0], m._generator_inputs()[0], CAPS, R)
        assert torch.equal(rows.reshape(out.shape), out) and stats == counts
    if mode == "composer":                                          # one MultiNADE: a cap per track
        rows, stats = step_by_step(m.generators[0], m._generator_inputs()[0], CAPS, R)
        assert torch.equal(rows.reshape(out.shape), out) and stats == counts
    if mode in ("joint", "jamming", "composer"):                    # and a session's chunks are the one call
        sess = m.session()
        sess.max_notes, sess.redraws = CAPS, R
        total = np.zeros(2, int)
        chunks = []
        for k in (2, 4):
            chunks.append(sess.generate(k))
            total += sess.redraw_counts()
        assert torch.equal(torch.cat(chunks, 1), out) and tuple(total) == counts
    if mode == "jamming":                                           # a chunk that gives track 0 as a whole: its generator reports nothing for it
        sess = m.session()
        sess.max_notes, sess.redraws = CAPS, R
        sess.generate(2)
        assert sess._subs[0].redraw_counts()[0] > 0
        sess.generate(2, given=out[:, 2:4].contiguous(), given_mask=torch.tensor([True, False, False]))
        assert sess._subs[0].redraw_counts() == (0, 0)
        assert sess.redraw_counts() == tuple(int(v) for v in np.sum([s_.redraw_counts() for s_ in sess._subs[1:]], 0))
    got = m.generate(STEPS, max_notes=CAPS, redraws=R, temperature=(0.8, 1.0, 1.2))
    assert int(got.sum(2)[..., 0].max()) <= CAPS[0]
    with pytest.raises(ValueError):
        m.generate(STEPS, max_notes=CAPS, redraws=R, temperature=None)


def test_feedback_scan_against_the_checker(monkeypatch):
    """The feedback scan under caps and redraws against det.feedback_rnn_generate restated attempt by attempt: generator i's step s is
    redraw_reference on its Dense output with its own seed, sub-counter s, E4 = P rounded up to 4 and element 0 (a job of the multi-job
    launch).  The grouped sampler (one nade_sample_multi per step) gives those bits and redraw_counts() the sum over generators and steps;
    the per-lane sampler (sample_single_redrawn on M streams, one shared cell) gives the same bits and counts."""
    from oracle import det, philox, generators as G
    from multinn_amd import RnnNade
    from multinn_amd.feedback import FeedbackRnn, FeedbackRnnSampler
    Bn, Ti, Pn, Mn, Hn, Fb, temps, caps = 8, 3, 8, 3, 16, 32, (0.8, 1.0, 1.2), (1, None, 2)
    x = (np.random.default_rng(14).random((Bn, Ti, Pn, Mn)) < .3).astype(np.uint8)
    fb = FeedbackRnn(Pn * Mn, [64, Fb], precision="fp32", seed=40)

    class LaneNade(RnnNade):                                        # not an RnnNade by name: the scan takes its per-lane path
        pass

    gens, lane_gens, gparams, seeds = [], [], [], []
    for i in range(Mn):
        p = G.init_rnn_nade(60 + i, Pn + Fb, Pn, Hn, [32, 32], F)
        p['fc_b'][Hn:] = F(np.log(0.2 / 0.8) * temps[i])            # about 1.6 ones of 8 from the tempered sampler
        for cls, lst in ((RnnNade, gens), (LaneNade, lane_gens)):
            g = cls(Pn, Hn, [32, 32], precision="fp32", seed=50 + i)
            g._materialize(Pn + Fb)
            TN.load_nade_params(g, p)
            lst.append(g)
        gparams.append(p)
        seeds.append(50 + i)
    fb_layers = [(fb.store[f"feedback/rnn/cell_{l}/kernel"].cpu().numpy(), fb.store[f"feedback/rnn/cell_{l}/bias"].cpu().numpy()) for l in range(2)]
    # the checker's loop (det.feedback_rnn_generate), the sample of a capped generator taken attempt by attempt
    enc = np.concatenate([np.zeros((Bn, 1, Pn, Mn), np.float32), x.astype(np.float32)], axis=1)
    stack = enc.reshape(Bn, Ti + 1, Pn * Mn)
    fb_state, states, hs = None, [None] * Mn, [None] * Mn
    for t in range(Ti + 1):
        f, fb_state = det.lstm_step(stack[:, t], fb_state, fb_layers)
        for i, p in enumerate(gparams):
            hs[i], states[i] = det.lstm_step(np.concatenate([enc[:, t, :, i], f], 1), states[i], p['lstm'])
    outs = [det.dense(hs[i], p['fc_k'], p['fc_b']) for i, p in enumerate(gparams)]
    rows = np.arange(gens[0].row0, gens[0].row0 + Bn, dtype=np.uint32)
    free = np.full((Bn, Pn), FREE, np.uint8)
    ref, accepted = np.empty((Bn, STEPS, Pn, Mn), np.uint8), []
    for s in range(STEPS):
        cur = []
        for i, p in enumerate(gparams):
            if caps[i] is None:
                u = philox.uniform_block(seeds[i], philox.STREAM_NADE, rows, s, Pn)
                cur.append(det.nade_sample(outs[i], p['w_enc'][0], p['w_dec'][0], 1, 0, Pn, Hn, temps[i], u)[0])
            else:
                smp, _, acc = RR.redraw_reference(outs[i], p['w_enc'][0], p['w_dec'][0], 1, 0, Pn, Hn, temps[i], seeds[i], rows, s, free,
                                                  np.zeros(Pn, int), [caps[i]], R)
                cur.append(smp)
                accepted.append(acc)
        st = np.stack(cur, -1)
        ref[:, s] = st
        f, fb_state = det.lstm_step(st.reshape(Bn, Pn * Mn), fb_state, fb_layers)
        for i, p in enumerate(gparams):
            hs[i], states[i] = det.lstm_step(np.concatenate([cur[i].astype(np.float32), f], 1), states[i], p['lstm'])
            outs[i] = det.dense(hs[i], p['fc_k'], p['fc_b'])
    counts = RR.stats_of(accepted)
    accepted = np.concatenate(accepted)
    assert (accepted == 0).any() and (accepted > 0).any() and counts[1] > 0, "on the checker alone: every outcome of a scan occurs"
    sampler = FeedbackRnnSampler(gens, fb)
    kw = dict(temperature=temps, max_notes=caps)
    out = sampler.generate(dev(x), STEPS, redraws=R, **kw)
    assert np.array_equal(out.cpu().numpy(), ref) and sampler.redraw_counts() == counts
    capped = sampler.generate(dev(x), STEPS, **kw)                  # without redraws: no counts; the replay behind it: its own again
    assert sampler.redraw_counts() == (0, 0) and not torch.equal(capped, out)
    assert torch.equal(sampler.generate(dev(x), STEPS, redraws=R, **kw), out) and sampler.redraw_counts() == counts
    assert torch.equal(sampler.generate(dev(x), STEPS, **kw), capped) and sampler.redraw_counts() == (0, 0)
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(sampler.generate(dev(x), STEPS, redraws=R, **kw), out) and sampler.redraw_counts() == counts
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    lanes = FeedbackRnnSampler(lane_gens, fb)                       # the per-lane path, captured and eager
    assert torch.equal(lanes.generate(dev(x), STEPS, redraws=R, **kw), out) and lanes.redraw_counts() == counts
    assert torch.equal(lanes.generate(dev(x), STEPS, redraws=R, **kw), out) and lanes.redraw_counts() == counts
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    assert torch.equal(lanes.generate(dev(x), STEPS, redraws=R, **kw), out) and lanes.redraw_counts() == counts
    monkeypatch.delenv("MULTINN_GENERATE_GRAPH")
    assert torch.equal(lanes.generate(dev(x), STEPS, **kw), capped) and lanes.redraw_counts() == (0, 0)
