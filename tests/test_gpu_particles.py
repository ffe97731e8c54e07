"""NADE importance resampling on the device (mnn_nade_sample_sir_at, ops.nade_sample_sir, generate(particles=)): the step op against
tests/nade_sir_reference.py -- every particle bit for bit, the log weights against float64, the pick against the float64 restatement applied
to the device's own log weights, the emitted vector, nll and ESS --, the short cut against ops.nade_sample(given=), strides and temperatures,
the statistical pin of tests/test_particles_cpu.py as one launch, and the scan level: one call against the eager loop, sessions, captured
against eager, the calls without particles, the clamp, the statistics and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nade_sir_reference as REF         # noqa: E402
import test_gpu_nade_is as TI            # noqa: E402
import test_particles_cpu as TP          # noqa: E402

DEV = "cuda:0"
FREE = REF.FREE
SHAPES, SEED, ROW0, SUB, SUB_CELL = TP.SHAPES, TP.SEED, TP.ROW0, TP.SUB, TP.SUB_CELL
dev = TI.dev


def test_the_reference_restates_the_estimators_problem():
    """nade_sir_reference.problem is tests/test_gpu_nade_is.py::problem (its six code patterns), array for array."""
    for shape in SHAPES + [TP.NINE]:
        for a, b in zip(REF.problem(*shape), TI.problem(*shape)[:4]):
            assert np.array_equal(a, b)
    assert REF.PATTERNS == TI.PATTERNS


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def flat(codes):
    """[tracks, N, D] -> the [N, tracks * D] layout of ops.nade_sample (feature m D + i)."""
    tracks, N, D = codes.shape
    return np.ascontiguousarray(codes.transpose(1, 0, 2).reshape(N, tracks * D))


def run(ops, bias, we, wd, codes, C, temps=(1.0, False), seed=SEED, row0=ROW0, sub=SUB, cell=SUB_CELL):
    """One launch -> (samples [tracks, N, D], nll, ess, pick [tracks, N], log_w [tracks, N, C]) as NumPy.  The sub-counter is sub + cell, the
    cell read on the device."""
    tracks, N, D = codes.shape
    Hn = we.shape[2]
    out = torch.full((N, tracks * D), 9, device=DEV, dtype=torch.uint8)
    nll = torch.full((tracks, N), 7.0, device=DEV)
    log_w = torch.full((tracks, N, C), 7.0, device=DEV)
    base = None if cell is None else torch.tensor([cell], dtype=torch.int32, device=DEV)
    ess, pick = ops.nade_sample_sir(dev(bias), dev(we), dev(wd), tracks, D, Hn, temps[0], seed, row0, sub, out, dev(flat(codes)), C, nll=nll,
                                    by_visible=temps[1], sub_base=base, log_w=log_w)
    torch.cuda.synchronize()
    return (out.cpu().numpy().reshape(N, tracks, D).transpose(1, 0, 2),) + tuple(t.cpu().numpy() for t in (nll, ess, pick, log_w))


def plain(ops, bias, we, wd, codes, temps=(1.0, False), seed=SEED, row0=ROW0, sub=SUB + SUB_CELL):
    """ops.nade_sample(given=) at the same counters -> (samples [tracks, N, D], nll [tracks, N])."""
    tracks, N, D = codes.shape
    out = torch.full((N, tracks * D), 9, device=DEV, dtype=torch.uint8)
    nll = torch.full((tracks, N), 7.0, device=DEV)
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, we.shape[2], temps[0], seed, row0, sub, out, nll=nll, given=dev(flat(codes)), by_visible=temps[1])
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(N, tracks, D).transpose(1, 0, 2), nll.cpu().numpy()


def check_against_reference(ops, N, D, Hn, tracks, C, kind):
    parts, prob, tvecs = REF.cached_particles(N, D, Hn, tracks, max(C, TP.C_SHARED) if kind == "one" else C, SEED, ROW0, SUB + SUB_CELL, kind)
    bias, we, wd, codes = prob[:4]
    temps = REF.temps_argument(kind, tracks)
    out, nll, ess, pick, log_w = run(ops, bias, we, wd, codes, C, temps)
    base, base_nll = plain(ops, bias, we, wd, codes, temps)
    rows = ROW0 + np.arange(N)
    left_out = 0
    for m in range(tracks):
        ref = REF.resample(bias, we, wd, tracks, m, D, Hn, codes[m], C, SEED, rows, SUB + SUB_CELL, tvecs[m], parts=parts[m])
        sc = ref["shortcut"]
        assert sc.any() and not sc.all()
        # the short cut: the bits of the call without particles, ESS = C
        assert np.array_equal(out[m][sc], base[m][sc]) and nll[m][sc].tobytes() == base_nll[m][sc].tobytes()
        assert np.all(ess[m][sc] == C) and np.all(pick[m][sc] == 0)
        assert np.all(log_w[m][sc].view(np.uint32) == log_w[m][sc].view(np.uint32)[:, :1])
        # the weights against float64
        print("track", m, "log_w rel", TI.rel(log_w[m], ref["log_w"]))
        assert TI.rel(log_w[m][~sc], ref["log_w"][~sc]) < 1e-5 and TI.rel(log_w[m][sc, 0], ref["log_w"][sc, 0]) < 1e-5
        # the pick: the float64 restatement on the device's own log weights
        p_dev, ess_ref, near = REF.pick_from(log_w[m], REF.pick_uniform(SEED, rows, SUB + SUB_CELL, m))
        use = ~sc & ~near
        left_out += int((near & ~sc).sum())
        assert np.array_equal(pick[m][use], p_dev[use])
        np.testing.assert_allclose(ess[m][~sc], ess_ref[~sc], rtol=1e-2)
        assert np.all(ess[m] >= 1 - 1e-3) and np.all(ess[m] <= C * (1 + 1e-3))
        # the emitted vector is particle `pick`, bit for bit (so every particle that any row picked is checked; all of them: below), its nll the model's
        n = np.arange(N)
        assert np.array_equal(out[m], ref["v"][n, pick[m]])
        assert TI.rel(nll[m], ref["nll"][n, pick[m]]) < 1e-5
        assert np.array_equal(out[m][codes[m] != FREE], codes[m][codes[m] != FREE])
    assert left_out <= 1e-3 * N * tracks
    return bias, we, wd, codes, parts


# ------------------------------------------------------------------------------------------------
# 1. the step op against the reference
@pytest.mark.parametrize("C", TP.CS)
@pytest.mark.parametrize("N,D,Hn,tracks", SHAPES)
def test_step_against_reference(ops, N, D, Hn, tracks, C):
    check_against_reference(ops, N, D, Hn, tracks, C, "one")


@pytest.mark.parametrize("kind", ["scalar", "track", "visible"])
@pytest.mark.parametrize("N,D,Hn,tracks", SHAPES[:3])
def test_step_temperatures(ops, N, D, Hn, tracks, kind):
    check_against_reference(ops, N, D, Hn, tracks, 5, kind)


@pytest.mark.parametrize("kind", ["one", "scalar", "visible"])
def test_more_tracks_than_table_entries(ops, kind):
    """Nine tracks: the plain sampler walks them eight at a time, and a scalar temperature is one number for all nine -- against the reference
    and, where nothing is resampled, ops.nade_sample(given=)."""
    check_against_reference(ops, *TP.NINE, 5, kind)


@pytest.mark.parametrize("kind", ["one", "visible"])
@pytest.mark.parametrize("N,D,Hn,tracks", SHAPES)
def test_every_particle_bit_exact(ops, N, D, Hn, tracks, kind):
    """Every particle's vector (read out of the workspace) against the checker: all C of a scan that resamples, particle 0 of a short-cut scan."""
    C = TP.C_SHARED if kind == "one" else 5
    parts, prob, tvecs = REF.cached_particles(N, D, Hn, tracks, C, SEED, ROW0, SUB + SUB_CELL, kind)
    bias, we, wd, codes = prob[:4]
    temps = REF.temps_argument(kind, tracks)
    out = torch.full((N, tracks * D), 9, device=DEV, dtype=torch.uint8)
    v = torch.full((tracks, N, C, D), 9, device=DEV, dtype=torch.uint8)
    ops.nade_sample_sir(dev(bias), dev(we), dev(wd), tracks, D, Hn, temps[0], SEED, ROW0, SUB, out, dev(flat(codes)), C, by_visible=temps[1],
                        sub_base=torch.tensor([SUB_CELL], dtype=torch.int32, device=DEV), v_out=v)
    v = v.cpu().numpy()
    for m in range(tracks):
        sc = REF.is_shortcut(codes[m])
        assert np.array_equal(v[m][~sc], parts[m][0][~sc]), "particles must be bit-exact"
        assert np.array_equal(v[m][sc, 0], parts[m][0][sc, 0])


def test_particles_do_not_depend_on_their_company(ops):
    """A scan's result depends on its own counters only: the same rows in a smaller launch (other N, another row0 offsetting to the same row
    ids) return the same bytes; C and 2 C share their first C log weights."""
    N, D, Hn, tracks = SHAPES[2]
    bias, we, wd, codes = REF.problem(N, D, Hn, tracks)
    full = run(ops, bias, we, wd, codes, 5)
    part = run(ops, bias[2:4], we, wd, codes[:, 2:4], 5, row0=ROW0 + 2)
    for a, b in zip(full, part):
        assert a[:, 2:4].tobytes() == b.tobytes()
    twice = run(ops, bias, we, wd, codes, 10)
    assert full[4].tobytes() == np.ascontiguousarray(twice[4][:, :, :5]).tobytes()


@pytest.mark.parametrize("N,D,Hn,tracks,temps", [(150, 7, 256, 2, (1.0, False)), (150, 13, 32, 2, (REF.VISIBLE_TEMPS, True))])
def test_a_workgroup_that_outlives_one_particle_group(ops, N, D, Hn, tracks, temps):
    """C = 1021 is 256 groups of four against 219 workgroups a scan gets, so every workgroup takes two (G = 128) and a wave runs a second
    particle, c >= 4 G = 512, from the state it kept: the first five particles (their vectors out of the workspace, their log weights) are the
    bytes of the C = 5 launch, and the first 600, which reach behind 4 G, those of a C = 600 launch in which every particle is its wave's
    first (150 groups fit the workgroups)."""
    C, H = 1021, 600
    most = -(-65536 // (N * tracks))
    assert -(-C // 4) == 256 > most >= -(-H // 4) and 4 * 128 + 64 < H
    bias, we, wd, codes = REF.problem(N, D, Hn, tracks)
    got = []
    for c in (5, H, C):
        out = torch.full((N, tracks * D), 9, device=DEV, dtype=torch.uint8)
        v = torch.full((tracks, N, c, D), 9, device=DEV, dtype=torch.uint8)
        log_w = torch.full((tracks, N, c), 7.0, device=DEV)
        ops.nade_sample_sir(dev(bias), dev(we), dev(wd), tracks, D, Hn, temps[0], SEED, ROW0, SUB, out, dev(flat(codes)), c, by_visible=temps[1],
                            sub_base=torch.tensor([SUB_CELL], dtype=torch.int32, device=DEV), log_w=log_w, v_out=v)
        got.append((v.cpu().numpy(), log_w.cpu().numpy()))
    (v5, lw5), (vh, lwh), (vc, lwc) = got
    for m in range(tracks):
        sc = REF.is_shortcut(codes[m])
        assert sc.any() and not sc.all()
        assert vc[m][~sc][:, :5].tobytes() == v5[m][~sc].tobytes()
        assert vc[m][sc, 0].tobytes() == v5[m][sc, 0].tobytes()
        assert lwc[m][:, :5].tobytes() == lw5[m].tobytes()
        assert vc[m][~sc][:, :H].tobytes() == vh[m][~sc].tobytes()
        assert vc[m][sc, 0].tobytes() == vh[m][sc, 0].tobytes()
        assert lwc[m][:, :H].tobytes() == lwh[m].tobytes()


def test_strides(ops):
    """Track-minor samples (feature i tracks + m), and a view of track m of a [B, steps, P, M] roll: the bytes of the contiguous call."""
    N, D, Hn, tracks = SHAPES[0]
    bias, we, wd, codes = REF.problem(N, D, Hn, tracks)
    want = run(ops, bias, we, wd, codes, 5, cell=None)
    out = torch.full((N, D * tracks), 9, device=DEV, dtype=torch.uint8)
    given = dev(np.ascontiguousarray(codes.transpose(1, 2, 0).reshape(N, D * tracks)))
    ess, pick = ops.nade_sample_sir(dev(bias), dev(we), dev(wd), tracks, D, Hn, 1.0, SEED, ROW0, SUB, out, given, 5, track_minor=True)
    assert np.array_equal(out.cpu().numpy().reshape(N, D, tracks).transpose(2, 0, 1), want[0])
    assert np.array_equal(ess.cpu().numpy(), want[2]) and np.array_equal(pick.cpu().numpy(), want[3])
    # one NADE (track 0's weights, its own bias block) writing track 1 of step 2 of a roll
    b1 = np.ascontiguousarray(np.concatenate([bias[:, :Hn], bias[:, tracks * Hn:tracks * Hn + D]], 1))
    ref_out = torch.full((N, D), 9, device=DEV, dtype=torch.uint8)
    e1, p1 = ops.nade_sample_sir(dev(b1), dev(we[:1]), dev(wd[:1]), 1, D, Hn, 1.0, SEED, ROW0, SUB, ref_out, dev(codes[0]), 5)
    roll = torch.full((N, 4, D, 3), 9, device=DEV, dtype=torch.uint8)
    g_roll = torch.full((N, 4, D, 3), FREE, device=DEV, dtype=torch.uint8)
    g_roll[:, 2, :, 1] = dev(codes[0])
    e2, p2 = ops.nade_sample_sir(dev(b1), dev(we[:1]), dev(wd[:1]), 1, D, Hn, 1.0, SEED, ROW0, SUB, roll[:, 2, :, 1], g_roll[:, 2, :, 1], 5)
    assert torch.equal(roll[:, 2, :, 1], ref_out) and torch.equal(e1, e2) and torch.equal(p1, p2)
    roll[:, 2, :, 1] = 9
    assert bool((roll == 9).all()), "nothing outside the view is written"
    # (a launch of ONE track spaces its particles by E4 = 64, the two-track launch above by 124: from particle 2 on they are other draws)
    assert not np.array_equal(ref_out.cpu().numpy(), want[0][0])


def test_toy_bound_on_the_device(ops):
    """The statistical pin of test_particles_cpu.py as one launch: the particles are the reference's, and the frequency of v0 = 1 among the
    emitted rows meets the bound that the clamped scan misses."""
    bias, we, wd, codes = REF.toy_problem()
    p, rho = REF.toy_exact(bias, we, wd)
    out, nll, ess, pick, log_w = run(ops, bias, we, wd, codes[None], REF.TOY_C, seed=TP.TOY_SEED, row0=0, sub=0, cell=None)
    ref = TP.toy_reference()
    v = torch.full((1, REF.TOY_N, REF.TOY_C, REF.TOY_D), 9, device=DEV, dtype=torch.uint8)
    ops.nade_sample_sir(dev(bias), dev(we), dev(wd), 1, REF.TOY_D, REF.TOY_HN, 1.0, TP.TOY_SEED, 0, 0, torch.empty((REF.TOY_N, REF.TOY_D), device=DEV, dtype=torch.uint8),
                        dev(codes), REF.TOY_C, v_out=v)
    assert np.array_equal(v[0].cpu().numpy(), ref["v"]), "every particle of the toy is the reference's"
    assert TI.rel(log_w[0], ref["log_w"]) < 1e-5
    assert np.array_equal(out[0], ref["v"][np.arange(REF.TOY_N), pick[0]])
    agree = (pick[0] == ref["pick"]).mean()
    f = out[0][:, 0].mean()
    base, _ = plain(ops, bias, we, wd, codes[None], seed=TP.TOY_SEED, row0=0, sub=0)
    assert np.array_equal(base[0], ref["v"][:, 0])
    print("p", p, "rho", rho, "f", f, "clamped", base[0][:, 0].mean(), "bound", REF.toy_bound(p, rho), "picks equal to the reference's", agree)
    assert abs(f - p) <= REF.toy_bound(p, rho)
    assert abs(base[0][:, 0].mean() - p) > REF.toy_bound(p, rho)
    assert agree >= 0.999


def test_step_refusals(ops):
    N, D, Hn, tracks = SHAPES[0]
    bias, we, wd, codes = REF.problem(N, D, Hn, tracks)
    out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
    args = (dev(bias), dev(we), dev(wd), tracks, D, Hn)
    for bad in (1, 1025, True, 2.0):
        with pytest.raises(ValueError):
            ops.nade_sample_sir(*args, 1.0, SEED, ROW0, SUB, out, dev(flat(codes)), bad)
    with pytest.raises(ValueError):
        ops.nade_sample_sir(*args, None, SEED, ROW0, SUB, out, dev(flat(codes)), 4)
    # no codes at all: the launch of ops.nade_sample, with the statistics of a scan that resamples nothing
    a, b = torch.full((N, tracks * D), 9, device=DEV, dtype=torch.uint8), torch.full((N, tracks * D), 9, device=DEV, dtype=torch.uint8)
    na, nb = torch.zeros((tracks, N), device=DEV), torch.zeros((tracks, N), device=DEV)
    ess, pick = ops.nade_sample_sir(*args, 0.5, SEED, ROW0, SUB, a, None, 7, nll=na, ess=torch.full((tracks, N), -1.0, device=DEV),
                                    pick=torch.full((tracks, N), -1, device=DEV, dtype=torch.int32))
    ops.nade_sample(*args, 0.5, SEED, ROW0, SUB, b, nll=nb)
    assert torch.equal(a, b) and torch.equal(na, nb) and bool((ess == 7).all()) and bool((pick == 0).all())
    assert ops.nade_sample_sir_workspace_bytes(tracks, N, D, 1) == 0
    assert ops.nade_sample_sir_workspace_bytes(tracks, N, D, 4) >= tracks * N * 4 * (D + 8)


# ------------------------------------------------------------------------------------------------
# 2. the scan level, at the small model shapes of tests/test_gpu_session.py
import test_gpu_session as TS            # noqa: E402

C_SCAN = 4


def scan_problem(tracks):
    gen = TS.nade_gen(tracks, 24 if tracks == 1 else 8, 32, [64, 32], seed=37)[0]
    B, Ti, steps, n_out = 6, 3, 7, 24
    R = np.random.default_rng(51 + tracks)
    intro = dev((R.random((B, Ti, n_out)) < .3).astype(np.uint8))
    codes = dev(TS.random_codes(R, (B, steps, n_out)))
    return gen, intro, codes, steps, (0.5 if tracks == 1 else (0.5, 1.0, 2.0))


def eager(monkeypatch, fn):
    monkeypatch.setenv("MULTINN_GENERATE_GRAPH", "0")
    try:
        return fn()
    finally:
        monkeypatch.delenv("MULTINN_GENERATE_GRAPH")


@pytest.mark.parametrize("tracks", [1, 3])
def test_one_call_step_loop_sessions_and_graphs_agree(monkeypatch, tracks):
    gen, intro, codes, steps, temp = scan_problem(tracks)
    B = intro.shape[0]
    clamped = codes != FREE
    for T in (1.0, temp):
        plain_out = gen.generate(intro, steps, given=codes, temperature=T)
        assert gen.particle_ess() is None
        one = gen.generate(intro, steps, given=codes, temperature=T, particles=C_SCAN)              # captured
        ess, picks = gen.particle_ess(), gen.particle_picks()
        assert ess.shape == picks.shape == (B, steps, tracks) and ess.dtype == torch.float32 and picks.dtype == torch.int32
        assert bool((ess >= 1 - 1e-3).all()) and bool((ess <= C_SCAN + 1e-3).all()) and bool((picks >= 0).all()) and bool((picks < C_SCAN).all())
        assert bool((picks > 0).any()) and not torch.equal(one, plain_out), "some scan picked another particle than the clamped scan's"
        assert torch.equal(one[clamped], codes[clamped])
        assert torch.equal(gen.generate(intro, steps, given=codes, temperature=T, particles=C_SCAN), one)      # replayed
        assert torch.equal(gen.particle_ess(), ess) and torch.equal(gen.particle_picks(), picks)
        # the eager one-call scan, and the eager step loop through sample_single_resampled
        assert torch.equal(eager(monkeypatch, lambda: gen.generate(intro, steps, given=codes, temperature=T, particles=C_SCAN)), one)
        assert torch.equal(gen.particle_ess(), ess) and torch.equal(gen.particle_picks(), picks)
        assert torch.equal(gen.generate(intro.float(), steps, given=codes, temperature=T, particles=C_SCAN), one)
        assert torch.equal(gen.particle_ess(), ess) and torch.equal(gen.particle_picks(), picks)
        assert torch.equal(eager(monkeypatch, lambda: gen.generate(intro.float(), steps, given=codes, temperature=T, particles=C_SCAN)), one)
        # the calls without particles return the parent call's bytes
        for none in (None, 0, 1):
            assert torch.equal(gen.generate(intro, steps, given=codes, temperature=T, particles=none), plain_out)
            assert gen.particle_ess() is None and gen.particle_picks() is None
        assert torch.equal(gen.generate(intro, steps, temperature=T, particles=C_SCAN), gen.generate(intro, steps, temperature=T))
        assert gen.particle_ess() is None
        # sessions: every split is the one call; the statistics are the last chunk's
        for split in ((3, 2, 2), (1, 6)):
            for x in (intro, intro.float()):
                sess = gen.session(x)
                sess.particles = C_SCAN
                assert sess.particles == C_SCAN
                got = TS.chunks(sess, split, given=codes, temperature=T)
                assert torch.equal(got, one), (split, x.dtype, int((got != one).sum()))
                assert torch.equal(sess.particle_ess(), ess[:, -split[-1]:]) and torch.equal(sess.particle_picks(), picks[:, -split[-1]:])

    def schedule(sess):                                               # particles changing between chunks, a chunk without codes among them
        out = []
        for n, a, c in ((2, 0, C_SCAN), (2, 2, 0), (1, 4, 2), (2, 5, C_SCAN)):
            sess.particles = c
            out.append(sess.generate(n, given=codes[:, a:a + n].contiguous() if a != 4 else None))
            assert (sess.particle_ess() is None) == (c == 0 or a == 4)
        return torch.cat(out, 1)
    cap = schedule(gen.session(intro))
    assert torch.equal(eager(monkeypatch, lambda: schedule(gen.session(intro))), cap)
    assert torch.equal(schedule(gen.session(intro.float())), cap)
    one = gen.generate(intro, steps, given=codes, particles=C_SCAN)
    assert torch.equal(cap[:, :2], one[:, :2]) and not torch.equal(cap, one)


def test_generator_refusals_on_the_device():
    from multinn_amd._lib import MnnUnsupported
    gen, intro, codes, steps, temp = scan_problem(1)
    with pytest.raises(MnnUnsupported, match="max_notes"):
        gen.generate(intro, steps, given=codes, particles=4, max_notes=1)
    with pytest.raises(ValueError, match="temperature"):
        gen.generate(intro, steps, given=codes, particles=4, temperature=None)
    for bad in (True, 1.5, -1, 1025):
        with pytest.raises(ValueError):
            gen.generate(intro, steps, given=codes, particles=bad)
    sess = gen.session(intro)
    sess.particles, sess.max_notes = 4, 1
    with pytest.raises(MnnUnsupported, match="max_notes"):
        sess.generate(2, given=codes[:, :2].contiguous())
    assert sess.steps == 0
    sess.max_notes = None
    with pytest.raises(ValueError, match="temperature"):
        sess.generate(2, given=codes[:, :2].contiguous(), temperature=None)
    assert sess.generate(2, temperature=None).shape == (6, 2, 24)                                  # nothing given: nothing to resample
    state = gen.steps(intro)
    with pytest.raises(ValueError):
        gen.sample_single_resampled(None, state, given=codes[:, 0].contiguous(), particles=1025)
    a, _ = gen.sample_single_resampled(None, state, given=codes[:, 0].contiguous(), particles=1)
    b, _ = gen.sample_single(None, state, given=codes[:, 0].contiguous())
    assert torch.equal(a, b)
    # an RBM generator ignores the argument: its clamped chain already conditions on every given cell
    rbm = TS.rbm_gen(24, 40, [64, 32], 4)[0]
    assert torch.equal(rbm.generate(intro, 3, given=codes[:, :3].contiguous(), particles=4), rbm.generate(intro, 3, given=codes[:, :3].contiguous()))
    assert rbm.particle_ess() is None


@pytest.mark.parametrize("mode", ["joint", "composer", "jamming"])
def test_modes(mode):
    m = TS.make_mode(mode, "NADE")
    B, steps, P, M = 4, 6, 8, 3
    R = np.random.default_rng(3)
    given = dev((R.random((B, steps, P, M)) < 0.3).astype(np.uint8))
    track = torch.tensor([True, False, False])                       # one of M tracks given: accompaniment
    cells = torch.from_numpy(R.random((B, steps, P, M)) < 0.3)
    plain_t, plain_c = m.generate(steps, given=given, given_mask=track), m.generate(steps, given=given, given_mask=cells)
    assert all(e is None for e in m.particle_ess())
    out_t = m.generate(steps, given=given, given_mask=track, particles=C_SCAN)
    ess_t = m.particle_ess()
    out_c = m.generate(steps, given=given, given_mask=cells, particles=C_SCAN)
    ess_c, picks_c = m.particle_ess(), m.particle_picks()
    assert torch.equal(out_t[..., 0], given[..., 0]) and torch.equal(out_c[cells.to(DEV)], given[cells.to(DEV)])
    assert len(ess_c) == len(m.generators)
    if mode == "joint":                                               # one NADE over p M + m: the free tracks' cells now know of the given track's notes behind them
        assert ess_t[0].shape == (B, steps, 1) and bool((ess_t[0] < C_SCAN).any()) and not torch.equal(out_t, plain_t)
    else:                                                             # a NADE per track, wholly given or wholly free: the short cut, at the bits of the call without
        assert torch.equal(out_t, plain_t)
        assert all(e is None or bool((e == C_SCAN).all()) for e in ess_t)
    assert not torch.equal(out_c, plain_c)
    for e, p in zip(ess_c, picks_c):
        assert e.shape == p.shape == (B, steps, M if mode == "composer" else 1)       # (composer: one MultiNADE of M tracks)
        assert bool((e >= 1 - 1e-3).all()) and bool((e <= C_SCAN + 1e-3).all()) and bool((p >= 0).all()) and bool((p < C_SCAN).all())
    for none in (None, 0, 1):
        assert torch.equal(m.generate(steps, given=given, given_mask=cells, particles=none), plain_c)
    assert torch.equal(m.generate(steps, particles=C_SCAN), m.generate(steps))
    # the session carries the particles as a property
    sess = m.session()
    sess.particles = C_SCAN
    got = torch.cat([sess.generate(b - a, given=given[:, a:b].contiguous(), given_mask=cells[:, a:b]) for a, b in ((0, 2), (2, 3), (3, 6))], 1)
    assert torch.equal(got, out_c)
    assert all(torch.equal(a, b[:, 3:]) for a, b in zip(sess.particle_ess(), ess_c))
    from multinn_amd._lib import MnnUnsupported
    with pytest.raises(MnnUnsupported, match="max_notes"):
        m.generate(steps, given=given, given_mask=cells, particles=C_SCAN, max_notes=1)
    with pytest.raises(ValueError, match="temperature"):
        m.generate(steps, given=given, given_mask=cells, particles=C_SCAN, temperature=None)


@pytest.mark.parametrize("mode", ["feedback", "feedback-rnn"])
def test_feedback_modes_refuse(mode):
    from multinn_amd._lib import MnnUnsupported
    from multinn_amd import MultINN
    P, M, B, Ti = 8, 3, 4, 3
    cfg = {"model_name": "t", "data": {"pitch_range": {"lowest": 0, "highest": P}, "instruments": TS.TRACKS[:M], "beat_resolution": 4},
           "training": {"num_pixels": 1, "random_seed": 23}}
    prm = {"mode": mode, "tune_encoder": False, "keep_prob": 0.9, "encoder": {"type": "Pass", "num_hidden": None},
           "generator": {"type": "NADE", "num_hidden": 16, "num_hidden_rnn": [32, 32], "feedback": [32, 32], "k": 3}}
    x = (np.random.default_rng(14).random((B, Ti, P, M)) < 0.3).astype(np.uint8)
    m = MultINN(cfg, prm, mode=mode, precision="fp32")
    m.build(dev(x), lengths=None, is_train=False, mode="generate")
    given = dev((np.random.default_rng(3).random((B, 4, P, M)) < 0.3).astype(np.uint8))
    with pytest.raises(MnnUnsupported, match="particle form"):
        m.generate(4, given=given, given_mask=torch.tensor([True, False, False]), particles=4)
    with pytest.raises(ValueError):
        m.generate(4, particles=True)
    assert torch.equal(m.generate(4, particles=4), m.generate(4))      # nothing given: the call without particles
