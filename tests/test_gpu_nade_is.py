"""The NADE importance estimator on the device (mnn_nade_given_is, ops.nade_given_is, estimate_nll(partial="importance"),
driver.evaluate(partial=)): the kernel against tests/nade_is_reference.py -- every particle bit for bit, the log weights against float64 --,
its identities (nothing given, everything given, a given prefix), the independence of a particle from the launch around it, the estimates
against exact enumeration and the direction of their two biases at the seeds tests/test_nade_is_cpu.py fixed, and the model-level API."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nade_is_reference as REF          # noqa: E402
import test_gpu_raise as TR              # noqa: E402
import test_nade_is_cpu as TC            # noqa: E402

DEV = "cuda:0"
FREE = REF.FREE
PATTERNS = ["density 0.3", "all free", "all given", "given prefix", "given suffix", "last given mid-row"]
SHAPES = [(3, 61, 30, 2),                # idle lanes, Hn % 4 != 0
          (4, 7, 256, 2),                # D under one Philox block
          (5, 333, 256, 3),              # elem0 = m D off a block boundary
          (72, 440, 256, 1)]             # the joint shape
dev, same_bytes = TR.dev, TR.same_bytes


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def pattern_of(n, m, N):
    return PATTERNS[(m * N + n) % len(PATTERNS)]


def problem(N, D, Hn, tracks, seed=0):
    """(bias, w_enc, w_dec, codes u8 [tracks, N, D], data u8 [tracks, N, D], row ids): the six code patterns on different (row, track) cells
    of one launch."""
    R = np.random.default_rng(N * 31 + D + seed)
    bias = (R.standard_normal((N, tracks * (Hn + D))) * .5).astype(np.float32)
    we = (R.standard_normal((tracks, D, Hn)) * .3).astype(np.float32)
    wd = (R.standard_normal((tracks, D, Hn)) * .3).astype(np.float32)
    vals = (R.random((tracks, N, D)) < 0.3).astype(np.uint8)
    codes = np.full((tracks, N, D), FREE, np.uint8)
    k = max(1, D // 3)
    for m in range(tracks):
        for n in range(N):
            kind = pattern_of(n, m, N)
            if kind == "density 0.3":
                codes[m, n] = np.where(R.random(D) < 0.3, vals[m, n], FREE)
            elif kind == "all given":
                codes[m, n] = vals[m, n]
            elif kind == "given prefix":
                codes[m, n, :k] = vals[m, n, :k]
            elif kind == "given suffix":
                codes[m, n, D - k:] = vals[m, n, D - k:]
            elif kind == "last given mid-row":
                codes[m, n, :D // 2] = np.where(R.random(D // 2) < 0.3, vals[m, n, :D // 2], FREE)
                codes[m, n, D // 2] = vals[m, n, D // 2]
    data = (R.random((tracks, N, D)) < 0.3).astype(np.uint8)
    ids = (1000 + 7 * np.arange(N)).astype(np.int32)
    return bias, we, wd, codes, data, ids


def run(ops, bias, we, wd, codes, data, C, seed, ids=None, row0=0, v=True):
    """One launch -> (log_pg [tracks, N], log_w [tracks, N, C], v_out [tracks, N, C, D] or None, stats [tracks, N, 2]) as NumPy."""
    tracks, N, D = codes.shape
    Hn = we.shape[2]
    log_w = torch.full((tracks, N, C), 7.0, device=DEV)
    v_out = torch.full((tracks, N, C, D), 9, device=DEV, dtype=torch.uint8) if v else None
    stats = torch.full((tracks, N, 2), 7.0, device=DEV)
    log_pg = ops.nade_given_is(dev(bias), dev(we), dev(wd), tracks, D, Hn, dev(codes), C, seed, row0=row0, row_ids=None if ids is None else dev(ids),
                               data=None if data is None else dev(data), log_w=log_w, v_out=v_out, stats=stats)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (log_pg, log_w, v_out, stats)]


# ------------------------------------------------------------------------------------------------
# 1. the kernel against the reference
@pytest.mark.parametrize("C", [1, 3, 8, 33])
@pytest.mark.parametrize("N,D,Hn,tracks", SHAPES)
def test_particles_bit_exact_and_weights_against_float64(ops, N, D, Hn, tracks, C):
    bias, we, wd, codes, data, ids = problem(N, D, Hn, tracks)
    seed = 77
    for side in (None, data):
        log_pg, log_w, v_out, stats = run(ops, bias, we, wd, codes, side, C, seed, ids)
        for m in range(tracks):
            v_ref, lw_ref, pg_ref, ess_ref, se_ref = REF.estimate(bias, we, wd, tracks, m, D, Hn, codes[m], None if side is None else side[m], C, seed, ids)
            assert np.array_equal(v_out[m], v_ref), "particles must be bit-exact"
            big = max(1.0, np.abs(lw_ref).max())
            print("side", "lower" if side is None else "upper", "track", m, "log_w rel", rel(log_w[m], lw_ref), "log_pg abs", np.abs(log_pg[m] - pg_ref).max(),
                  "bound", 1e-5 * big)
            assert rel(log_w[m], lw_ref) < 1e-5
            assert np.abs(log_pg[m] - pg_ref).max() <= 1e-5 * big
            np.testing.assert_allclose(stats[m, :, 0], ess_ref, rtol=1e-2)
            np.testing.assert_allclose(stats[m, :, 1], se_ref, rtol=1e-2)
            if side is not None:                                            # particle 0 is the data at the free cells, the codes at the others
                assert np.array_equal(v_out[m, :, 0], np.where(codes[m] != FREE, codes[m], side[m]))


# 2. identities
@pytest.mark.parametrize("C", [1, 3, 8, 33])
@pytest.mark.parametrize("N,D,Hn,tracks", SHAPES)
def test_identities(ops, N, D, Hn, tracks, C):
    """Nothing given: log_pg == 0, ESS == C, stderr == 0 (one particle: inf, mnn_rbm_ais's value -- a single weight says nothing about its
    spread), exactly.  Everything given: every particle's log w is -nll of ops.nade_sample(given=codes).  A given prefix only: all particles
    carry the same bits, ESS == C."""
    bias, we, wd, codes, data, ids = problem(N, D, Hn, tracks)
    smp = torch.empty((N, tracks * D), device=DEV, dtype=torch.uint8)
    nll = torch.empty((tracks, N), device=DEV)
    full = np.where(codes != FREE, codes, data)                              # every cell of every row given: the codes, the data where they are free
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, 1.0, 5, 0, 0, smp, nll=nll, given=dev(full.transpose(1, 0, 2).reshape(N, tracks * D)))
    nll = nll.cpu().numpy()
    assert np.array_equal(smp.cpu().numpy().reshape(N, tracks, D).transpose(1, 0, 2), full)
    for side in (None, data):
        log_pg, log_w, _, stats = run(ops, bias, we, wd, codes, side, C, 3, ids, v=False)
        pg_full, lw_full, _, st_full = run(ops, bias, we, wd, full, side, C, 3, ids, v=False)
        for c in range(C):
            assert rel(lw_full[:, :, c], -nll) < 1e-5
        assert np.all(lw_full.view(np.uint32) == lw_full.view(np.uint32)[:, :, :1]) and np.all(st_full[:, :, 0] == C) and np.all(pg_full == lw_full[:, :, 0])
        seen = set()
        for m in range(tracks):
            for n in range(N):
                kind = pattern_of(n, m, N)
                seen.add(kind)
                if kind == "all free":
                    assert log_pg[m, n] == 0.0 and np.all(log_w[m, n] == 0.0) and stats[m, n, 0] == C
                    assert stats[m, n, 1] == (0.0 if C > 1 else np.inf)
                elif kind == "all given":                                    # the same row in other company: the same bits
                    assert log_w[m, n].tobytes() == lw_full[m, n].tobytes()
                if kind in ("all given", "given prefix"):
                    assert np.all(log_w[m, n].view(np.uint32) == log_w[m, n].view(np.uint32)[0]) and stats[m, n, 0] == C
                    assert log_pg[m, n] == log_w[m, n, 0] and stats[m, n, 1] == (0.0 if C > 1 else np.inf)
        assert seen == set(PATTERNS) or N * tracks < len(PATTERNS)


# 3. a particle depends on its own counters only
@pytest.mark.parametrize("N,D,Hn,tracks", [(5, 333, 256, 3), (6, 61, 30, 2)])
def test_counter_independence(ops, N, D, Hn, tracks):
    """Particle c of row id r: the same log w bits in a launch of other N, other C and other companions, with the samples requested or not
    (a scan that stops behind the last given visible against one that runs to D), by row ids or by row0."""
    bias, we, wd, codes, data, ids = problem(N, D, Hn, tracks, seed=1)
    pick = [N - 1, 1]
    for side in (None, data):
        base = run(ops, bias, we, wd, codes, side, 8, 11, ids, v=False)
        with_v = run(ops, bias, we, wd, codes, side, 8, 11, ids, v=True)
        assert base[1].tobytes() == with_v[1].tobytes() and base[0].tobytes() == with_v[0].tobytes() and base[3].tobytes() == with_v[3].tobytes()
        other = run(ops, bias[pick], we, wd, codes[:, pick], None if side is None else side[:, pick], 33, 11, ids[pick], v=True)
        assert other[1][:, :, :8].tobytes() == base[1][:, pick].tobytes()
        assert other[2][:, :, :8].tobytes() == with_v[2][:, pick].tobytes()
        one = run(ops, bias[2:3], we, wd, codes[:, 2:3], None if side is None else side[:, 2:3], 3, 11, None, row0=int(ids[2]), v=False)
        assert one[1].tobytes() == base[1][:, 2:3, :3].tobytes()
    lower, upper = run(ops, bias, we, wd, codes, None, 8, 11, ids), run(ops, bias, we, wd, codes, data, 8, 11, ids)
    assert lower[2][:, :, 1:].tobytes() != upper[2][:, :, 1:].tobytes()      # the two sides of one seed share no uniform


@pytest.mark.parametrize("N,D,Hn,tracks,C,H", [(4, 7, 256, 2, 40001, 20100), (3, 61, 30, 2, 50001, 25100)])
def test_a_workgroup_that_outlives_one_particle_group(ops, N, D, Hn, tracks, C, H):
    """More particle groups than a row gets workgroups (10001 / 12501 groups of four against 8192 / 10923 workgroups: every workgroup takes two,
    G = 5001 / 6251), so a wave runs a second particle, c >= 4 G = 20004 / 25004, from the state it kept.  The first 33 particles are the
    bits of the C = 33 launch that test_particles_bit_exact_and_weights_against_float64 checks against the reference, and the first H, which
    reach behind 4 G, those of a C = H launch in which every particle is its wave's first (H / 4 groups fit the workgroups)."""
    most = -(-65536 // (N * tracks))
    groups = -(-C // 4)
    G = -(-groups // -(-groups // most))
    assert groups > most and 4 * G + 64 < H and -(-H // 4) <= most
    bias, we, wd, codes, data, ids = problem(N, D, Hn, tracks)
    for side in (None, data):
        small = run(ops, bias, we, wd, codes, side, 33, 77, ids)
        first = run(ops, bias, we, wd, codes, side, H, 77, ids)
        large = run(ops, bias, we, wd, codes, side, C, 77, ids)
        assert large[1][:, :, :33].tobytes() == small[1].tobytes()
        assert large[2][:, :, :33].tobytes() == small[2].tobytes()
        assert large[1][:, :, :H].tobytes() == first[1].tobytes()
        assert large[2][:, :, :H].tobytes() == first[2].tobytes()
        assert np.all(np.isfinite(large[0]))


# 4. the estimates against enumeration, and the direction of the two biases (the toy and seeds of tests/test_nade_is_cpu.py)
def toy_run(ops, p, side_data):
    bias, we, wd, x, codes = REF.toy_problem(p["n_rows"], p["w_scale"], p["seed"])
    out = run(ops, bias, we, wd, codes[None], None if not side_data else x[None], p["C"], p["draw_seed"], np.arange(p["n_rows"], dtype=np.int32), v=False)
    return out, TC.toy_exact(bias, we, wd, codes)


def test_lower_estimate_matches_enumeration(ops):
    (log_pg, _, _, stats), exact = toy_run(ops, TC.ACCURACY, False)
    err = np.abs(log_pg[0] - exact) / stats[0, :, 1]
    print("lower estimate against enumeration, C = 4096: error in reported standard errors, max", err.max())
    assert np.all(err < 5)


def test_biases_point_in_opposite_directions(ops):
    (lower, _, _, _), exact = toy_run(ops, TC.BIAS, False)
    (upper, _, _, _), _ = toy_run(ops, TC.BIAS, True)
    below, above = REF.paired_margin(exact, lower[0]), REF.paired_margin(upper[0], exact)
    print("means: lower", lower.mean(), "exact", exact.mean(), "upper", upper.mean(), "| margins in standard errors:", below, above)
    assert lower.mean() < exact.mean() < upper.mean() and below > 3 and above > 3, (below, above)


# ------------------------------------------------------------------------------------------------
# 5. estimators and modes (tiny models, fp32)
mode_config, mode_params, mode_batch = TR.mode_config, TR.mode_params, TR.mode_batch
TRACK0 = torch.tensor([True, False])
LOW1 = (torch.arange(10) < 4)[:, None] & torch.tensor([False, True])         # track 0 free, the low pitches of track 1 given
LOW1_GIVEN0 = LOW1 | torch.tensor([True, False])                             # track 0 wholly given, track 1 as above
B, T = 3, 4


def api_ids(g, lengths=None):
    keep = [(b, t) for b in range(B) for t in range(T) if lengths is None or t < int(lengths[b])]
    return torch.tensor([t * 65536 + g.row0 + b for b, t in keep], dtype=torch.int32, device=DEV)


def nade_weights(g):
    return g.store["nade/w_enc"], g.store["nade/w_dec"]


def by_hand(ops, g, codes_planes, tgt_planes, C, seed, side, ids):
    """ops.nade_given_is on the last build's valid rows: codes / targets u8 [tracks, n, D] in API order."""
    bias = g._ctx["out"][g._idx()].contiguous()
    M, D, Hn = g.num_tracks, g.num_dims, g.num_hidden[-1]
    stats = torch.empty((M, bias.shape[0], 2), device=DEV)
    lp = ops.nade_given_is(bias, *nade_weights(g), M, D, Hn, codes_planes.contiguous(), C, seed, row_ids=ids,
                           data=tgt_planes.contiguous() if side == "raise" else None, stats=stats)
    return lp, stats


def test_joint_nade_scores_one_track_given_the_other(ops):
    from multinn_amd import MultINN
    from multinn_amd.generators import NllBracket
    m = MultINN(mode_config(), mode_params("joint", "NADE"), mode="joint", precision="fp32")
    x = mode_batch(5)
    g = m._generators[0]
    kw = dict(given_mask=TRACK0, partial="importance", num_chains=16, seed=40)
    both = m.estimate_nll(x, method="both", **kw)
    assert isinstance(both, NllBracket) and both.gap == both.upper.mean - both.lower.mean
    codes = torch.where(TRACK0.to(DEV), x, torch.full_like(x, FREE)).reshape(1, B * T, 20)           # visibles p M + m, API order
    for method, side in (("ais", both.lower), ("raise", both.upper)):
        est = m.estimate_nll(x, method=method, **kw)
        lp, stats = by_hand(ops, g, codes, x.reshape(1, B * T, 20), 16, 40, method, api_ids(g))
        assert torch.equal(est.nll, g.log_probs + lp[0]) and same_bytes(est.nll, side.nll)
        assert torch.equal(est.log_z, lp[0]) and torch.equal(est.free_energy, g.log_probs)
        assert torch.equal(est.row_stderr, stats[0, :, 1]) and torch.equal(est.row_ess, stats[0, :, 0])
        assert est.nll.numel() == B * T and est.stderr > 0 and 1 <= est.ess <= 16.001
    assert not same_bytes(both.lower.log_z, both.upper.log_z)
    free = m.estimate_nll(x)
    assert both.upper.mean < free.mean                                       # one track given the other costs less than both
    # the generator's own call: x [B, T, P, M] flattened p M + m, the mask with it; default seed = the generator's
    own = g.estimate_nll(x.reshape(B, T, 20), given_mask=TRACK0.repeat(10), partial="importance", num_chains=16, seed=40)
    lp, _ = by_hand(ops, g, codes, x.reshape(1, B * T, 20), 16, 40, "ais", api_ids(g))
    assert torch.equal(own.nll, g.log_probs + lp[0])
    torch.testing.assert_close(own.nll, both.lower.nll, rtol=1e-4, atol=1e-4)


def test_one_data_particle_is_the_free_cells_own_conditionals(ops):
    """method="raise", num_chains=1: the one particle is the data, no RNG is involved: NLL(x) + log w = -sum_{i in F} log(1e-6 + q_i)."""
    from multinn_amd import MultINN
    m = MultINN(mode_config(), mode_params("joint", "NADE"), mode="joint", precision="fp32")
    x = mode_batch(5)
    g = m._generators[0]
    est = m.estimate_nll(x, given_mask=TRACK0, partial="importance", num_chains=1, method="raise")
    cp = g.cond_probs.double()
    v = x.reshape(B * T, 20).double()
    q = torch.where(v > 0, cp, 1 - cp)
    free = (~TRACK0).repeat(10).to(DEV)
    ref = -(torch.log(1e-6 + q) * free).sum(1)
    print("one data particle against the build's conditionals: max abs", float((est.nll.double() - ref).abs().max()))
    assert float((est.nll.double() - ref).abs().max()) < 1e-4
    again = m.estimate_nll(x, given_mask=TRACK0, partial="importance", num_chains=1, method="raise", seed=99)
    assert same_bytes(est.nll, again.nll)


def test_a_pitch_prefix_needs_no_sampling(ops):
    from multinn_amd import MultINN
    m = MultINN(mode_config(), mode_params("joint", "NADE"), mode="joint", precision="fp32")
    x = mode_batch(5)
    prefix = (torch.arange(10) < 4)[:, None].expand(10, 2)                   # visibles 0 .. 7 of p M + m
    both = m.estimate_nll(x, given_mask=prefix, partial="importance", num_chains=8, method="both")
    assert same_bytes(both.lower.nll, both.upper.nll) and both.gap == 0.0
    for side in (both.lower, both.upper):
        assert bool((side.row_stderr == 0).all()) and side.stderr == 0.0 and bool((side.row_ess == 8).all())
    cp = m._generators[0].cond_probs.double()
    v = x.reshape(B * T, 20).double()
    ref = -(torch.log(1e-6 + torch.where(v > 0, cp, 1 - cp))[:, 8:]).sum(1)
    assert float((both.lower.nll.double() - ref).abs().max()) < 1e-4


@pytest.mark.parametrize("mode", ["jamming", "feedback"])
def test_per_track_nades_estimate_only_the_partly_given_track(ops, mode):
    from multinn_amd import MultINN
    m = MultINN(mode_config(), mode_params(mode, "NADE"), mode=mode, precision="fp32")
    x = mode_batch(2)
    kw = dict(partial="importance", num_chains=8, seed=70)
    g0, g1 = m._generators
    codes1 = torch.where(LOW1[:, 1].to(DEV), x[..., 1], torch.full_like(x[..., 1], FREE)).reshape(1, B * T, 10)
    for method in ("ais", "raise"):
        est = m.estimate_nll(x, given_mask=LOW1, method=method, **kw)
        lp, _ = by_hand(ops, g1, codes1, x[..., 1].reshape(1, B * T, 10), 8, 71, method, api_ids(g1))       # generator i: seed + i
        part = g1.log_probs + lp[0]
        assert torch.equal(est.nll, g0.log_probs + part)                     # the free track adds its exact rows
        assert torch.equal(est.log_z, lp[0]) and torch.equal(est.free_energy, g1.log_probs)
        given0 = m.estimate_nll(x, given_mask=LOW1_GIVEN0, method=method, **kw)
        assert torch.equal(given0.nll, part)                                 # the wholly given track adds 0
    with pytest.raises(NotImplementedError, match="not a sum of its conditionals"):
        m.estimate_nll(x, given_mask=LOW1)


def test_composer_multinade_estimates_per_track(ops):
    from multinn_amd import MultINN
    m = MultINN(mode_config(), mode_params("composer", "NADE"), mode="composer", precision="fp32")
    x = mode_batch(4)
    g = m._generators[0]
    assert g.num_tracks == 2
    kw = dict(partial="importance", num_chains=8, seed=40)
    planes = x.permute(3, 0, 1, 2).reshape(2, B * T, 10)                     # [M, API rows, D]
    low = LOW1[:, 1].to(DEV)
    for method in ("ais", "raise"):
        est = m.estimate_nll(x, given_mask=LOW1, method=method, **kw)
        codes = torch.full_like(planes, FREE)
        codes[1] = torch.where(low, planes[1], codes[1])
        lp, _ = by_hand(ops, g, codes, planes, 8, 40, method, api_ids(g))     # one generator, one seed: the tracks differ by their elements m D + i
        rows = g.log_probs
        assert bool((lp[0] == 0).all())                                      # the free track: nothing to weigh
        assert torch.equal(est.nll, rows[0] + (rows[1] + lp[1]))
        given0 = m.estimate_nll(x, given_mask=LOW1_GIVEN0, method=method, **kw)
        assert torch.equal(given0.nll, rows[1] + lp[1])
    both_partial = LOW1 | ((torch.arange(10) >= 7)[:, None] & torch.tensor([True, False]))
    est = m.estimate_nll(x, given_mask=both_partial, **kw)
    codes = torch.where(both_partial.to(DEV), x, torch.full_like(x, FREE)).permute(3, 0, 1, 2).reshape(2, B * T, 10)
    lp, stats = by_hand(ops, g, codes, planes, 8, 40, "ais", api_ids(g))
    rows = g.log_probs
    assert torch.equal(est.nll, (rows[0] + lp[0]) + (rows[1] + lp[1])) and torch.equal(est.log_z, lp[0] + lp[1])
    assert torch.equal(est.row_ess, torch.minimum(stats[0, :, 0], stats[1, :, 0]))


def test_ragged_lengths_return_the_valid_rows_in_api_order(ops):
    from multinn_amd import MultINN
    m = MultINN(mode_config(), mode_params("joint", "NADE"), mode="joint", precision="fp32")
    x = mode_batch(5)
    kw = dict(given_mask=TRACK0, partial="importance", num_chains=8, seed=3, method="both")
    full = m.estimate_nll(x, **kw)
    lengths = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    rag = m.estimate_nll(x, lengths=lengths, **kw)
    keep = (torch.arange(T)[None, :] < lengths.cpu()[:, None]).reshape(-1).to(DEV)
    for side, whole in ((rag.lower, full.lower), (rag.upper, full.upper)):
        assert side.nll.numel() == 9
        assert torch.equal(side.log_z, whole.log_z[keep])                    # same bias rows, codes, targets and row ids: the same particles
        torch.testing.assert_close(side.nll, whole.nll[keep], rtol=1e-6, atol=1e-5)


def test_driver_evaluate_reports_a_gap(ops):
    from multinn_amd import MultINN, driver
    m = MultINN(mode_config(), mode_params("joint", "NADE"), mode="joint", precision="fp32")
    R = np.random.default_rng(3)
    X = (R.random((4, 8, 10, 2)) < 0.3).astype(np.uint8)
    lengths = np.array([8, 8, 6, 8])
    kw = dict(num_chains=4)
    mask = [True, False]
    lo = driver.evaluate(m, X, lengths, 2, 8, nll="ais", ais=kw, given_mask=mask, partial="importance")
    up = driver.evaluate(m, X, lengths, 2, 8, nll="raise", ais=kw, given_mask=mask, partial="importance")
    br = driver.evaluate(m, X, lengths, 2, 8, nll="bracket", ais=kw, given_mask=mask, partial="importance")
    assert set(br) == {"lower", "upper", "gap"} and br["lower"] == lo and br["upper"] == up and br["gap"] == up - lo
    assert np.isfinite(lo) and np.isfinite(up) and up != lo
    with pytest.raises(NotImplementedError, match="not a sum of its conditionals"):
        driver.evaluate(m, X, lengths, 2, 8, nll="bracket", ais=kw, given_mask=mask)
