"""The polyphony cap by rejection, restated on the deterministic checker (no device): what `redraws=R` must emit, bit for bit.

One scan (track m of a launch, or the joint NADE's whole vector with its by-visible counters) runs in attempts.  Attempt a draws from its own
uniforms -- stream NADE at element e for a = 0, stream NADE_REDRAW at element (a - 1) E4 + e behind it, E4 the launch's element count rounded
up to a multiple of 4 -- with the clamped, UNCONSTRAINED scan (det.nade_sample on clamp_u'd uniforms).  A row violates on an attempt iff some
free visible is 1 at a position where the ones of its counter in front of it, given and drawn, have already reached the cap (a given 1 past
the cap pushes the count beyond it: `>=`).  Abandoning the attempt at the first violation is the same as finishing the scan and checking, so
the reference finishes it.  A row accepts the first attempt < R on which it does not violate and emits that scan; a row still pending at
attempt R emits test_gpu_max_notes.capped_reference -- the truncating sampler -- on attempt R's uniforms, and is a fallback iff the
unconstrained scan on those uniforms violates (up to its first violation the truncating scan IS the unconstrained one)."""
import numpy as np

from oracle import det, philox
import test_gpu_conditional as TN
import test_gpu_max_notes as TM

FREE = 255
F = np.float32
STREAM_NADE_REDRAW = 10
FALLBACK = -1


def attempt_uniforms(seed, rows, sub, elem0, D, E4, a):
    """[len(rows), D]: what attempt a reads for the visibles of a scan whose visible 0 is element elem0 of the launch."""
    e = np.arange(elem0, elem0 + D, dtype=np.int64)
    if a == 0:
        return philox.uniform(seed, philox.STREAM_NADE, np.asarray(rows, np.uint32)[:, None], sub, e[None, :].astype(np.uint32))
    return philox.uniform(seed, STREAM_NADE_REDRAW, np.asarray(rows, np.uint32)[:, None], sub, ((a - 1) * E4 + e)[None, :].astype(np.uint32))


def violations(s, codes, counter, caps):
    """[N, D] bool: the free ones of s that stand where their counter is exhausted."""
    out = np.zeros(s.shape, bool)
    free = codes == FREE
    for c, k in enumerate(caps):
        if k is None:
            continue
        idx = np.flatnonzero(counter == c)
        before = np.cumsum(s[:, idx], 1, dtype=np.int64) - s[:, idx]
        out[:, idx] = free[:, idx] & (s[:, idx] == 1) & (before >= k)
    return out


def redraw_reference(bias, we, wd, tracks, m, D, Hn, temp, seed, rows, sub, codes, counter, caps, redraws, E4=None, elem0=None):
    """One scan under caps with `redraws` tries -> (samples u8 [N, D], conditionals f32 [N, D], accepted [N]: the accepting attempt, or
    FALLBACK).  bias [N, tracks (Hn + D)]; we / wd [D, Hn] of track m; rows: the N Philox rows; codes [N, D]; counter [D] and caps as
    capped_reference's; E4 / elem0 default to a launch of `tracks` tracks of D visibles (the multi-job launch: E4 = roundup4(D), elem0 = 0)."""
    N = bias.shape[0]
    E4 = (tracks * D + 3) // 4 * 4 if E4 is None else E4
    elem0 = m * D if elem0 is None else elem0
    rows = np.asarray(rows)
    s_out, p_out = np.zeros((N, D), np.uint8), np.zeros((N, D), F)
    accepted = np.full(N, FALLBACK, int)
    pending = np.arange(N)
    for a in range(redraws + 1):
        if pending.size == 0:
            break
        u = attempt_uniforms(seed, rows[pending], sub, elem0, D, E4, a)
        s, p = det.nade_sample(bias[pending], we, wd, tracks, m, D, Hn, temp, TN.clamp_u(u, codes[pending]))
        bad = violations(s, codes[pending], counter, caps).any(1)
        if a < redraws:
            ok = pending[~bad]
            s_out[ok], p_out[ok], accepted[ok] = s[~bad], p[~bad], a
            pending = pending[bad]
        else:
            s_out[pending], p_out[pending], _ = TM.capped_reference(bias[pending], we, wd, tracks, m, D, Hn, temp, u, codes[pending], counter, caps)
            accepted[pending[~bad]] = a
    return s_out, p_out, accepted


def stats_of(accepted_list):
    """(redrawn, fallback): the scans that did not accept on attempt 0, and those that fell back -- what the kernels add to stats[2]."""
    acc = np.concatenate([np.ravel(a) for a in accepted_list])
    return int((acc != 0).sum()), int((acc == FALLBACK).sum())


def sparse_problem(N, D, Hn, tracks, seed=0, temps=None, given_ones=0.1):
    """About two expected ones per track: b_dec around logit(2 / D), small weights (the dense problem() of the capped tests would send every
    row to the fallback).  temps (None: 1, a float, or one per track): the block of a track drawn at temperature T is scaled by T, so that it
    is the TEMPERED sampler that emits about two ones.  Codes: about three given cells per track and row, `given_ones` ones among them per
    track on average.  -> bias, we, wd, codes [N, tracks, D]"""
    R = np.random.default_rng(seed)
    bias = np.empty((N, tracks * (Hn + D)), F)
    bias[:, :tracks * Hn] = R.standard_normal((N, tracks * Hn)) * .5
    p = min(0.5, 2.0 / D)
    t = np.ones(tracks) if temps is None else np.broadcast_to(np.asarray(temps, float), (tracks,))
    bias[:, tracks * Hn:] = (np.log(p / (1 - p)) + R.standard_normal((N, tracks * D)) * .25) * np.repeat(t, D)[None, :]
    we = (R.standard_normal((tracks, D, Hn)) * .02).astype(F)
    wd = (R.standard_normal((tracks, D, Hn)) * .02).astype(F)
    shape = (N, tracks, D)
    vals = (R.random(shape) < given_ones / 3.0).astype(np.uint8)
    codes = np.where(R.random(shape) < min(0.5, 3.0 / D), vals, FREE).astype(np.uint8)
    return bias, we, wd, codes


# ------------------------------------------------------------------------------------------------
# the distribution test's problem: 8 visibles, one cap of 1, every row the same model
DIST_N, DIST_D, DIST_HN, DIST_REDRAWS, DIST_SEED, DIST_ROW0, DIST_SUB = 16384, 8, 256, 32, 123, 0, 2


def distribution_problem(seed=0):
    """One bias row shared by DIST_N rows (non-zero w_enc and w_dec, marginals near 0.25) -> bias [DIST_N, Hn + D], we, wd [1, D, Hn]."""
    R = np.random.default_rng(seed)
    row = np.concatenate([R.standard_normal(DIST_HN) * .5, np.log(1 / 3.0) + R.standard_normal(DIST_D) * .25]).astype(F)
    we = (R.standard_normal((1, DIST_D, DIST_HN)) * .05).astype(F)
    wd = (R.standard_normal((1, DIST_D, DIST_HN)) * .02).astype(F)
    return np.ascontiguousarray(np.broadcast_to(row, (DIST_N, row.size))), we, wd


def exact_restricted(bias_row, we, wd, cap=1):
    """pi(v) = q(v) 1[E] / Z over the 2^D vectors, float64: q the NADE's ancestral distribution at temperature 1, E "at most `cap` ones" (one
    counter, nothing given: no free 1 past the cap).  -> pi [2^D] indexed by sum_i v_i 2^i."""
    D, Hn = we.shape
    be, bd = bias_row[:Hn].astype(np.float64), bias_row[Hn:Hn + D].astype(np.float64)
    we, wd = we.astype(np.float64), wd.astype(np.float64)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    q = np.zeros(1 << D)
    for code in range(1 << D):
        a, lq = be.copy(), 0.0
        for i in range(D):
            p = sig(bd[i] + sig(a) @ wd[i])
            on = (code >> i) & 1
            lq += np.log(p if on else 1.0 - p)
            if on:
                a += we[i]
        q[code] = np.exp(lq)
    assert abs(q.sum() - 1.0) < 1e-9
    allowed = np.array([bin(c).count("1") <= cap for c in range(1 << D)])
    pi = np.where(allowed, q, 0.0)
    return pi / pi.sum()


def outcome_counts(samples):
    """samples u8 [N, D] -> counts [2^D] of the codes sum_i v_i 2^i."""
    codes = (samples.astype(np.int64) << np.arange(samples.shape[1])).sum(1)
    return np.bincount(codes, minlength=1 << samples.shape[1])


def sigma_excess(counts, pi, N):
    """Per allowed outcome |n_v - N pi_v| / sqrt(N pi_v (1 - pi_v)) (the others: nan)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(pi > 0, np.abs(counts - N * pi) / np.sqrt(N * pi * (1 - pi)), np.nan)
