"""Reference of NADE importance resampling (mnn_nade_sample_sir_at; DESIGN.md section 4 "NADE importance resampling"); no device.

A scan is one (row, track).  Particle 0 is a row of the deterministic checker det.nade_sample on the uniforms of the plain sampler (Philox
stream 1, row id, sub, elem = m D + i), particle c >= 1 the same on stream 13 at elem (c - 1) E4 + m D + i (E4 = tracks D rounded up to a
multiple of 4), both with clamp_u's clamp at the given cells.  log w = sum over the given cells of log(1e-6 + q) in
float64 from the checker's float32 conditionals AT THE SCAN'S TEMPERATURE, nll = the same sum over all cells from the untempered ones.  The
pick in float64 as the header states it: e_c = exp(log w_c - max), a running sum in the order c = 0 .. C - 1, the smallest c whose running
sum exceeds u total (u: stream 14, row id, sub, elem = track), C - 1 if none.  A scan with no given cell behind a free one is particle 0.

Temperatures are powers of two: the checker has one scalar temperature, and dividing a logit by a power of two is multiplying b_dec and
w_dec by its inverse, exactly (tests/test_gpu_temperature.py), which also hands back the tempered conditionals."""
import functools
import itertools

import numpy as np

from oracle import det, philox
from nade_is_reference import FREE, split_bias

STREAM_SIR, STREAM_PICK = 13, 14
F = np.float32


def clamp_u(u, codes):
    """The uniforms that make det.nade_sample emit the clamped values (as tests/test_gpu_conditional.py's)."""
    return np.where(codes == 1, F(-1.0), np.where(codes == 0, F(2.0), u)).astype(F)


PATTERNS = ["density 0.3", "all free", "all given", "given prefix", "given suffix", "last given mid-row"]


def problem(N, D, Hn, tracks, seed=0):
    """(bias, w_enc, w_dec, codes u8 [tracks, N, D]): the six code patterns on different (row, track) cells of one launch -- the arrays of
    tests/test_gpu_nade_is.py::problem, restated here so that this file needs no GPU test module (the GPU tests compare the two)."""
    R = np.random.default_rng(N * 31 + D + seed)
    bias = (R.standard_normal((N, tracks * (Hn + D))) * .5).astype(F)
    we = (R.standard_normal((tracks, D, Hn)) * .3).astype(F)
    wd = (R.standard_normal((tracks, D, Hn)) * .3).astype(F)
    vals = (R.random((tracks, N, D)) < 0.3).astype(np.uint8)
    codes = np.full((tracks, N, D), FREE, np.uint8)
    k = max(1, D // 3)
    for m in range(tracks):
        for n in range(N):
            kind = PATTERNS[(m * N + n) % len(PATTERNS)]
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
    return bias, we, wd, codes


def e4(tracks, D):
    return (tracks * D + 3) // 4 * 4


def inv_temps(tvec):
    s = F(1.0) / np.asarray(tvec, F)
    assert np.all(s.astype(np.float64) * np.asarray(tvec, np.float64) == 1.0) and np.all(np.frexp(s)[0] == 0.5), "power-of-two temperatures only"
    return s


def uniforms(seed, rows, sub, tracks, m, D, C, c0=0):
    """Particles c0 .. c0 + C - 1 of track m -> f32 [N, C, D]: a particle's uniforms depend on (seed, row id, sub, c, m, i) and E4 alone."""
    rows = np.asarray(rows, np.uint32)
    elem = (m * D + np.arange(D, dtype=np.uint32))[None, None, :]
    out = np.empty((len(rows), C, D), F)
    for k in range(C):
        c = c0 + k
        if c == 0:
            out[:, k] = philox.uniform(seed, philox.STREAM_NADE, rows[:, None], np.uint32(sub), elem[0])
        else:
            out[:, k] = philox.uniform(seed, STREAM_SIR, rows[:, None], np.uint32(sub), np.uint32((c - 1) * e4(tracks, D)) + elem[0])
    return out


def particles(bias, w_enc, w_dec, tracks, m, D, Hn, codes, C, seed, rows, sub, tvec=None, c0=0):
    """The particles c0 .. c0 + C - 1 of every row of track m.  codes u8 [N, D]; tvec None (temperature 1) or the D temperatures of the
    track's visibles -> (v u8 [N, C, D], log_w f64 [N, C], nll f64 [N, C])."""
    N = bias.shape[0]
    u = uniforms(seed, rows, sub, tracks, m, D, C, c0)
    held = np.broadcast_to(codes[:, None, :], (N, C, D))
    u = clamp_u(u, held).reshape(N * C, D)
    big = np.repeat(bias, C, axis=0)
    if tvec is None or np.all(np.asarray(tvec) == 1.0):
        s, p = det.nade_sample(big, w_enc[m], w_dec[m], tracks, m, D, Hn, 1.0, u)
        pt = p
    else:
        sc = inv_temps(tvec)
        big_s, wd_s = big.copy(), w_dec[m] * sc[:, None]
        big_s[:, tracks * Hn + m * D:tracks * Hn + (m + 1) * D] *= sc[None, :]
        s, pt = det.nade_sample(big_s, w_enc[m], wd_s, tracks, m, D, Hn, 1.0, u)                    # the tempered draws and conditionals
        _, p = det.nade_sample(big, w_enc[m], w_dec[m], tracks, m, D, Hn, 1.0, clamp_u(u, s))      # the model's own of the emitted vectors
    given = np.repeat(codes != FREE, C, axis=0)
    assert np.array_equal(s[given], np.repeat(codes, C, axis=0)[given])
    qt = np.where(s > 0, pt, F(1.0) - pt).astype(np.float64)
    q = np.where(s > 0, p, F(1.0) - p).astype(np.float64)
    log_w = np.where(given, np.log(1e-6 + qt), 0.0).sum(1)
    nll = -np.log(1e-6 + q).sum(1)
    return s.reshape(N, C, D), log_w.reshape(N, C), nll.reshape(N, C)


def is_shortcut(codes):
    """[N]: no given cell ordered behind a free one (nothing given, everything given, a given prefix)."""
    D = codes.shape[1]
    free = codes == FREE
    first_free = np.where(free.any(1), free.argmax(1), D)
    last_given = np.where((~free).any(1), D - 1 - (~free)[:, ::-1].argmax(1), -1)
    return last_given < first_free


def pick_uniform(seed, rows, sub, m):
    return philox.uniform(seed, STREAM_PICK, np.asarray(rows, np.uint32), np.uint32(sub), np.uint32(m)).astype(np.float64)


def pick_from(log_w, u):
    """log_w [N, C] (any float dtype), u f64 [N] -> (pick [N], ess [N], near [N]: u total lies within 1e-12 total of a running sum)."""
    lw = np.asarray(log_w, np.float64)
    C = lw.shape[1]
    e = np.exp(lw - lw.max(1, keepdims=True))
    run = np.cumsum(e, axis=1)                                   # serial, in the order c = 0 .. C - 1
    total = run[:, -1]
    thr = u * total
    over = run > thr[:, None]
    pick = np.where(over.any(1), over.argmax(1), C - 1)
    ess = total * total / np.cumsum(e * e, axis=1)[:, -1]
    near = (np.abs(run - thr[:, None]) <= 1e-12 * total[:, None]).any(1)
    return pick, ess, near


def resample(bias, w_enc, w_dec, tracks, m, D, Hn, codes, C, seed, rows, sub, tvec=None, parts=None):
    """One track of a launch -> dict(v, log_w, nll: the particles; shortcut, pick, ess, near [N]; out u8 [N, D], out_nll [N]).  parts: the
    particles if the caller has them (a larger C's first C)."""
    v, log_w, nll = parts if parts is not None else particles(bias, w_enc, w_dec, tracks, m, D, Hn, codes, C, seed, rows, sub, tvec)
    v, log_w, nll = v[:, :C], log_w[:, :C], nll[:, :C]
    sc = is_shortcut(codes)
    pick, ess, near = pick_from(log_w, pick_uniform(seed, rows, sub, m))
    pick, ess, near = np.where(sc, 0, pick), np.where(sc, float(C), ess), near & ~sc
    n = np.arange(len(pick))
    return dict(v=v, log_w=log_w, nll=nll, shortcut=sc, pick=pick, ess=ess, near=near, out=v[n, pick], out_nll=nll[n, pick])


@functools.lru_cache(maxsize=None)
def cached_particles(N, D, Hn, tracks, C, seed, row0, sub, temps_kind="one"):
    """The particles of problem(N, D, Hn, tracks) for every track, computed once: ([(v, log_w, nll)] per track, problem, tvecs).  temps_kind: "one" | "scalar" (0.5) | "track" ((0.5, 1, 2, ..)[m]) | "visible" (t[i % 3] of (0.5, 2, 4))."""
    prob = problem(N, D, Hn, tracks)
    bias, we, wd, codes = prob[:4]
    tv = [temps_vector(temps_kind, tracks, m, D) for m in range(tracks)]
    rows = row0 + np.arange(N)
    return [particles(bias, we, wd, tracks, m, D, Hn, codes[m], C, seed, rows, sub, tv[m]) for m in range(tracks)], prob, tv


TRACK_TEMPS, VISIBLE_TEMPS = (0.5, 1.0, 2.0, 4.0, 0.25, 1.0, 2.0, 0.5), (0.5, 2.0, 4.0)


def temps_argument(kind, tracks):
    """What ops.nade_sample_sir takes as (temperature, by_visible) for a temps_kind."""
    return {"one": (1.0, False), "scalar": (0.5, False), "track": (TRACK_TEMPS[:tracks], False), "visible": (VISIBLE_TEMPS, True)}[kind]


def temps_vector(kind, tracks, m, D):
    if kind == "one":
        return None
    if kind == "scalar":
        return np.full(D, 0.5, F)
    if kind == "track":
        return np.full(D, TRACK_TEMPS[m], F)
    return np.array([VISIBLE_TEMPS[i % len(VISIBLE_TEMPS)] for i in range(D)], F)


# ------------------------------------------------------------------------------------------------
# The toy of the statistical pin: D = 8, Hn = 4; visible 0 switches the hidden units on (w_enc[0] = 6 against b_enc = -3) and visible 7,
# given as 1, reads them (w_dec[7] = 2, b_dec[7] = -4): p(v0 = 1 | v7 = 1) is about 0.975 where the clamped scan draws v0 near 0.5.
TOY_D, TOY_HN, TOY_N, TOY_C = 8, 4, 4096, 64


def toy_problem(seed=0):
    """(bias f32 [TOY_N, Hn + D] -- the same row N times --, w_enc, w_dec f32 [1, D, Hn], codes u8 [N, D]: visible 7 given as 1)."""
    R = np.random.default_rng(seed)
    D, Hn = TOY_D, TOY_HN
    w_enc = (R.standard_normal((1, D, Hn)) * .3).astype(F)
    w_dec = (R.standard_normal((1, D, Hn)) * .3).astype(F)
    b = (R.standard_normal(Hn + D) * .3).astype(F)
    w_enc[0, 0], w_dec[0, 7], b[:Hn], b[Hn + 7] = 6.0, 2.0, -3.0, -4.0
    bias = np.tile(b, (TOY_N, 1))
    codes = np.full((TOY_N, D), FREE, np.uint8)
    codes[:, 7] = 1
    return bias, w_enc, w_dec, codes


def joint_prob(x, b_enc, b_dec, w_enc, w_dec):
    """p(x) of a NADE per row of x [n, D], float64: prod_i p(x_i | x_<i), p(x_i = 1 | x_<i) = sigmoid(b_dec_i + sigmoid(a_i) . w_dec_i),
    a_0 = b_enc, a_{i+1} = a_i + x_i w_enc_i."""
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    a = np.tile(np.asarray(b_enc, np.float64), (len(x), 1))
    prob = np.ones(len(x))
    for i in range(x.shape[1]):
        p1 = sig(b_dec[i] + sig(a) @ w_dec[i])
        prob *= np.where(x[:, i] > 0, p1, 1.0 - p1)
        a = a + x[:, i:i + 1] * w_enc[i][None, :]
    return prob


def toy_exact(bias, w_enc, w_dec):
    """(p = p(v0 = 1 | v7 = 1), rho = E_q[w^2] / E_q[w]^2) by enumeration of the seven free cells in float64; q is the clamped scan's
    proposal, w = p(v7 = 1 | v_<7) its weight."""
    D, Hn = TOY_D, TOY_HN
    b_enc, b_dec = split_bias(bias[:1].astype(np.float64), 1, 0, D, Hn)
    x = np.array(list(itertools.product([0.0, 1.0], repeat=D - 1)))
    x1 = np.concatenate([x, np.ones((len(x), 1))], 1)
    x0 = np.concatenate([x, np.zeros((len(x), 1))], 1)
    we, wd = w_enc[0].astype(np.float64), w_dec[0].astype(np.float64)
    j1, j0 = joint_prob(x1, b_enc[0], b_dec[0], we, wd), joint_prob(x0, b_enc[0], b_dec[0], we, wd)      # p(x_F, v7 = 1), p(x_F, v7 = 0)
    q = j1 + j0                                                  # the proposal: p(x_0 .. x_6)
    w = j1 / q
    p = (j1 * x[:, 0]).sum() / j1.sum()
    rho = (q * w * w).sum() / (q * w).sum() ** 2
    return p, rho


def toy_bound(p, rho, N=TOY_N, C=TOY_C):
    """Four binomial standard errors + the first-order bias rho / C of a self-normalised estimate of a [0, 1] function, doubled for the
    neglected terms."""
    return 4.0 * np.sqrt(p * (1.0 - p) / N) + 2.0 * rho / C
