"""Reference of the NADE importance estimator (mnn_nade_given_is; DESIGN.md section 4 "NADE importance estimator"); no device.

A particle is a row of the deterministic checker det.nade_sample on the Philox uniforms of its counters (stream 11 without data, 12 with;
row id, sub = particle, elem = m D + i) with test_gpu_conditional.clamp_u's clamp at the given cells; particle 0 of the upper side is
clamped to the data everywhere and reads no uniform.  log w = sum over the given cells of log(1e-6 + q) in float64 from the checker's
float32 conditionals (1 - p in float32, as the kernels form it); log p^, ESS and the standard error in float64.  exact_log_pg: log p(x_G)
by enumeration of the free cells with the float64 oracle."""
import itertools

import numpy as np

from oracle import det, nade as onade, philox
from test_gpu_conditional import clamp_u

FREE = 255
STREAM_IS, STREAM_IS_DATA = 11, 12


def split_bias(bias, tracks, m, D, Hn):
    """(b_enc, b_dec) of track m in the Dense output layout of mnn_nade_sample."""
    return bias[:, m * Hn:(m + 1) * Hn], bias[:, tracks * Hn + m * D:tracks * Hn + (m + 1) * D]


def particles(bias, w_enc, w_dec, tracks, m, D, Hn, codes, data, C, seed, row_ids):
    """The C particles of every row of track m: codes u8 [N, D] (0 / 1 given, 255 free), data None (lower side) or u8 [N, D] (upper side),
    row_ids [N] -> (v u8 [N, C, D], log_w float64 [N, C])."""
    N = bias.shape[0]
    rows = np.asarray(row_ids, np.uint32)
    u = philox.uniform(seed, STREAM_IS if data is None else STREAM_IS_DATA, rows[:, None, None], np.arange(C, dtype=np.uint32)[None, :, None],
                       (m * D + np.arange(D, dtype=np.uint32))[None, None, :])
    held = np.broadcast_to(codes[:, None, :], (N, C, D)).copy()
    if data is not None:
        held[:, 0] = np.where(codes != FREE, codes, (data != 0).astype(np.uint8))        # particle 0: the data's free cells, no uniform
    u = clamp_u(u, held).reshape(N * C, D)
    s, p = det.nade_sample(np.repeat(bias, C, axis=0), w_enc[m], w_dec[m], tracks, m, D, Hn, 1.0, u)
    q = np.where(s > 0, p, np.float32(1.0) - p).astype(np.float64)
    given = np.repeat(codes != FREE, C, axis=0)
    log_w = np.where(given, np.log(1e-6 + q), 0.0).sum(1)
    assert np.array_equal(s[given], np.repeat(codes, C, axis=0)[given])
    return s.reshape(N, C, D), log_w.reshape(N, C)


def reduce_particles(log_w):
    """log_w float64 [N, C] -> (log p^ = logsumexp_c - log C, ESS = (sum w)^2 / sum w^2, standard error of log p^ by the delta method on the
    mean of w: sqrt((C / ESS - 1) / (C - 1)), inf with one particle) -- mnn_rbm_ais's formulas."""
    C = log_w.shape[1]
    m = log_w.max(1)
    e = np.exp(log_w - m[:, None])
    a, b = e.sum(1), (e * e).sum(1)
    ess = a * a / b
    se = np.sqrt(np.maximum(C / ess - 1.0, 0.0) / (C - 1)) if C > 1 else np.full(len(m), np.inf)
    return m + np.log(a) - np.log(C), ess, se


def estimate(bias, w_enc, w_dec, tracks, m, D, Hn, codes, data, C, seed, row_ids):
    """-> (v, log_w, log_pg, ess, stderr) of track m."""
    v, log_w = particles(bias, w_enc, w_dec, tracks, m, D, Hn, codes, data, C, seed, row_ids)
    return (v, log_w) + reduce_particles(log_w)


def exact_log_pg(b_enc, b_dec, w_enc, w_dec, codes):
    """log p(x_G) per row by enumeration of its free cells (at most 12), float64: logsumexp over the free configurations of -NLL(x) of the
    float64 oracle.  b_enc [N, Hn], b_dec [N, D], w_enc / w_dec [D, Hn], codes u8 [N, D]."""
    b_enc, b_dec, w_enc, w_dec = (np.asarray(a, np.float64) for a in (b_enc, b_dec, w_enc, w_dec))
    out = np.empty(codes.shape[0])
    for n in range(codes.shape[0]):
        free = np.flatnonzero(codes[n] == FREE)
        assert len(free) <= 12
        x = np.tile((codes[n] == 1).astype(np.float64), (2 ** len(free), 1))
        if len(free):
            x[:, free] = np.array(list(itertools.product([0.0, 1.0], repeat=len(free))))
        nll, _ = onade.log_prob(x, np.tile(b_enc[n], (len(x), 1)), np.tile(b_dec[n], (len(x), 1)), w_enc, w_dec)
        t = -nll
        out[n] = t.max() + np.log(np.exp(t - t.max()).sum())
    return out


def model_rows(R, b_enc, b_dec, w_enc, w_dec):
    """One vector per row drawn from the model itself (float64 ancestral sampling on R's uniforms) -> u8 [N, D]."""
    b_enc, b_dec, w_enc, w_dec = (np.asarray(a, np.float64) for a in (b_enc, b_dec, w_enc, w_dec))
    x, _ = onade.sample(b_enc, b_dec, w_enc, w_dec, u=R.random(b_dec.shape))
    return x.astype(np.uint8)


# the toy of the direction-of-bias check: D = 10, Hn = 8, weights N(0, 2^2), cells {2, 5, 6, 9} given, two particles
TOY_D, TOY_HN, TOY_GIVEN = 10, 8, (2, 5, 6, 9)


def toy_problem(n_rows, w_scale, seed):
    """(bias f32 [n, Hn + D], w_enc, w_dec f32 [1, D, Hn], x u8 [n, D] drawn from the model, codes u8 [n, D]: x at TOY_GIVEN, 255 elsewhere)."""
    R = np.random.default_rng(seed)
    D, Hn = TOY_D, TOY_HN
    w_enc = (R.standard_normal((1, D, Hn)) * w_scale).astype(np.float32)
    w_dec = (R.standard_normal((1, D, Hn)) * w_scale).astype(np.float32)
    bias = R.standard_normal((n_rows, Hn + D)).astype(np.float32)
    b_enc, b_dec = split_bias(bias, 1, 0, D, Hn)
    x = model_rows(R, b_enc, b_dec, w_enc[0], w_dec[0])
    codes = np.full((n_rows, D), FREE, np.uint8)
    codes[:, list(TOY_GIVEN)] = x[:, list(TOY_GIVEN)]
    return bias, w_enc, w_dec, x, codes


def paired_margin(a, b):
    """Mean of a - b in standard errors of the paired differences."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return d.mean() / (d.std(ddof=1) / np.sqrt(len(d)))
