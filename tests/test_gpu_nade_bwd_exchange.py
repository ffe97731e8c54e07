"""NADE backward (`mnn_nade_logprob_bwd`, hidden widths above 64): the cross-wave exchange sends a wave's d w_enc partial only for the
visibles at which one of the wave's 8 rows flips, behind a flag word per wave; the summing wave adds the flagged partials and sends no
atomics where there are none.  Every case runs the backward after the matching forward and checks d w_enc, d w_dec and d b_enc against
the float64 oracle at the 1e-4 (relative to the largest entry) of test_gpu_kernels.py::test_nade_logprob_fwd_bwd.  The shapes are the
smallest at which the new paths differ: rows off the 64 / 8 grid, D off the 8-visible chunk, one and two hidden slices, a partial slice,
several tracks, no flip at all, flips everywhere, exactly one flip, the multiplicative instantiation, a compacted ragged batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nade as onade   # noqa: E402

DEV = "cuda:0"
F8 = np.float64


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    a, b = np.asarray(a, F8), np.asarray(b, F8)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def inputs(N, D, Hn, tracks, seed, w_scale=0.3):
    R = np.random.default_rng(seed)
    ld = tracks * (Hn + D) + 3
    bias = (R.standard_normal((N, ld)) * .5).astype(np.float32)
    we = (R.standard_normal((tracks, D, Hn)) * w_scale).astype(np.float32)
    wd = (R.standard_normal((tracks, D, Hn)) * w_scale).astype(np.float32)
    rw = (R.random(N).astype(np.float32) + 0.5) / N
    return R, bias, we, wd, rw


def run(ops, v, bias, we, wd, rw, n_rows=None, gated=False, repeat=1):
    """forward, then `repeat` backward calls on the forward's results -> [(d w_enc, d w_dec, d bias)], all numpy."""
    tracks, N, D = v.shape
    Hn = we.shape[2]
    vt, bt, wet, wdt = dev(v), dev(bias), dev(we), dev(wd)
    d0 = torch.zeros_like(bt)
    a_fin = torch.zeros((tracks, N, Hn), device=DEV)
    nll = torch.zeros((tracks, N), device=DEV)
    nr = None if n_rows is None else torch.tensor([n_rows], device=DEV, dtype=torch.int32)
    word = None
    if gated:                     # the density-gated dense forward leaves 0 in `unsafe`: the backward then takes the multiplicative form
        word = torch.full((1,), 7, device=DEV, dtype=torch.int32)
        ops.nade_logprob_fwd(vt, bt, wet, wdt, tracks, D, Hn, dev(rw), nll, None, d0, a_fin, n_rows_dev=nr,
                             gate=torch.tensor([1], device=DEV, dtype=torch.int32), run_if=1, unsafe=word)
        assert int(word) == 0, int(word)
    else:
        ops.nade_logprob_fwd(vt, bt, wet, wdt, tracks, D, Hn, dev(rw), nll, None, d0, a_fin, n_rows_dev=nr)
    out = []
    for _ in range(repeat):
        db = d0.clone()
        dwe = torch.zeros((tracks, D, Hn), device=DEV)
        dwd = torch.zeros((tracks, D, Hn), device=DEV)
        ops.nade_logprob_bwd(vt, bt, wet, wdt, tracks, D, Hn, a_fin, db, dwe, dwd, n_rows_dev=nr, unsafe=word)
        out.append((dwe.cpu().numpy(), dwd.cpu().numpy(), db.cpu().numpy()))
    return out


def oracle(v, bias, we, wd, rw, rows=None):
    """[(d b_enc, d w_enc, d w_dec)] per track from the float64 oracle, over the first `rows` rows."""
    tracks, N, D = v.shape
    Hn = we.shape[2]
    n = N if rows is None else rows
    ref = []
    for m in range(tracks):
        be = bias[:n, m * Hn:(m + 1) * Hn].astype(F8)
        bd = bias[:n, tracks * Hn + m * D: tracks * Hn + (m + 1) * D].astype(F8)
        g = onade.log_prob_bwd(v[m, :n].astype(F8), be, bd, we[m].astype(F8), wd[m].astype(F8), rw[:n].astype(F8))
        ref.append((g[0], g[2], g[3]))
    return ref


def check(got, ref, Hn, rows=None, what=""):
    dwe, dwd, db = got
    for m, (g_be, g_we, g_wd) in enumerate(ref):
        n = db.shape[0] if rows is None else rows
        errs = (rel(dwe[m], g_we) if np.abs(g_we).max() > 0 else float(np.abs(dwe[m]).max()), rel(dwd[m], g_wd),
                rel(db[:n, m * Hn:(m + 1) * Hn], g_be))
        print(f"\n[nade bwd exchange {what} track {m}] d w_enc {errs[0]:.2e}  d w_dec {errs[1]:.2e}  d b_enc {errs[2]:.2e}")
        assert errs[0] < 1e-4 and errs[1] < 1e-4 and errs[2] < 1e-4, errs


@pytest.mark.parametrize("N,D,Hn,tracks", [(70, 13, 256, 1), (64, 16, 96, 1), (128, 88, 128, 5)])
def test_sparse_batch_against_oracle(ops, N, D, Hn, tracks):
    R, bias, we, wd, rw = inputs(N, D, Hn, tracks, 100 * N + D)
    v = (R.random((tracks, N, D)) < 0.03).astype(np.uint8)
    assert v.any()
    (got,) = run(ops, v, bias, we, wd, rw)
    check(got, oracle(v, bias, we, wd, rw), Hn, what=f"N={N} D={D} Hn={Hn} tracks={tracks} rho=0.03")


def test_no_flip_sends_no_encoder_gradient(ops):
    N, D, Hn = 64, 16, 256
    _, bias, we, wd, rw = inputs(N, D, Hn, 1, 1)
    v = np.zeros((1, N, D), np.uint8)
    (got,) = run(ops, v, bias, we, wd, rw)
    assert not got[0].any()                                  # every exchange and every atomic of d w_enc is skipped: exactly zero
    check(got, oracle(v, bias, we, wd, rw), Hn, what="v = 0")


def test_all_flip_skips_nothing(ops):
    N, D, Hn = 64, 16, 256
    _, bias, we, wd, rw = inputs(N, D, Hn, 1, 2)
    v = np.ones((1, N, D), np.uint8)
    (got,) = run(ops, v, bias, we, wd, rw)
    check(got, oracle(v, bias, we, wd, rw), Hn, what="v = 1")


def test_single_flip_reaches_its_row_only(ops):
    N, D, Hn = 64, 16, 256
    _, bias, we, wd, rw = inputs(N, D, Hn, 1, 3)
    v = np.zeros((1, N, D), np.uint8)
    v[0, 19, 5] = 1                                          # wave 2 flips at visible 5 (second half-chunk, k = 1): one flag bit in all
    (got,) = run(ops, v, bias, we, wd, rw)
    ref = oracle(v, bias, we, wd, rw)
    check(got, ref, Hn, what="one 1 at (19, 5)")
    assert rel(got[0][0, 5], ref[0][1][5]) < 1e-4 and np.abs(ref[0][1][5]).max() > 0
    others = np.delete(got[0][0], 5, axis=0)
    assert not others.any()                                  # every other row of d w_enc: exactly zero


def test_dense_batch_multiplicative_instantiation(ops):
    N, D, Hn = 128, 32, 256
    R, bias, we, wd, rw = inputs(N, D, Hn, 1, 4)
    v = (R.random((1, N, D)) < 0.5).astype(np.uint8)
    (got,) = run(ops, v, bias, we, wd, rw, gated=True)
    check(got, oracle(v, bias, we, wd, rw), Hn, what="rho=0.5, multiplicative form")


def test_compacted_ragged_batch(ops):
    N, D, Hn, valid = 128, 16, 256, 70
    R, bias, we, wd, rw = inputs(N, D, Hn, 1, 5)
    v = (R.random((1, N, D)) < 0.03).astype(np.uint8)
    v[0, valid:] = (R.random((N - valid, D)) < 0.5)          # padding rows carry set cells: they must contribute nothing
    rw[valid:] = 0.0                                         # (the row weight of a padding row is 0)
    (got,) = run(ops, v, bias, we, wd, rw, n_rows=valid)
    check(got, oracle(v, bias, we, wd, rw, rows=valid), Hn, rows=valid, what="n_rows_dev=70 of N=128")
    assert not got[2][valid:, :Hn].any()                     # d b_enc of the padding rows


def test_single_workgroup_is_bit_reproducible(ops):
    """N <= 64: one workgroup per hidden slice, so every address of d w_enc receives exactly ONE atomic and two runs agree bit for bit; a
    race on the flag words (a summing wave reading a flag of the other exchange) shows as a difference."""
    N, D, Hn = 50, 24, 256
    R, bias, we, wd, rw = inputs(N, D, Hn, 1, 6)
    v = (R.random((1, N, D)) < 0.1).astype(np.uint8)
    a, b = run(ops, v, bias, we, wd, rw, repeat=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check(a, oracle(v, bias, we, wd, rw), Hn, what="N=50 one workgroup per slice")
