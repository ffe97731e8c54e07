"""The one launch path of the RBM Gibbs chain (csrc/rbm_chain.h), anchored to the deterministic checker where "grouped equals single" would
compare the launch template with itself: the stepped single chain, the grouped launch in the streaming and matrix-core forms (free, clamped
and with one temperature per job, in both addressings), and the edge shapes N = 1 and M = 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_conditional_rbm as TC   # noqa: E402
import test_gpu_multirbm as TR   # noqa: E402
from test_gpu_temperature import inv, set_form   # noqa: E402
from oracle import det, generators as G   # noqa: E402

DEV = "cuda:0"
FREE = 255
STREAM = {"MNN_RBM_STREAM_W": "1", "MNN_RBM_NO_MFMA": "1"}      # (test_gpu_temperature.RBM_FORMS)
NO_LDS = {"MNN_RBM_STREAM_W": "1"}      # N = 65, D = 88, Hn = 256 is a shape of the LDS form: without it, the next form, the matrix cores

dev = TR.dev


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


# form, N, D, Hn, broadcast bias row, switches
SINGLE_FORMS = [("lds", 5, 30, 20, True, {}), ("stream", 13, 30, 20, False, STREAM), ("mfma", 33, 300, 100, False, {})]


@pytest.mark.parametrize("form,N,D,Hn,bcast,env", SINGLE_FORMS)
@pytest.mark.parametrize("k", [0, 1, 4])
@pytest.mark.parametrize("with_row_ids", [False, True])
def test_stepped_single_chain_against_the_checker(ops, monkeypatch, form, N, D, Hn, bcast, env, k, with_row_ids):
    """seed_step = [5] on the device is seed + 5 on the host, and both are the checker on the uniforms of seed + 5."""
    seed = 40 + k
    R, W, bh, bv, v0 = TC.rbm_problem(N, D, Hn, bcast, N + k)
    rows = (R.permutation(4 * N)[:N] + 1000).astype(np.int32) if with_row_ids else np.arange(700, 700 + N)
    kw = dict(row_ids=dev(rows), sub0=2) if with_row_ids else dict(row0=700, sub0=2)
    args = (dev(v0), dev(W), dev(bh), dev(bv), k)
    set_form(monkeypatch, env)
    p_s, v_s = TC.run_gibbs(ops, *args, seed=seed, seed_step=torch.tensor([5], device=DEV, dtype=torch.int32), **kw)
    p_h, v_h = TC.run_gibbs(ops, *args, seed=seed + 5, **kw)
    set_form(monkeypatch, {})
    u_h, u_v = G.gibbs_uniforms(seed + 5, rows, k, Hn, D, sub0=2)
    p_ref, v_ref = det.rbm_gibbs(v0, W, bh, bv, k, u_h, u_v)
    assert torch.equal(v_s, v_h) and torch.equal(p_s, p_h), form
    assert np.array_equal(v_s.cpu().numpy(), v_ref) and np.array_equal(p_s.cpu().numpy(), p_ref), form


def checker_jobs(x, W, out, M, D, Hn, k, seed, rows, sub0, codes, temps):
    """The checker's (p_v [M, N, D], v [M, N, D]) of the M chains of a composer-layout batch: clamped by `codes`, job m at the power of two
    temps[m] (the checker at temperature 1 on parameters times 1 / temps[m])."""
    ps, vs = [], []
    for m in range(M):
        u_h, u_v = G.gibbs_uniforms(seed + m, rows, k, Hn, D, sub0=sub0)
        s = inv(temps[m])
        c = np.full(x[:, m::M].shape, FREE, np.uint8) if codes is None else codes[:, m::M]
        p, v = TC.clamped_gibbs(x[:, m::M], W[m] * s, out[:, m * Hn:(m + 1) * Hn] * s, out[:, M * Hn + m * D:M * Hn + (m + 1) * D] * s, k, u_h, u_v, c)
        ps.append(p); vs.append(v)
    return np.stack(ps), np.stack(vs)


TEMPS = (0.5, 1.0, 2.0, 4.0, 0.25, 1.0, 2.0, 0.5)
GROUPED_FORMS = [("stream", 13, 30, 20, 3, STREAM), ("mfma", 33, 300, 100, 2, {}), ("mfma", 65, 88, 256, 8, NO_LDS)]


@pytest.mark.parametrize("form,N,D,Hn,M,env", GROUPED_FORMS)
@pytest.mark.parametrize("variant", ["free", "given", "temps"])
def test_grouped_chain_against_the_checker_streaming_and_matrix_cores(ops, monkeypatch, form, N, D, Hn, M, env, variant):
    k, seed = 3, 31
    R, W, out, x = TR.multi_problem(N, D, Hn, M, False, N + M)
    W_d, out_d, x_d = dev(W), dev(out), dev(x)
    bh, bv = TR.bias_views(out_d, M, D, Hn)
    codes = TC.random_codes(R, (N, D * M), 0.4) if variant == "given" else None
    temps = TEMPS[:M] if variant == "temps" else (1.0,) * M
    kw = dict(temperature=temps) if variant == "temps" else {}
    p_ref, v_ref = checker_jobs(x, W, out, M, D, Hn, k, seed, np.arange(300, 300 + N), 2, codes, temps)
    for es in (M, 1):
        set_form(monkeypatch, env)
        p_v, v = TR.grouped_launch(ops, x_d, W_d, bh, bv, k, seed, es, given=None if codes is None else dev(codes), row0=300, sub0=2, **kw)
        set_form(monkeypatch, {})
        assert np.array_equal(v.cpu().numpy(), v_ref), (form, es)
        assert np.array_equal(p_v.cpu().numpy(), p_ref), (form, es)


@pytest.mark.parametrize("N,D,Hn,M,env", [(1, 30, 20, 3, {}), (1, 30, 20, 3, STREAM), (1, 300, 100, 2, {}), (1, 88, 256, 1, {}), (5, 30, 20, 1, {}),
                                          (33, 300, 100, 1, {})])
@pytest.mark.parametrize("with_given", [False, True])
def test_one_row_and_one_job(ops, monkeypatch, N, D, Hn, M, env, with_given):
    """N = 1 (a row stride means nothing there: ops.rbm_gibbs_multi passes one the library accepts) and M = 1, single and grouped: the
    grouped launch, the single launches and the checker agree."""
    k, seed = 2, 17
    R, W, out, x = TR.multi_problem(N, D, Hn, M, False, 3 * N + M)
    W_d, out_d, x_d = dev(W), dev(out), dev(x)
    bh, bv = TR.bias_views(out_d, M, D, Hn)
    codes = TC.random_codes(R, (N, D * M), 0.4) if with_given else None
    g_d = None if codes is None else dev(codes)
    p_ref, v_ref = checker_jobs(x, W, out, M, D, Hn, k, seed, np.arange(9, 9 + N), 1, codes, (1.0,) * M)
    set_form(monkeypatch, env)
    res = [TR.single_launches(ops, x_d, W_d, bh, bv, k, seed, given=g_d, row0=9, sub0=1)]
    res += [TR.grouped_launch(ops, x_d, W_d, bh, bv, k, seed, es, given=g_d, row0=9, sub0=1) for es in sorted({1, M})]
    set_form(monkeypatch, {})
    for p_v, v in res:
        assert np.array_equal(v.cpu().numpy(), v_ref) and np.array_equal(p_v.cpu().numpy(), p_ref)
