"""Matrix-core NADE forward (Hn = 256) with the sparse side owned by rows: wave w of a workgroup executes the flips of rows 8w .. 8w+7 only,
for all 256 hidden units (a lane holds four), keeps their pre-activations and fetches their w_enc rows a tile ahead (a fixed number P per
wave and tile, the rest in place); flip slots are row-major, every wave derives its own list entries from the ballots of its rows.

Both forms run on every case.  The split-operand form (`nade_logprob_fwd_auto(..., gate=None, dense_above=1.0, exact=True)`) is compared
with the float64 oracle at the tolerances of test_gpu_kernels.py::test_nade_mfma_exact_forward_vs_oracle (conditionals 1e-5 absolute,
per-row NLL 2e-5 relative, d nll / d b_dec 1e-4 of its scale, a_final 1e-4 absolute); the bf16 form with the f32 vector kernel
(`nade_logprob_fwd`) at those of test_nade_mfma_forward_matches_f32_kernel.  Every launch is repeated and must be bit-equal.

The cases are the smallest at which the ownership can go wrong: a second workgroup with one valid row and a tail tile of 8 columns; one
wave owning every flip of the workgroup (the first wave, the last wave); a wave with 0, 1, ..., 20 flips in one tile (every prefetch depth
up to 20 is crossed, alone and with the other waves busy); a chunk boundary of the 32-slot flip tile inside the flips of a workgroup, with
a later row's flips in the second chunk; all cells set (32 chunks per tile); no cell set; two tracks at a bias pitch off the 16-byte grid;
a compacted ragged batch with a partly valid and an all-padding workgroup."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nade as onade   # noqa: E402

DEV = "cuda:0"
F8 = np.float64
Hn = 256


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


def bernoulli(seed, tracks, N, D, rho):
    return (np.random.default_rng(seed).random((tracks, N, D)) < rho).astype(np.uint8)


def one_wave(first_row):
    """N = 32, D = 64: the eight rows from `first_row` drawn at rho = 0.5, every other row zero."""
    v = np.zeros((1, 32, 64), np.uint8)
    v[0, first_row:first_row + 8] = bernoulli(first_row + 1, 1, 8, 64, 0.5)[0]
    return v


def depth_ladder(others):
    """N = 32, D = 672: tile k (k = 0..20) has exactly k flips in rows 0-7, dealt round-robin over the rows at distinct columns; with
    `others`, every other wave has 3 flips per tile in its rows as well."""
    v = np.zeros((1, 32, 672), np.uint8)
    for k in range(21):
        for t in range(k):
            v[0, t % 8, 32 * k + t] = 1
        if others:
            for w in (1, 2, 3):
                for i, r in enumerate((0, 3, 7)):
                    v[0, 8 * w + r, 32 * k + (5 * w + 11 * i + k) % 32] = 1
    assert all(int(v[0, :8, 32 * k:32 * k + 32].sum()) == k for k in range(21))
    return v


def chunk_boundary():
    """N = 32, D = 65: row 3 all ones, row 20 ones in columns 0..9 -- tile 0 has 42 flips, row 20's lie in the second chunk."""
    v = np.zeros((1, 32, 65), np.uint8)
    v[0, 3, :] = 1
    v[0, 20, :10] = 1
    assert int(v[0, :, :32].sum()) == 42
    return v


# name -> (v [tracks, N, D], n_rows of a compacted batch or None)
CASES = {
    "second_workgroup_one_row_tail_8": lambda: (bernoulli(1, 1, 33, 40, 0.03), None),
    "two_workgroups_14_tiles": lambda: (bernoulli(2, 1, 64, 440, 0.03), None),
    "first_wave_owns_every_flip": lambda: (one_wave(0), None),
    "last_wave_owns_every_flip": lambda: (one_wave(24), None),
    "prefetch_depths_0_to_20_alone": lambda: (depth_ladder(False), None),
    "prefetch_depths_0_to_20_others_busy": lambda: (depth_ladder(True), None),
    "chunk_boundary_inside_a_row": lambda: (chunk_boundary(), None),
    "all_ones_32_chunks": lambda: (bernoulli(6, 1, 40, 65, 1.0), None),
    "no_flip": lambda: (bernoulli(7, 1, 5, 440, 0.0), None),
    "two_tracks": lambda: (bernoulli(8, 2, 33, 31, 0.5), None),
    "compacted_rows": lambda: (bernoulli(9, 1, 96, 70, 0.1), 40),
}
_shared = {}


def case(name):
    """Inputs and the float64 reference of a case: computed once, shared by the two tests, left unchanged."""
    if name not in _shared:
        v, n_rows = CASES[name]()
        tracks, N, D = v.shape
        R = np.random.default_rng(N * 1000 + D)
        ld = tracks * (Hn + D)
        bias = (R.standard_normal((N, ld)) * .5).astype(np.float32)
        we = (R.standard_normal((tracks, D, Hn)) * .1).astype(np.float32)
        wd = (R.standard_normal((tracks, D, Hn)) * .1).astype(np.float32)
        rw = R.random(N).astype(np.float32)
        ref = []
        for m in range(tracks):
            be = bias[:, m * Hn:(m + 1) * Hn].astype(F8)
            bd = bias[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D].astype(F8)
            vm = v[m].astype(F8)
            n_ref, c_ref = onade.log_prob(vm, be, bd, we[m].astype(F8), wd[m].astype(F8))
            g = onade.log_prob_bwd(vm, be, bd, we[m].astype(F8), wd[m].astype(F8), rw.astype(F8))
            ref.append((n_ref, c_ref, g[1], be + vm @ we[m].astype(F8)))
        _shared[name] = (v, n_rows, bias, we, wd, rw, ref)
    return _shared[name]


def outputs(tracks, N, D, ld, fill):
    f = lambda *s: torch.full(s, fill, device=DEV)
    return f(tracks, N), f(tracks, N, D), f(N, ld), f(tracks, N, Hn)


def padding_is_zero(n_rows, tracks, D, nll, db):
    """Workgroups of 32 rows that lie wholly behind the compacted batch's valid rows write zeros: NLL and the decoder part of d_bias."""
    first = -(-n_rows // 32) * 32
    assert first < nll.shape[1]
    assert float(nll[:, first:].abs().max()) == 0.0
    assert float(db[first:, tracks * Hn: tracks * (Hn + D)].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_split_form_vs_oracle(ops, name):
    v, n_rows, bias, we, wd, rw, ref = case(name)
    tracks, N, D = v.shape
    ld = bias.shape[1]
    wpk = torch.empty((tracks * D, Hn), device=DEV)
    ops.nade_f32_pack(dev(wd).view(tracks * D, Hn), wpk)
    nr = None if n_rows is None else torch.tensor([n_rows], device=DEV, dtype=torch.int32)
    args = (dev(v), dev(bias), dev(we), dev(wd), wpk.view(tracks, D, Hn), tracks, D, Hn, None, None, 1.0, dev(rw))
    nll, cp, db, af = outputs(tracks, N, D, ld, 7.0)
    ops.nade_logprob_fwd_auto(*args, nll, cp, db, af, exact=True, n_rows_dev=nr)
    nll2, cp2, db2, af2 = outputs(tracks, N, D, ld, 7.0)
    ops.nade_logprob_fwd_auto(*args, nll2, cp2, db2, af2, exact=True, n_rows_dev=nr)
    lim = N if n_rows is None else n_rows
    for m in range(tracks):
        n_ref, c_ref, db_ref, a_ref = ref[m]
        e_cp = np.abs(cp[m].cpu().numpy()[:lim] - c_ref[:lim]).max()
        e_nll = np.abs(nll[m].cpu().numpy()[:lim] - n_ref[:lim]).max() / np.abs(n_ref[:lim]).max()
        e_db = rel(db.cpu().numpy()[:lim, tracks * Hn + m * D: tracks * Hn + (m + 1) * D], db_ref[:lim])
        e_af = np.abs(af[m].cpu().numpy()[:lim] - a_ref[:lim]).max()
        print(f"\n[split {name} track {m}] cond_p abs {e_cp:.2e}  nll rel {e_nll:.2e}  d b_dec rel {e_db:.2e}  a_final abs {e_af:.2e}")
        assert e_cp < 1e-5 and e_nll < 2e-5
        assert e_db < 1e-4
        assert e_af < 1e-4
    if n_rows is not None:
        padding_is_zero(n_rows, tracks, D, nll, db)
    for a, b in ((nll, nll2), (cp, cp2), (db, db2), (af, af2)):
        assert torch.equal(a, b)                         # deterministic (untouched cells keep the fill in both)


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_form_vs_f32_kernel(ops, name):
    v, n_rows, bias, we, wd, rw, _ = case(name)
    tracks, N, D = v.shape
    ld = bias.shape[1]
    nr = None if n_rows is None else torch.tensor([n_rows], device=DEV, dtype=torch.int32)
    vt, bt, wet, wdt, rwt = dev(v), dev(bias), dev(we), dev(wd), dev(rw)
    nll0, cp0, db0, af0 = outputs(tracks, N, D, ld, 0.0)
    ops.nade_logprob_fwd(vt, bt, wet, wdt, tracks, D, Hn, rwt, nll0, cp0, db0, af0, n_rows_dev=nr)
    args = (vt, bt, wet, wdt, wdt.to(torch.bfloat16), tracks, D, Hn, None, None, 1.0, rwt)
    nll1, cp1, db1, af1 = outputs(tracks, N, D, ld, 7.0)
    ops.nade_logprob_fwd_auto(*args, nll1, cp1, db1, af1, n_rows_dev=nr)
    nll2, cp2, db2, af2 = outputs(tracks, N, D, ld, 7.0)
    ops.nade_logprob_fwd_auto(*args, nll2, cp2, db2, af2, n_rows_dev=nr)
    lim = N if n_rows is None else n_rows
    dec = slice(tracks * Hn, tracks * (Hn + D))
    e_cp = float((cp0[:, :lim] - cp1[:, :lim]).abs().max())
    e_db = float((db0[:lim, dec] - db1[:lim, dec]).abs().max())
    print(f"\n[bf16 {name}] cond_p abs {e_cp:.2e}  d b_dec abs {e_db:.2e}  nll abs {float((nll0[:, :lim] - nll1[:, :lim]).abs().max()):.2e}"
          f"  a_final abs {float((af0[:, :lim] - af1[:, :lim]).abs().max()):.2e}")
    assert e_cp < 1.5e-2
    assert torch.allclose(nll0[:, :lim], nll1[:, :lim], rtol=5e-3, atol=5e-2)
    assert e_db < 1.5e-2
    assert torch.allclose(af0[:, :lim], af1[:, :lim], rtol=1e-5, atol=1e-5)
    if n_rows is not None:
        padding_is_zero(n_rows, tracks, D, nll1, db1)
    for a, b in ((nll1, nll2), (cp1, cp2), (db1, db2), (af1, af2)):
        assert torch.equal(a, b)                         # deterministic
