"""The step's support kernels (elementwise.hip, the CD / axpby group of rbm.hip) at their dtype, view and grid-cap edges.

Every expected value is exact or bounded by a stated derivation:
  conversions : torch's CPU dtype conversion (round to nearest even, as the device stores do), compared as raw words
  reductions  : integer-valued / power-of-two inputs whose f32 sums are exact in any order, compared with ==; single-probe launches
                (one 1.0 among zeros) at the first / last element and at the seams between vector body, scalar tail and second grid pass
  random sums : float64, within sum_bound() = (k + 8 + g) 2^-24 sum|term| worked out from n and the launch geometry
  dropout     : oracle/philox.py, bit-exact
The reference helpers at the top have a CPU self-check (test_reference_helpers_cpu) that runs without a device.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import philox, generators as G
from oracle import tf_semantics as S

gpu = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"u8": torch.uint8, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
U = 2.0 ** -24                                   # unit roundoff of f32


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


# ------------------------------------------------------------------------------------------------
# reference helpers
# ------------------------------------------------------------------------------------------------
def gate_perm(u):
    """perm[g * u + j] = packed (gate-interleaved) column of natural column (gate g, unit j)."""
    g, j = np.divmod(np.arange(4 * u), u)
    return (j // 32) * 128 + g * 32 + j % 32


def gate_perm_inv(u):
    inv = np.empty(4 * u, np.int64)
    inv[gate_perm(u)] = np.arange(4 * u)
    return inv


def pack_np(W, b, n_in, u, ld_in):
    """natural W [(n_in + u), 4u], b [4u] -> wx_t [4u, ld_in] (K padding zero), wh_t [4u, u], wh_p [u, 4u], wx_p [n_in, 4u], bias_p [4u]."""
    Wp = W[:, gate_perm_inv(u)]                  # Wp[:, pc] = W[:, natural column of pc]
    wx_p, wh_p = Wp[:n_in], Wp[n_in:]
    wx_t = np.zeros((4 * u, ld_in), W.dtype)
    wx_t[:, :n_in] = wx_p.T
    return wx_t, np.ascontiguousarray(wh_p.T), np.ascontiguousarray(wh_p), np.ascontiguousarray(wx_p), b[gate_perm_inv(u)]


def unpack_np(dwx_t, dwh_t, db_p, n_in, u):
    """packed gradients -> natural dW [(n_in + u), 4u], db [4u]."""
    p = gate_perm(u)
    return np.concatenate([dwx_t[:, :n_in].T, dwh_t.T], 0)[:, p], db_p[p]


@functools.lru_cache(maxsize=None)
def dropout_uniforms(seed, row0, layer, t, B, u):
    """The uniforms of timestep t (global rows row0 .. row0 + B) of one layer: f32 [B, u].  Computed once per key and shared."""
    a = philox.uniform_block(seed, philox.STREAM_DROPOUT, np.arange(row0, row0 + B), (t << 8) | layer, u)
    a.setflags(write=False)
    return a


def dropout_keep(kp, seed, row0, layer, t, B, u):
    return np.floor(np.float32(kp) + dropout_uniforms(seed, row0, layer, t, B, u))


def dropout_expect(h32, kp, keep):
    """float32(h) / float32(kp) * keep, in f32 (the caller rounds it to the storage type)."""
    return h32.astype(np.float32) / np.float32(kp) * keep.astype(np.float32)


def cpu_cvt(x, dtype):
    """torch's CPU conversion (round to nearest even) of a NumPy array or CPU tensor."""
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.to(dtype)


def raw(t):
    """The words of a tensor, as integers (so that -0 != +0 and NaNs compare)."""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).numpy()


def sum_bound(k, g, abs_sum):
    """Worst-case |f32 sum - exact sum| of the reduction kernels, first order: a term passes through at most k roundings of its thread's
    chain, 8 of the shuffle / LDS tree and g same-word atomics (one per workgroup)."""
    return (k + 8 + g) * U * abs_sum


def sumsq_geometry(n, aligned):
    """(workgroups, float4 elements of the vector body) of mnn_sumsq."""
    return min(256, (n + 1023) // 1024), (n // 4 if aligned else 0)


def chain_len(n, threads, n4=0):
    """longest per-thread chain: 4 per float4 of the body + the grid-stride tail."""
    return 4 * -(-n4 // threads) + -(-(n - 4 * n4) // threads)


def emulate_block_sum(a, b, grid, n4):
    """NumPy emulation of sumsq_kernel (b = a) / wsum_kernel over the terms a[i] * b[i]: per-thread fmaf chains in launch order (the f32
    product of two f32 numbers is exact in float64; each step rounds the sum once, to f32), a 6-level xor butterfly per wave, the four wave
    partials added in order, one f32 add per workgroup into the result."""
    a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    threads = grid * 256
    acc = np.zeros(threads, np.float32)

    def fma(seg_a, seg_b):
        acc[:len(seg_a)] = (acc[:len(seg_a)].astype(np.float64) + seg_a * seg_b).astype(np.float32)
    qa, qb = a[:4 * n4].reshape(-1, 4), b[:4 * n4].reshape(-1, 4)
    for i in range(-(-n4 // threads)):
        for e in range(4):
            fma(qa[i * threads:(i + 1) * threads, e], qb[i * threads:(i + 1) * threads, e])
    ta, tb = a[4 * n4:], b[4 * n4:]
    for i in range(-(-len(ta) // threads)):
        fma(ta[i * threads:(i + 1) * threads], tb[i * threads:(i + 1) * threads])
    w = acc.reshape(-1, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    part = w[:, 0].reshape(grid, 4)
    blk = ((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]
    out = np.float32(0)
    for v in blk:
        out = np.float32(out + v)
    return out


def test_reference_helpers_cpu():
    from test_gpu_kernels import _unperm
    R = np.random.default_rng(0)
    for n_in, u, ld_in in [(12, 32, 16), (17, 96, 24)]:
        W = R.integers(-9, 10, (n_in + u, 4 * u)).astype(np.float32)
        b = R.integers(-9, 10, 4 * u).astype(np.float32)
        wx_t, wh_t, wh_p, wx_p, bias_p = pack_np(W, b, n_in, u, ld_in)
        dW, db = unpack_np(wx_t, wh_t, bias_p, n_in, u)
        assert np.array_equal(dW, W) and np.array_equal(db, b)                      # pack then unpack: identity
        assert np.array_equal(wx_t[:, n_in:], np.zeros((4 * u, ld_in - n_in))) and np.array_equal(wx_p.T, wx_t[:, :n_in])
        assert np.array_equal(_unperm(np.concatenate([wx_p, wh_p], 0), u), W) and np.array_equal(_unperm(bias_p, u), b)
        assert np.array_equal(gate_perm(u)[gate_perm_inv(u)], np.arange(4 * u))
        assert np.array_equal(_unperm(np.arange(4 * u), u), gate_perm(u))
    # dropout helper against the oracle's DropoutWrapper at the shape of test_dropout_matches_contract
    T, B, u = 3, 5, 32
    h = np.random.default_rng(4).standard_normal((T, B, u)).astype(np.float32)
    uu = np.stack([philox.uniform_block(23, philox.STREAM_DROPOUT, np.arange(100, 100 + B), (t << 8) | 1, u) for t in range(T)])
    ref, keep = S.dropout_output(h, 0.9, uu)
    mine_keep = np.stack([dropout_keep(0.9, 23, 100, 1, t, B, u) for t in range(T)])
    assert np.array_equal(mine_keep, keep) and np.array_equal(dropout_expect(h, 0.9, mine_keep), ref)
    # conversion wrapper: ties go to even, 70000 overflows f16, 1e-6 is an f16 subnormal
    x = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 70000.0, 1e-6, -0.0], np.float32)
    assert raw(cpu_cvt(x, torch.float16)).tolist() == [0x3C00, 0x3C02, 0x7C00, 0x0011, -0x8000]
    assert raw(cpu_cvt(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], np.float32), torch.bfloat16)).tolist() == [0x3F80, 0x3F82]
    # the bound covers the f32-vs-f64 error of the emulated summation tree on random data
    for n, aligned in [(5, True), (1023, False), (70001, True), (300001, True), (300001, False)]:
        x = R.standard_normal(n).astype(np.float32) * 3
        terms = x.astype(np.float64) ** 2
        grid, n4 = sumsq_geometry(n, aligned)
        err = abs(float(emulate_block_sum(x, x, grid, n4)) - terms.sum())
        assert err <= sum_bound(chain_len(n, grid * 256, n4), grid, terms.sum()), (n, aligned, err)
    assert chain_len(300001, 256 * 256, 75000) == 9 and chain_len(5, 256, 1) == 5 and chain_len(1023, 256) == 4


# ------------------------------------------------------------------------------------------------
def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV)


# ±0, ties of both 16-bit formats (to even: down and up), the largest finite f16 and the tie above it, overflow, f16 subnormals
SPECIALS = np.array([0.0, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 65504.0, 65520.0, 70000.0, -70000.0,
                     1e-6, -1e-6, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25], np.float32)


def source_matrix(R, C, src, seed):
    """CPU tensor [R, C] of dtype `src`: the special values first (where they fit), seeded random numbers behind."""
    rng = np.random.default_rng(seed)
    if src == "u8":
        x = rng.integers(0, 256, R * C).astype(np.uint8)
        x[:4] = [0, 1, 255, 128][:min(4, R * C)]
        return torch.from_numpy(x.reshape(R, C))
    x = (rng.standard_normal(R * C) * np.exp(rng.uniform(-12, 6, R * C))).astype(np.float32)
    k = min(len(SPECIALS), R * C)
    x[:k] = SPECIALS[:k]
    return torch.from_numpy(x.reshape(R, C)).to(TDT[src])


PAIRS = [(s, d) for s in ("u8", "f32", "bf16", "f16") for d in ("f32", "bf16", "f16")]


@gpu
@pytest.mark.parametrize("src,dst", PAIRS)
def test_transpose_all_dtype_pairs_bit_exact(ops, src, dst):
    """mnn_transpose, all 12 instantiations: full tiles, edge tiles, single row / column; `out` wider than R (padding untouched); `src` a
    column slice at an odd element offset of a wider matrix."""
    for R, C in [(77, 45), (32, 32), (1, 33), (33, 1), (100, 64)]:
        x = source_matrix(R, C, src, seed=R * 131 + C)
        exp = x.to(TDT[dst]).t().contiguous()
        wide = torch.zeros((R, C + 7), dtype=TDT[src])
        wide[:, 3:3 + C] = x
        for xin in (dev(x), dev(wide)[:, 3:3 + C]):
            out = torch.full((C, R + 5), 7.0, device=DEV, dtype=TDT[dst])
            ops.transpose(xin, out)
            assert np.array_equal(raw(out[:, :R]), raw(exp)), (R, C, xin.stride())
            assert np.array_equal(raw(out[:, R:]), raw(torch.full((C, 5), 7.0, dtype=TDT[dst]))), (R, C)


@gpu
@pytest.mark.parametrize("src,dst", PAIRS)
def test_convert2d_all_dtype_pairs_bit_exact(ops, src, dst):
    """mnn_convert2d, all 12 instantiations: 700 x 760 = 532 000 elements (the grid is capped at 2048 x 256 = 524 288 threads, so the last
    7 712 are a second pass), and both operands as column slices at odd offsets and different pitches (bytes outside the slice untouched)."""
    R, C = 700, 760
    x = source_matrix(R, C, src, seed=5)
    out = torch.full((R, C), 7.0, device=DEV, dtype=TDT[dst])
    ops.convert2d(dev(x), out)
    assert np.array_equal(raw(out), raw(x.to(TDT[dst])))
    R, C = 37, 53
    x = source_matrix(R, C, src, seed=6)
    wide = torch.zeros((R, C + 8), dtype=TDT[src])
    wide[:, 3:3 + C] = x
    big = torch.full((R, C + 11), 7.0, device=DEV, dtype=TDT[dst])
    ops.convert2d(dev(wide)[:, 3:3 + C], big[:, 5:5 + C])
    exp = torch.full((R, C + 11), 7.0, dtype=TDT[dst])
    exp[:, 5:5 + C] = x.to(TDT[dst])
    assert np.array_equal(raw(big), raw(exp))


# ------------------------------------------------------------------------------------------------
# dropout: [5, 2048, 512] is 1 310 720 quads; the grid is capped at 4096 x 256 = 1 048 576 threads, which is timesteps 0 .. 3 exactly, so
# timestep 4 lies wholly in the second grid pass
# ------------------------------------------------------------------------------------------------
DT, DB, DU, KP, SEED, ROW0, LAYER = 5, 2048, 512, 0.9, 23, 100, 1
CHECK_T = (0, 3, 4)


@gpu
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_dropout_fwd_all_dtypes_past_the_grid_cap(ops, dt):
    h = torch.from_numpy(np.random.default_rng(11).standard_normal((DT, DB, DU)).astype(np.float32)).to(TDT[dt])
    hd = dev(h)
    y = torch.full((DT, DB, DU), 7.0, device=DEV, dtype=TDT[dt])
    ops.dropout_fwd(hd, y, KP, SEED, ROW0, LAYER)
    for t in CHECK_T:
        exp = cpu_cvt(dropout_expect(h[t].float().numpy(), KP, dropout_keep(KP, SEED, ROW0, LAYER, t, DB, DU)), TDT[dt])
        assert np.array_equal(raw(y[t]), raw(exp)), t
    y1 = torch.full((DT, DB, DU), 7.0, device=DEV, dtype=TDT[dt])
    ops.dropout_fwd(hd, y1, 1.0, SEED, ROW0, LAYER)                 # keep_prob = 1: the copy path (y is not h)
    assert np.array_equal(raw(y1), raw(h))


@gpu
def test_dropout_bwd_past_the_grid_cap(ops):
    dy = np.random.default_rng(12).standard_normal((DT, DB, DU)).astype(np.float32)
    dyd = dev(dy)
    keep = {t: dropout_keep(KP, SEED, ROW0, LAYER, t, DB, DU) for t in CHECK_T}
    dh = torch.full((DT, DB, DU), 7.0, device=DEV)
    ops.dropout_bwd(dyd, dh, KP, SEED, ROW0, LAYER, accumulate=False)          # the old contents vanish
    for t in CHECK_T:
        assert np.array_equal(raw(dh[t]), raw(torch.from_numpy(dropout_expect(dy[t], KP, keep[t])))), t
    dh.fill_(3.0)
    ops.dropout_bwd(dyd, dh, KP, SEED, ROW0, LAYER, accumulate=True)
    for t in CHECK_T:
        assert np.array_equal(dh[t].cpu().numpy(), np.float32(3.0) + dropout_expect(dy[t], KP, keep[t])), t
    dh.fill_(7.0)
    ops.dropout_bwd(dyd, dh, KP, SEED - 3, ROW0, LAYER, step_dev=torch.tensor([3], device=DEV, dtype=torch.int32))   # seed + *step_dev
    for t in CHECK_T:
        assert np.array_equal(raw(dh[t]), raw(torch.from_numpy(dropout_expect(dy[t], KP, keep[t])))), t
    dh.fill_(7.0)
    ops.dropout_bwd(dyd, dh, 1.0, SEED, ROW0, LAYER)                            # keep_prob = 1: no Philox
    assert np.array_equal(raw(dh), raw(torch.from_numpy(dy)))
    dh.fill_(2.0)
    ops.dropout_bwd(dyd, dh, 1.0, SEED, ROW0, LAYER, accumulate=True)
    assert np.array_equal(dh.cpu().numpy(), np.float32(2.0) + dy)
    dh.fill_(7.0)
    ops.dropout_bwd(dyd, dh, KP, SEED, ROW0, LAYER, t_offset=2)                 # local step t draws the counters of step t + 2
    for t in range(DT):                                                         # (counters 3 and 4 are shared with the checks above; local step 4 is the second pass)
        k = dropout_keep(KP, SEED, ROW0, LAYER, t + 2, DB, DU)
        assert np.array_equal(raw(dh[t]), raw(torch.from_numpy(dropout_expect(dy[t], KP, k)))), t


@gpu
def test_dropout_mask_16_per_thread_second_grid_pass(ops):
    """[33, 2048, 512] = 34 603 008 flags: 8192 x 256 threads x 16 cover timesteps 0 .. 31 exactly, timestep 32 is the second pass."""
    T = 33
    mask = torch.full((T, DB, DU), 9, device=DEV, dtype=torch.uint8)
    assert mask.data_ptr() % 16 == 0
    ops.dropout_mask(mask, KP, SEED, ROW0, LAYER)
    for t in (0, 31, 32):
        assert np.array_equal(mask[t].cpu().numpy(), dropout_keep(KP, SEED, ROW0, LAYER, t, DB, DU).astype(np.uint8)), t


@gpu
def test_dropout_mask_4_per_thread_fallbacks_equal_the_16_form(ops):
    T, B = 3, 37
    ref = torch.full((T, B, 32), 9, device=DEV, dtype=torch.uint8)
    assert ref.data_ptr() % 16 == 0
    ops.dropout_mask(ref, KP, SEED, ROW0, LAYER)                                 # aligned, u % 16 == 0: the 16-per-thread form
    exp = np.stack([dropout_keep(KP, SEED, ROW0, LAYER, t, B, 32) for t in range(T)]).astype(np.uint8)
    assert np.array_equal(ref.cpu().numpy(), exp)
    m20 = torch.full((T, B, 20), 9, device=DEV, dtype=torch.uint8)
    ops.dropout_mask(m20, KP, SEED, ROW0, LAYER)                                 # u % 16 != 0
    assert torch.equal(m20, ref[:, :, :20])
    n = T * B * 32
    store = torch.full((n + 8,), 9, device=DEV, dtype=torch.uint8)
    mis = store[4:4 + n].view(T, B, 32)
    assert mis.data_ptr() % 16 == 4
    ops.dropout_mask(mis, KP, SEED, ROW0, LAYER)                                 # u % 16 == 0 on storage 4 bytes into an allocation
    assert torch.equal(mis, ref)
    assert store[:4].tolist() == [9] * 4 and store[4 + n:].tolist() == [9] * 4


# ------------------------------------------------------------------------------------------------
# reductions
# ------------------------------------------------------------------------------------------------
RED_SIZES = [1, 3, 4, 5, 1023, 262147, 300001]


def _probe_positions(n, n4, threads):
    pos = {0, n - 1}
    if n4 > 0:
        pos.add(4 * n4 - 1)                      # last element of the vector body
        if n4 > threads:
            pos.add(4 * threads)                 # first float4 of the body's second grid pass
    if 4 * n4 < n:
        pos.add(4 * n4)                          # first element of the scalar tail
        if n - 4 * n4 > threads:
            pos.add(4 * n4 + threads)            # first element of the tail's second grid pass
    return sorted(pos)


@gpu
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("n", RED_SIZES)
def test_sumsq_exact_sums_and_probes(ops, n, mis):
    R = np.random.default_rng(n)
    x = R.integers(1, 4, n).astype(np.float32)                      # squares <= 9, n <= 300 001: every partial sum < 2^24
    buf = torch.zeros(n + 1, device=DEV)
    xd = buf[mis:mis + n]
    assert (xd.data_ptr() % 16 == 0) == (mis == 0)
    xd.copy_(dev(x))
    out = torch.full((1,), 5.0, device=DEV)                         # accumulates into a non-zero word
    ops.sumsq(xd, out)
    assert float(out) == 5.0 + float((x.astype(np.int64) ** 2).sum())
    grid, n4 = sumsq_geometry(n, mis == 0)
    xd.zero_()
    for p in _probe_positions(n, n4, grid * 256):
        xd[p] = 1.0
        out.zero_()
        ops.sumsq(xd, out)
        assert float(out) == 1.0, p
        xd[p] = 0.0
    # random data against float64, within the derived worst case
    g = (R.standard_normal(n) * 3).astype(np.float32)
    xd.copy_(dev(g))
    out.zero_()
    ops.sumsq(xd, out)
    terms = g.astype(np.float64) ** 2
    assert abs(float(out) - terms.sum()) <= sum_bound(chain_len(n, grid * 256, n4), grid, terms.sum())


@gpu
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("n", RED_SIZES)
def test_weighted_sum_exact_sums_and_probes(ops, n, mis):
    R = np.random.default_rng(n + 1)
    x = R.integers(1, 4, n).astype(np.float32)
    w = R.integers(1, 4, n).astype(np.float32)
    buf, wbuf = torch.zeros(n + 1, device=DEV), torch.zeros(n + 1, device=DEV)
    xd, wd = buf[mis:mis + n], wbuf[mis:mis + n]
    xd.copy_(dev(x)); wd.copy_(dev(w))
    out = torch.full((1,), 5.0, device=DEV)
    ops.weighted_sum(xd, None, out)
    assert float(out) == 5.0 + float(x.astype(np.int64).sum())
    out.fill_(5.0)
    ops.weighted_sum(xd, wd, out)
    assert float(out) == 5.0 + float((x.astype(np.int64) * w.astype(np.int64)).sum())
    grid = min(1024, (n + 255) // 256)
    xd.zero_()
    for p in _probe_positions(n, 0, grid * 256):
        xd[p] = 1.0
        for ww in (None, wd):
            out.zero_()
            ops.weighted_sum(xd, ww, out)
            assert float(out) == (1.0 if ww is None else float(w[p])), p
        xd[p] = 0.0
    g = (R.standard_normal(n) * 3).astype(np.float32)
    wr = R.random(n).astype(np.float32)
    xd.copy_(dev(g)); wd.copy_(dev(wr))
    out.zero_()
    ops.weighted_sum(xd, wd, out)
    terms = g.astype(np.float64) * wr
    assert abs(float(out) - terms.sum()) <= sum_bound(chain_len(n, grid * 256), grid, np.abs(terms).sum())


# ------------------------------------------------------------------------------------------------
# optimiser
# ------------------------------------------------------------------------------------------------
def _adam_case(n, seed):
    R = np.random.default_rng(seed)
    return ((R.standard_normal(n)).astype(np.float32), (R.standard_normal(n) * 3).astype(np.float32),
            (R.standard_normal(n) * 0.1).astype(np.float32), (R.random(n) * 0.5 + 0.01).astype(np.float32))


def _sliced(a, mis):
    buf = torch.zeros(a.size + 4, device=DEV)
    t = buf[mis:mis + a.size]
    t.copy_(dev(a))
    return t


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


ADAM_CASES = [(n, mis) for n in (3, 4, 7, 524291, 2097155, 2097159) for mis in ((0, 0, 0, 0), (1, 1, 1, 1))] + [(7, (0, 1, 0, 0)), (2097155, (0, 1, 0, 0))]


@gpu
@pytest.mark.parametrize("n,mis", ADAM_CASES, ids=["%d-%s" % (n, "".join(map(str, mis))) for n, mis in ADAM_CASES])
def test_clip_adam_step_sizes_and_alignment(ops, n, mis):
    """One Adam step from non-zero moments against the float64 TF semantics.  The launch is min(2048, ceil(n / 256)) x 256 = 524 288 threads
    at most.  Aligned: n / 4 float4 in the vector body, a scalar tail behind; 2 097 155 = 4 x 524 288 + 3 fills the body exactly once (every
    thread one float4, no wrap) and leaves a 3-element tail; 2 097 159 = 4 x 524 289 + 3 puts one float4 in the body's second grid pass (the
    issue's size is one float4 short of the wrap it names).  Misaligned buffers take the scalar path, which wraps from 524 291 on, as does
    sgd=True.  mis = which of (theta, grad, m, v) is a [1:] slice; 0100: only the gradient is misaligned."""
    th, g, m, v = _adam_case(n, n)
    thd, gd, md, vd = (_sliced(a, k) for a, k in zip((th, g, m, v), mis))
    assert [t.data_ptr() % 16 for t in (thd, gd, md, vd)] == [4 * k for k in mis]
    clipped, gn = S.clip_by_global_norm([g.astype(np.float64)], 5.0)
    ssq = torch.tensor([gn * gn], device=DEV, dtype=torch.float32)
    ref_th, ref_m, ref_v = S.adam_tf_step(th.astype(np.float64), clipped[0], m.astype(np.float64), v.astype(np.float64), 2, 0.01)
    ops.clip_adam_step(thd, gd, md, vd, ssq, 5.0, 0.01, 0.9, 0.999, 1e-4, 2)
    assert rel(thd.cpu().numpy(), ref_th) < 1e-5 and rel(md.cpu().numpy(), ref_m) < 1e-5 and rel(vd.cpu().numpy(), ref_v) < 5e-5
    assert np.array_equal(gd.cpu().numpy(), g)
    if n >= 524291 and mis != (0, 1, 0, 0):
        th2 = _sliced(th, mis[0])
        ops.clip_adam_step(th2, gd, None, None, None, 0.0, 0.1, 0.9, 0.999, 1e-4, 1, sgd=True)
        assert rel(th2.cpu().numpy(), th.astype(np.float64) - 0.1 * g.astype(np.float64)) < 1e-6


@gpu
def test_clip_adam_clip_branches(ops):
    """The effective gradient scale through a plain-SGD step with lr = 1 on integer data: theta - g is exact, so scale == 1 shows as equality."""
    n = 1027
    R = np.random.default_rng(3)
    th = R.integers(-50, 50, n).astype(np.float32)
    g = R.integers(-9, 10, n).astype(np.float32)

    def run(ssq, clip):
        t = dev(th)
        buf = None if ssq is None else torch.tensor([ssq], device=DEV, dtype=torch.float32)
        ops.clip_adam_step(t, dev(g), None, None, buf, clip, 1.0, 0.9, 0.999, 1e-4, 1, sgd=True)
        return t.cpu().numpy()
    assert np.array_equal(run(4.0 * 4.0, 5.0), th - g)                  # norm 4 below the clip 5: scale exactly 1
    assert np.array_equal(run(5.0 * 5.0, 5.0), th - g)                  # norm equal to the clip
    assert np.array_equal(run(0.0, 5.0), th - g)                        # norm exactly 0
    assert np.array_equal(run(1e6, 0.0), th - g)                        # clip_norm = 0 with a sumsq buffer given: no clipping
    assert np.array_equal(run(None, 5.0), th - g)                       # no buffer
    got = run(400.0, 5.0)                                               # norm 20 above the clip: scale 5 / 20
    assert rel(got, th.astype(np.float64) - 0.25 * g) < 1e-6 and not np.array_equal(got, th - g)


@gpu
def test_clip_adam_device_step_counter_past_the_grid_cap(ops):
    n = 524291
    th, g, _, _ = _adam_case(n, 9)
    out = torch.zeros(1, device=DEV)
    ops.sumsq(dev(g), out)
    gd = dev(g)
    tht, m, v = dev(th), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    th_d, m_d, v_d = dev(th), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sd = torch.zeros(1, device=DEV, dtype=torch.int32)
    ref_th, ref_m, ref_v = th.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        clipped, gn = S.clip_by_global_norm([g.astype(np.float64)], 5.0)
        ref_th, ref_m, ref_v = S.adam_tf_step(ref_th, clipped[0], ref_m, ref_v, step, 0.01)
        ops.clip_adam_step(tht, gd, m, v, out, 5.0, 0.01, 0.9, 0.999, 1e-4, step)
        ops.clip_adam_step(th_d, gd, m_d, v_d, out, 5.0, 0.01, 0.9, 0.999, 1e-4, 0, step_dev=sd)
        ops.step_increment(sd)
    assert int(sd) == 3
    assert rel(th_d.cpu().numpy(), tht.cpu().numpy()) < 1e-6 and torch.equal(m_d, m) and torch.equal(v_d, v)
    assert rel(tht.cpu().numpy(), ref_th) < 1e-5 and rel(m.cpu().numpy(), ref_m) < 1e-5 and rel(v.cpu().numpy(), ref_v) < 5e-5


# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 64), (1000, 70), (16448, 65)])
def test_bias_grad_exact_column_sums(ops, rows, cols):
    """Integer-valued rows (column sums < 2^24: exact in any order); 16 448 rows make cdiv(rows, 64) = 257, one above the cap on grid.y."""
    R = np.random.default_rng(rows + cols)
    full = R.integers(1, 4, (rows, cols + 6)).astype(np.float32)
    ref = full[:, 3:3 + cols].astype(np.int64).sum(0)
    fd = dev(full)
    db = torch.full((cols,), 7.0, device=DEV)
    ops.bias_grad(fd[:, 3:3 + cols], db, accumulate=False)                   # column slice, ld > cols, odd start; overwrites
    assert np.array_equal(db.cpu().numpy().astype(np.int64), ref)
    ops.bias_grad(fd[:, 3:3 + cols], db, accumulate=True)
    assert np.array_equal(db.cpu().numpy().astype(np.int64), 2 * ref)
    db.fill_(7.0)
    ops.bias_grad(dev(np.ascontiguousarray(full[:, 3:3 + cols])), db, accumulate=True)
    assert np.array_equal(db.cpu().numpy().astype(np.int64), 7 + ref)


@gpu
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", [(48, 40, 33, 40), (200, 704, 696, 704), (64, 64, 64, 64), (130, 24, 17, 28), (16448, 72, 65, 72)])
def test_grad_rows_fanout_both_16_bit_types(ops, shape, dt):
    """Copy and transpose bit-exact against the CPU conversion (random data), column sums exact (integer data); the padding columns
    [cols_t, cols_c) of dY hold NaN: zeros in out_c, nothing in db.  16 448 rows wrap the 256 row slabs; cols_t = 65 ends in a scalar float4."""
    rows, cols_c, cols_t, ld = shape
    R = np.random.default_rng(6)
    Np = ops.round_up(rows, 64)
    for kind in ("random", "integer"):
        a = R.standard_normal((rows, ld)).astype(np.float32) if kind == "random" else R.integers(-3, 4, (rows, ld)).astype(np.float32)
        a[:, cols_t:cols_c] = np.nan
        dY = dev(a)[:, :cols_c]
        out_c = torch.full((rows, cols_c), 7.0, device=DEV, dtype=TDT[dt])
        out_t = torch.full((cols_t, Np), 7.0, device=DEV, dtype=TDT[dt])
        db = torch.full((cols_t,), 5.0, device=DEV)
        ops.grad_rows_fanout(dY, cols_t, out_c, out_t, db)
        ref = cpu_cvt(a[:, :cols_c], TDT[dt])
        ref[:, cols_t:] = 0
        assert np.array_equal(raw(out_c), raw(ref))
        assert np.array_equal(raw(out_t[:, :rows]), raw(ref[:, :cols_t].t()))
        assert np.array_equal(raw(out_t[:, rows:]), raw(torch.full((cols_t, Np - rows), 7.0, dtype=TDT[dt])))
        got = db.cpu().numpy()
        assert np.isfinite(got).all()
        if kind == "integer":
            assert np.array_equal(got.astype(np.int64), 5 + a[:, :cols_t].astype(np.int64).sum(0))


# ------------------------------------------------------------------------------------------------
# LSTM weight packs and gradient unpacks
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n_in,u,ld_in", [(12, 32, 16), (440, 512, 448), (17, 96, 24), (8, 128, 8)])
def test_lstm_pack_weights_bit_exact(ops, n_in, u, ld_in, dt):
    R = np.random.default_rng(n_in + u)
    W = (R.standard_normal((n_in + u, 4 * u)) * 0.2).astype(np.float32)
    W.reshape(-1)[:len(SPECIALS)] = SPECIALS
    b = (R.standard_normal(4 * u) * 0.1).astype(np.float32)
    exp = pack_np(W, b, n_in, u, ld_in)
    mk = lambda *s: torch.full(s, 7.0, device=DEV, dtype=TDT[dt])
    for with_wx_p in (True, False):
        wx_t, wh_t, wh_p, wx_p = mk(4 * u, ld_in), mk(4 * u, u), mk(u, 4 * u), (mk(n_in, 4 * u) if with_wx_p else None)
        bias_p = torch.full((4 * u,), 7.0, device=DEV)
        ops.lstm_pack_weights(dev(W), dev(b), n_in, u, wx_t, wh_t, wh_p, wx_p, bias_p)
        for got, e in zip((wx_t, wh_t, wh_p), exp[:3]):
            assert np.array_equal(raw(got), raw(cpu_cvt(e, TDT[dt])))
        assert np.array_equal(raw(wx_t[:, n_in:]), np.zeros((4 * u, ld_in - n_in), raw(wx_t).dtype))      # K padding: +0 over the pre-filled buffer
        if with_wx_p:
            assert np.array_equal(raw(wx_p), raw(cpu_cvt(exp[3], TDT[dt])))
        assert np.array_equal(raw(bias_p), raw(torch.from_numpy(exp[4])))


@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_lstm_rows_gate_minor_moves_raw_words(ops, dt):
    u, ld = 96, 24
    R = np.random.default_rng(2)
    words = R.integers(-2 ** 15, 2 ** 15, (4 * u, ld)).astype(np.int16) if dt != "f32" else R.integers(-2 ** 31, 2 ** 31, (4 * u, ld)).astype(np.int32)
    src = dev(words).view(TDT[dt])
    bias_p = R.standard_normal(4 * u).astype(np.float32)
    dst = torch.zeros((4 * u, ld), device=DEV, dtype=TDT[dt])
    bias_gm = torch.zeros(4 * u, device=DEV)
    ops.lstm_rows_gate_minor(src, dev(bias_p), dst, bias_gm)
    unit, g = np.divmod(np.arange(4 * u), 4)                         # destination row = unit * 4 + g
    pc = (unit // 32) * 128 + g * 32 + unit % 32
    assert np.array_equal(pc, gate_perm(u)[g * u + unit])
    assert np.array_equal(raw(dst), words[pc]) and np.array_equal(bias_gm.cpu().numpy(), bias_p[pc])


@gpu
@pytest.mark.parametrize("n_in,u,ld_in", [(17, 96, 24), (12, 32, 16), (8, 128, 8)])
def test_lstm_unpack_grads_three_forms_exact(ops, n_in, u, ld_in):
    """Integer-valued packed gradients added into non-zero integer dW / db: plain, consuming and concatenated-source forms give the same
    numbers; the consuming forms zero exactly what they read (the K padding [n_in, ld_in) is not read and keeps its contents)."""
    R = np.random.default_rng(u)
    iv = lambda *s: R.integers(-9, 10, s).astype(np.float32)
    dwx_t, dwh_t, db_p, dW0, db0 = iv(4 * u, ld_in), iv(4 * u, u), iv(4 * u), iv(n_in + u, 4 * u), iv(4 * u)
    eW, eb = unpack_np(dwx_t, dwh_t, db_p, n_in, u)
    eW, eb = dW0 + eW, db0 + eb
    a, b_, c = dev(dwx_t), dev(dwh_t), dev(db_p)
    dW, db = dev(dW0), dev(db0)
    ops.lstm_unpack_grads(a, b_, c, n_in, u, dW, db)
    assert np.array_equal(dW.cpu().numpy(), eW) and np.array_equal(db.cpu().numpy(), eb)
    assert np.array_equal(a.cpu().numpy(), dwx_t) and np.array_equal(b_.cpu().numpy(), dwh_t) and np.array_equal(c.cpu().numpy(), db_p)
    dW, db = dev(dW0), dev(db0)
    ops.lstm_unpack_grads(a, b_, c, n_in, u, dW, db, consume=True)
    assert np.array_equal(dW.cpu().numpy(), eW) and np.array_equal(db.cpu().numpy(), eb)
    assert not bool(a[:, :n_in].any()) and not bool(b_.any()) and not bool(c.any())
    assert np.array_equal(a[:, n_in:].cpu().numpy(), dwx_t[:, n_in:])
    cat = dev(np.concatenate([dwx_t, dwh_t], 1))
    c = dev(db_p)
    dW, db = dev(dW0), dev(db0)
    ops.lstm_unpack_grads_cat(cat, c, n_in, u, ld_in, dW, db)
    assert np.array_equal(dW.cpu().numpy(), eW) and np.array_equal(db.cpu().numpy(), eb)
    assert not bool(cat[:, :n_in].any()) and not bool(cat[:, ld_in:].any()) and not bool(c.any())
    assert np.array_equal(cat[:, n_in:ld_in].cpu().numpy(), dwx_t[:, n_in:])


# ------------------------------------------------------------------------------------------------
# RBM gradient-row group
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D,Hn", [(88, 168), (13, 65)])
@pytest.mark.parametrize("N", [1, 255, 256, 4095, 4096])
def test_rbm_cd_bias_delta_exact(ops, N, D, Hn):
    """{0,1} states, probabilities on the quarter grid, scale 1/2: every partial sum is a multiple of 1/8 below 2^13, exact in f32 in any
    order.  N = 255 | 256 and 4095 | 4096 straddle the 1 / 8 / 64 row-slab switch."""
    R = np.random.default_rng(N + D)
    v, h = R.integers(0, 2, (N, D)).astype(np.uint8), R.integers(0, 2, (N, Hn)).astype(np.uint8)
    p_v, p_h = (R.integers(0, 5, (N, D)) / 4).astype(np.float32), (R.integers(0, 5, (N, Hn)) / 4).astype(np.float32)
    pre_v, pre_h = R.integers(-5, 6, D).astype(np.float32), R.integers(-5, 6, Hn).astype(np.float32)
    dbv, dbh = dev(pre_v), dev(pre_h)
    ops.rbm_cd_bias_delta(dev(v), dev(p_v), dev(h), dev(p_h), 0.5, dbv, dbh)
    assert np.array_equal(dbv.cpu().numpy().astype(np.float64), pre_v + 0.5 * (v.astype(np.float64) - p_v).sum(0))
    assert np.array_equal(dbh.cpu().numpy().astype(np.float64), pre_h + 0.5 * (h.astype(np.float64) - p_h).sum(0))


@gpu
@pytest.mark.parametrize("N,D,Hn,ld", [(5, 88, 168, 264), (3, 13, 65, 300)])
def test_rbm_cd_rows_vs_float64(ops, N, D, Hn, ld):
    """ld > 256 wraps the column loop.  The scale is a power of two, so w = rw * scale is exact and every output is one f32 subtraction
    and one multiplication away from the float64 value: 2 x 2^-24 relative."""
    R = np.random.default_rng(N)
    v, vs = R.integers(0, 2, (N, D)).astype(np.uint8), R.integers(0, 2, (N, D)).astype(np.uint8)
    sv, ss = R.random((N, Hn)).astype(np.float32), R.random((N, Hn)).astype(np.float32)
    rw = R.random(N).astype(np.float32)
    rw[1] = 0.0                                                       # a masked row
    d_out = torch.full((N, ld), 7.0, device=DEV)
    pos, neg = torch.full((N, Hn), 7.0, device=DEV), torch.full((N, Hn), 7.0, device=DEV)
    ops.rbm_cd_rows(dev(v), dev(vs), dev(sv), dev(ss), dev(rw), 0.5, d_out, pos, neg)
    w = (rw.astype(np.float64) * 0.5)[:, None]
    got = d_out.cpu().numpy().astype(np.float64)
    close = lambda a, r: bool((np.abs(a - r) <= 2.0 ** -23 * np.abs(r)).all())
    assert close(got[:, :Hn], w * (ss.astype(np.float64) - sv)) and close(got[:, Hn:Hn + D], w * (vs.astype(np.float64) - v))
    assert close(pos.cpu().numpy().astype(np.float64), w * ss) and close(neg.cpu().numpy().astype(np.float64), -w * sv)
    assert not bool(d_out[:, Hn + D:].any()) and not bool(d_out[1].any()) and not bool(pos[1].any()) and not bool(neg[1].any())


@gpu
@pytest.mark.parametrize("n", [1, 524291])
def test_sigmoid_grad_vs_float64(ops, n):
    """dz = dy (y (1 - y)): a subtraction and two multiplications, each rounded once, so within 3 x 2^-24 of float64 (the form y - y y, built
    without contraction, missed this by up to y / (1 - y) roundings: 25 x 2^-24 on these inputs).  524 291 = 2048 x 256 + 3 wraps the grid."""
    R = np.random.default_rng(n)
    dy, y = R.standard_normal(n).astype(np.float32), R.uniform(0.02, 0.98, n).astype(np.float32)
    ref = dy.astype(np.float64) * y * (1.0 - y.astype(np.float64))
    dz = torch.full((n,), 7.0, device=DEV)
    ops.sigmoid_grad(dev(dy), dev(y), dz)
    assert (np.abs(dz.cpu().numpy() - ref) <= 3 * U * np.abs(ref)).all()
    dyd = dev(dy)
    ops.sigmoid_grad(dyd, dev(y), dyd)                                # dz aliasing dy
    assert torch.equal(dyd, dz)


@gpu
@pytest.mark.parametrize("n", [1, 262147])
def test_axpby_exact_aliased_and_misaligned(ops, n):
    """Integer data and coefficients (exact); 262 147 = 1024 x 256 + 3 wraps the grid; operands are buf[1:] / buf[3:] slices whose
    neighbours must keep their contents."""
    R = np.random.default_rng(n)
    x, y = R.integers(-99, 100, n).astype(np.float32), R.integers(-99, 100, n).astype(np.float32)

    def sl(a, off):
        buf = torch.full((n + 8,), 7.0, device=DEV)
        buf[off:off + n] = dev(a)
        return buf, buf[off:off + n]

    def untouched(buf, off):
        return buf[:off].tolist() == [7.0] * off and buf[off + n:].tolist() == [7.0] * (8 - off)
    bx, xd = sl(x, 1); by, yd = sl(y, 3); bo, od = sl(np.zeros(n, np.float32), 5)
    ops.axpby(3.0, xd, -2.0, yd, od)
    assert np.array_equal(od.cpu().numpy(), 3 * x - 2 * y) and untouched(bo, 5) and untouched(bx, 1) and untouched(by, 3)
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(yd.cpu().numpy(), y)
    ops.axpby(3.0, xd, -2.0, yd, xd)                                  # out aliasing x
    assert np.array_equal(xd.cpu().numpy(), 3 * x - 2 * y) and untouched(bx, 1)
    bx, xd = sl(x, 1)
    ops.axpby(3.0, xd, -2.0, yd, yd)                                  # out aliasing y
    assert np.array_equal(yd.cpu().numpy(), 3 * x - 2 * y) and untouched(by, 3)
    ops.axpby(4.0, xd, 0.0, None, od)                                 # y = None with b = 0
    assert np.array_equal(od.cpu().numpy(), 4 * x) and untouched(bo, 5)
    with pytest.raises(ValueError):
        ops.axpby(1.0, xd, 1.0, None, od)


@gpu
@pytest.mark.parametrize("D", [1, 88, 300])
def test_rbm_visible_bias_init_within_2_ulp(ops, D):
    count = np.float32(1000.0)
    R = np.random.default_rng(D)
    colsum = R.integers(0, 1000, D).astype(np.float32)
    colsum[:4] = [0.0, 1.0, 500.0, 999.0][:min(4, D)]                 # p = 0 (-> log 1e-6), small, 1/2, near 1
    bv = torch.full((D,), 7.0, device=DEV)
    ops.rbm_visible_bias_init(dev(colsum), float(count), bv)
    p = colsum / count
    ref = np.log(np.float32(1e-6) + p / (np.float32(1.0) - p)).astype(np.float32)
    got = bv.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - ref) <= 2 * np.spacing(np.abs(ref))).all()
    assert abs(float(got[0]) - float(np.log(np.float32(1e-6)))) <= 2 * np.spacing(np.float32(13.8))


@gpu
@pytest.mark.parametrize("n", [1, 524291])
def test_fill_on_a_slice(ops, n):
    buf = torch.full((n + 9,), 7.0, device=DEV)
    ops.fill(buf[5:5 + n], -1.25)
    assert buf[:5].tolist() == [7.0] * 5 and buf[5 + n:].tolist() == [7.0] * 4
    assert bool((buf[5:5 + n] == -1.25).all())


# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("n", [15, 16, 17, 4194320])
def test_density_gate_counts_bytes_not_bits(ops, n, mis):
    """Cells of 0x80, 0x10, 0x02 and 0xFF next to zero bytes in every byte lane of a 16-byte word: each counts once.  4 194 320 bytes put the
    second grid pass at byte 4 194 304 (1024 x 256 threads x 16).  The decision is count > threshold; the count words are left at zero.
    Through the C entry the gated NADE forward calls (its wrapper also launches the two scans, whose operands must be 0 / 1 cells)."""
    vals = np.array([0x80, 0x10, 0x02, 0xFF], np.uint8)
    R = np.random.default_rng(n)
    i = np.arange(n)
    v = np.where(R.random(n) < 0.5, vals[R.integers(0, 4, n)], 0).astype(np.uint8)
    head = min(n, 128)                                                 # every lane sees every value with a zero beside it
    v[:head] = np.where((i[:head] // 16 + i[:head]) % 2 == 0, vals[(i[:head] // 32 + i[:head]) % 4], 0)
    v[n - 1] = 0x80
    if n > 4194304:
        v[4194304:4194320] = np.where(np.arange(16) % 2 == 0, 0, vals[np.arange(16) % 4])
    exact = int(np.count_nonzero(v))
    buf = torch.zeros(n + 1, device=DEV, dtype=torch.uint8)
    vd = buf[mis:mis + n]
    assert (vd.data_ptr() % 16 == 0) == (mis == 0)
    vd.copy_(dev(v))
    gate = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    count = torch.zeros(ops.DENSITY_SLOTS, device=DEV, dtype=torch.int32)
    for thr, expect in ((exact - 1, 1), (exact, 0)):
        ops.call("mnn_density_gate", ops._stream(), ops._ptr(vd), n, thr, ops._ptr(gate), ops._ptr(count))
        assert int(gate) == expect, (thr, exact)
        assert not bool(count.any())


# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ragged", [False, True])
def test_pianoroll_shift_into_f16(ops, ragged):
    R = np.random.default_rng(2)
    B, T, P, M, ld = 5, 7, 6, 3, 24
    x = ((R.random((B, T, P, M)) < .3) * R.integers(1, 128, (B, T, P, M))).astype(np.uint8)
    D = P * M
    inp_ref, tgt_ref = G.joint_inputs(x.astype(np.float32))
    lengths = np.array([7, 3, 5, 1, 7], np.int32) if ragged else None
    inputs = torch.full((T, B, ld), 9.0, device=DEV, dtype=torch.float16)
    targets = torch.zeros((T, B, D), device=DEV, dtype=torch.uint8)
    rw = torch.zeros(T * B, device=DEV)
    ops.pianoroll_shift_timemajor(dev(x.reshape(B, T, D)), None if lengths is None else dev(lengths), inputs, targets, rw,
                                  int(lengths.sum()) if ragged else 0)
    got = inputs.float().cpu().numpy()
    assert np.array_equal(got[:, :, :D], inp_ref.transpose(1, 0, 2)) and float(np.abs(got[:, :, D:]).max()) == 0
    assert np.array_equal(targets.cpu().numpy(), tgt_ref.transpose(1, 0, 2).astype(np.uint8))
    m = S.sequence_mask(lengths, T) if ragged else np.ones((B, T), bool)
    assert np.allclose(rw.cpu().numpy().reshape(T, B), m.T / m.sum())


@gpu
@pytest.mark.parametrize("shape", [(5, 7, 6, 3, 24), (16, 9, 8, 5, 40), (3, 50, 11, 2, 24)])
@pytest.mark.parametrize("ragged", [False, True])
def test_pianoroll_shift_with_transposed_copy_f16(ops, shape, ragged):
    """The tiled form with dtype = f16: the assertions of test_pianoroll_shift_with_transposed_copy (velocities up to 127 are exact in f16)."""
    B, T, P, M, ld = shape
    R = np.random.default_rng(4)
    x = ((R.random((B, T, P, M)) < .3) * R.integers(1, 128, (B, T, P, M))).astype(np.uint8)
    D = P * M
    inp_ref, tgt_ref = G.joint_inputs(x.astype(np.float32))
    lengths = R.integers(1, T + 1, B).astype(np.int32) if ragged else None
    N, Np = T * B, ops.round_up(T * B, 64)
    inputs = torch.full((T, B, ld), 9.0, device=DEV, dtype=torch.float16)
    inputs_t = torch.zeros((ld, Np), device=DEV, dtype=torch.float16)
    targets = torch.zeros((T, B, D), device=DEV, dtype=torch.uint8)
    rw = torch.zeros(N, device=DEV)
    ops.pianoroll_shift_timemajor(dev(x.reshape(B, T, D)), None if lengths is None else dev(lengths), inputs, targets, rw,
                                  int(lengths.sum()) if ragged else 0, inputs_t=inputs_t)
    got = inputs.float().cpu().numpy()
    assert np.array_equal(got[:, :, :D], inp_ref.transpose(1, 0, 2)) and float(np.abs(got[:, :, D:]).max(initial=0)) == 0
    assert np.array_equal(inputs_t.float().cpu().numpy()[:, :N], got.reshape(N, ld).T)
    assert float(inputs_t[:, N:].abs().max()) == 0 if Np > N else True
    assert np.array_equal(targets.cpu().numpy(), tgt_ref.transpose(1, 0, 2).astype(np.uint8))
    m = S.sequence_mask(lengths, T) if ragged else np.ones((B, T), bool)
    assert np.allclose(rw.cpu().numpy().reshape(T, B), m.T / m.sum())
