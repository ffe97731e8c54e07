"""Kernel-level parity: every C-ABI entry against the CPU oracle on the same seeded inputs.

All calls go through the C ABI (multinn_amd.ops -> libmultinn_hip.so).  Tolerances:
  f32 paths  : 1e-4 relative (BASELINE.json north_star) -- most checks are far tighter
  bf16 paths : 2e-2 relative (bf16 has 8 significant bits; reported, not the parity gate)
  sampling   : bit-exact Bernoulli draws against oracle/det_ref.c
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nade as onade, rbm as orbm, lstm as olstm, philox, det, generators as G   # noqa: E402
from oracle import tf_semantics as S   # noqa: E402
import lstm_float64 as L64   # noqa: E402  (tests/lstm_float64.py: the float64 reference of the single-layer persistent recurrences)

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 72, 88), (1, 696, 256), (333, 2048, 440), (64, 40, 8), (300, 130, 448), (129, 257, 1024), (200, 300, 8192)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gemm_tn(ops, M, N, K, dt):
    R = np.random.default_rng(M * 7 + N)
    A = R.standard_normal((M, K)).astype(np.float32)
    B = R.standard_normal((N, K)).astype(np.float32)
    B[min(3, N - 1), :] = 0
    B[min(3, N - 1), K // 2] = 1.0            # asymmetric marker (catches a transposed C write)
    bias = R.standard_normal(N).astype(np.float32)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    At, Bt = dev(A, tdt), dev(B, tdt)
    Ar, Br = At.float().cpu().numpy().astype(np.float64), Bt.float().cpu().numpy().astype(np.float64)
    ref = Ar @ Br.T + bias
    C = torch.full((M, N), 7.0, device=DEV)
    ops.gemm_tn(At, Bt, C, bias=dev(bias))
    assert rel(C.cpu().numpy(), ref) < (2e-6 if dt == "f32" else 1e-5) * max(1, K // 1024)      # products of bf16 inputs are exact in f32
    C2 = torch.ones((M, N), device=DEV)
    ops.gemm_tn(At, Bt, C2, accumulate=True)
    assert rel(C2.cpu().numpy(), Ar @ Br.T + 1.0) < 1e-5
    C3 = torch.full((M, N), 5.0, device=DEV)
    ops.gemm_tn(At, Bt, C3, bias=dev(bias), split_k=3)
    assert rel(C3.cpu().numpy(), ref) < 1e-5
    Cb = torch.empty((M, N), device=DEV, dtype=torch.bfloat16)
    ops.gemm_tn(At, Bt, Cb)
    assert rel(Cb.float().cpu().numpy(), Ar @ Br.T) < 1e-2


@pytest.mark.parametrize("M,N,K,split_k", [(16384, 704, 256, 1), (16400, 2048, 448, 1), (16384, 704, 512, 1), (16384, 256, 704, 1),
                                          (2048, 512, 16384, 16), (704, 256, 16384, 8), (65536, 704, 256, 1)])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_step_shapes(ops, M, N, K, split_k, dt):
    """The GEMM shapes of the train step (Dense forward N = 704 with its ragged last column tile, input projection, dX, weight gradients with
    split-K) at a reduced row count, both 16-bit flavours, f32 and 16-bit C: every element against torch's f32 product of the same operands.
    (Round 3: a tile form without N-edge handling stored past the row end at N = 704 and only showed at the target shape.)"""
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    At = (torch.randn((M, K), device=DEV, generator=g) * 0.5).to(tdt)
    Bt = (torch.randn((N, K), device=DEV, generator=g) * 0.5).to(tdt)
    bias = torch.randn(N, device=DEV, generator=g)
    ref = At.float() @ Bt.float().T
    scale = float(ref.abs().max())
    C = torch.full((M + 1, N), 7.0, device=DEV)                     # a guard row behind the matrix
    if split_k == 1:
        ops.gemm_tn(At, Bt, C[:M], bias=bias)
        assert float((C[:M] - (ref + bias)).abs().max()) < 2e-5 * scale * max(1, K // 1024)
    else:
        C[:M].zero_()
        ops.gemm_tn(At, Bt, C[:M], accumulate=True, split_k=split_k)
        assert float((C[:M] - ref).abs().max()) < 2e-5 * scale * max(1, K // 1024)
    assert bool((C[M] == 7.0).all())
    if split_k == 1:
        Cb = torch.full((M + 1, N), 7.0, device=DEV, dtype=tdt)
        ops.gemm_tn(At, Bt, Cb[:M])
        assert float((Cb[:M].float() - ref).abs().max()) < (2e-3 if dt == "f16" else 1e-2) * scale
        assert bool((Cb[M] == 7.0).all())


@pytest.mark.parametrize("M,N,K,split_k,rows", [(256, 192, 64, 1, 256), (300, 704, 4096, 1, 320), (2048, 960, 16384, 8, 2048), (1024, 768, 16384, 20, 1024)])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_a_kblock(ops, M, N, K, split_k, rows, dt):
    """A stored K-blocked ([K/32, rows, 32]: the layout the backward recurrence writes dz^T in) against the K-contiguous form on the same
    values: bit-identical operands in LDS, so the results agree to the split-K summation order; also against torch's f32 product."""
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    A = (torch.randn((rows, K), device=DEV, generator=g) * 0.5).to(tdt)
    A[min(37, M - 1)] = 0
    A[min(37, M - 1), K // 2 + 3] = 1.0
    Akb = A.view(rows, K // 32, 32).permute(1, 0, 2).contiguous()
    Bt = (torch.randn((N, K), device=DEV, generator=g) * 0.5).to(tdt)
    ref = A[:M].float() @ Bt.float().T
    scale = float(ref.abs().max())
    C = torch.zeros((M + 1, N), device=DEV)
    C[M] = 7.0
    ops.gemm_tn(Akb, Bt, C[:M], accumulate=True, split_k=split_k, a_kblock=True)
    assert float((C[:M] - ref).abs().max()) < 2e-5 * scale * max(1, K // 1024)
    assert bool((C[M] == 7.0).all())
    if split_k == 1:
        C2 = torch.zeros((M, N), device=DEV)
        ops.gemm_tn(A[:M], Bt, C2, accumulate=True)
        assert torch.equal(C[:M], C2) or float((C[:M] - C2).abs().max()) < 1e-6 * scale


# ------------------------------------------------------------------------------------------------
# mnn_gemm_tn_rows: the m_rows / k_rows hints of a compacted ragged batch.  Only the 256 x 256 tile acts on them, and it is dispatched only for
# large problems (launch_gemm: K % 64 == 0, M >= 256, N >= 192, cdiv(M, 256) * cdiv(N, 256) * split_k >= 192, K / 64 / split_k >= 4, or a
# K-blocked A), so the shapes below are the smallest of each kind that reach it.  Reference: the float64 product of the same 16-bit operands
# on the device; bound: this kernel family's own, 2e-5 * max|ref| * max(1, K // 1024) for an f32 C (test_gemm_tn_step_shapes).
def _hint_operands(M, N, K, dt, marker_col):
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    A = (torch.randn((M, K), device=DEV, generator=g) * 0.5).to(tdt)
    B = (torch.randn((N, K), device=DEV, generator=g) * 0.5).to(tdt)
    B[min(3, N - 1)] = 0
    B[min(3, N - 1), marker_col] = 1.0          # asymmetric marker (test_gemm_tn): C[:, 3] = A[:, marker_col] -- a transposed or shifted C write shows
    bias = torch.randn(N, device=DEV, generator=g)
    return A, B, bias


def _word(n):
    return torch.tensor([n], device=DEV, dtype=torch.int32)


def _ceil_to(n, m):
    return -(-n // m) * m


def _zero_behind(X, k):
    X = X.clone()
    X[:, k:] = 0
    return X


def _kblocked(A):
    M, K = A.shape
    return A.view(M, K // 32, 32).permute(1, 0, 2).contiguous()


def _check_m_hint(C, M, N, m, full, brow, K, what):
    """C [M + 1, ldc] was filled with 7.0 and then written by a product hinted with m_rows = m whose A has zero rows from m on.
    full: float64 reference of the un-truncated product (+ bias), brow: what a zero row of A gives (bias or 0)."""
    lo, hi = min(m, M), min(M, _ceil_to(m, 256))
    if hi > 0:
        tol = 2e-5 * max(float(full[:lo].abs().max()) if lo else 0.0, float(brow.abs().max()), 1e-30) * max(1, K // 1024)
        if lo:
            err = float((C[:lo, :N] - full[:lo]).abs().max())
            assert err < tol, (what, m, "rows below the count", err, tol)                              # (a)
        if hi > lo:
            err = float((C[lo:hi, :N] - brow).abs().max())
            assert err < tol, (what, m, "rows of the tile that straddles the count", err, tol)         # (b)
    assert bool((C[M] == 7.0).all()) and bool((C[:, N:] == 7.0).all()), (what, m, "guard row / pad columns written")     # (c)
    assert bool((C[hi:M] == 7.0).all()), (what, m, "row tiles past the count were written: the hinted 256 x 256 kernel did not run")     # (d)


@pytest.mark.parametrize("M,N,K,ldc,has_bias", [(16384, 696, 256, 704, True), (16400, 2048, 448, 2056, True), (49152, 256, 704, 264, False)])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_rows_hint_m_rows(ops, M, N, K, ldc, has_bias, dt):
    """m_rows on the three shapes of the ragged step that dispatch the 256 x 256 tile (Dense forward with its N edge inside the last column
    tile; an M that is no multiple of 256, f32 C so that the weight-resident kernel does not take it; the dy product), counts at every edge
    of a row tile and beyond M.  A has zero rows from the count on, as ops.rows_gather16 leaves it.  Rows below the count and the rest of
    the tile that straddles it (the NADE workgroup there reads them) equal the float64 product; the guard row and the pad columns of ldc
    keep their sentinel.  (d) EVERY ROW TILE PAST THE COUNT STILL HOLDS THE SENTINEL: that is the witness that the hinted kernel ran at all.
    It pins the implementation on purpose -- if the dispatch thresholds of launch_gemm move and another kernel takes one of these shapes,
    it writes all of C, this assertion fails, and the shapes have to be chosen anew so that the hint stays under test."""
    A, B, bias = _hint_operands(M, N, K, dt, K // 2)
    full = A.double() @ B.double().T
    brow = torch.zeros(N, device=DEV, dtype=torch.float64)
    if has_bias:
        full += bias.double()
        brow = bias.double()
    for m in (0, 1, 255, 256, 257, 8191, M - 1, M, M + 1000):
        Am = A.clone()
        Am[m:] = 0
        C = torch.full((M + 1, ldc), 7.0, device=DEV)
        ops.gemm_tn(Am, B, C[:M, :N], bias=bias if has_bias else None, m_rows=_word(m))
        _check_m_hint(C, M, N, m, full, brow, K, (M, N, K, dt))


@pytest.mark.parametrize("M,N,K,split_k,kblock", [(256, 704, 65536, 64, False), (256, 704, 65536, 65, False), (2048, 960, 16384, 8, False),
                                                  (2048, 960, 16384, 8, True)])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_rows_hint_k_rows(ops, M, N, K, split_k, kblock, dt):
    """k_rows with accumulate=True into a random C0 (how the Dense weight gradient uses it): the slice mapping z = id % split_k (64 slices),
    the XCD-contiguous mapping (65 slices), a square-ish problem, and the K-blocked A, which receives the hint too.
    Contract variant, every count: both operands are zero from the count on, so C must equal C0 + the (truncated = full) float64 product;
    count 0 leaves C bit-equal to C0.  The error bound scales with the depth actually summed, min(k, K) // 1024 -- never wider than the
    family's K // 1024.
    Witness variant, one count that is no multiple of 64: the operands hold zeros in [k, ceil64(k)) and finite random values from
    ceil64(k) on.  The result must equal the product over the first ceil64(k) columns, NOT the full product: that proves the K loop
    stopped at the hinted tile.  It pins the implementation on purpose (a kernel that ignores the hint is within the header's contract
    but fails here): if another kernel takes these shapes, choose shapes that dispatch the hinted one again."""
    A, B, _ = _hint_operands(M, N, K, dt, 0)
    g = torch.Generator(device=DEV).manual_seed(7)
    C0 = torch.randn((M, N), device=DEV, generator=g)

    def run(Ak, Bk, k):
        C = torch.full((M + 1, N), 7.0, device=DEV)
        C[:M] = C0
        ops.gemm_tn(_kblocked(Ak) if kblock else Ak, Bk, C[:M], accumulate=True, split_k=split_k, a_kblock=kblock, k_rows=_word(k))
        assert bool((C[M] == 7.0).all())
        return C[:M]

    def ref_to(Ak, Bk, depth):
        return C0.double() + Ak[:, :depth].double() @ Bk[:, :depth].double().T

    for k in (0, 1, 63, 64, 65, 4097, 40000, K - 1, K, K + 5000):
        Ak, Bk = _zero_behind(A, k), _zero_behind(B, k)
        C = run(Ak, Bk, k)
        if k == 0:
            assert torch.equal(C, C0), "k_rows = 0 with accumulate must leave C alone"
            continue
        ref = ref_to(Ak, Bk, min(k, K))
        err, tol = float((C - ref).abs().max()), 2e-5 * float(ref.abs().max()) * max(1, min(k, K) // 1024)
        assert err < tol, (k, err, tol)
    k = 4097
    kc = _ceil_to(k, 64)
    Aw, Bw = A.clone(), B.clone()
    Aw[:, k:kc] = 0
    Bw[:, k:kc] = 0
    C = run(Aw, Bw, k)
    ref, ref_full = ref_to(Aw, Bw, kc), ref_to(Aw, Bw, K)
    tol = 2e-5 * float(ref.abs().max()) * max(1, kc // 1024)
    assert float((ref_full - ref).abs().max()) > 1e3 * tol            # (the operands behind the count do tell the two products apart)
    err = float((C - ref).abs().max())
    assert err < tol, ("the K loop did not stop at the hinted tile: the 256 x 256 kernel did not run, or ignores k_rows", err, tol)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_rows_hint_both(ops, dt):
    """m_rows = 5000 and k_rows = 200 on one product (f32 C, bias, no accumulate): the assertions of the m_rows test, on operands that are
    zero behind both counts."""
    M, N, K, ldc, m, k = 16384, 704, 512, 712, 5000, 200
    A, B, bias = _hint_operands(M, N, K, dt, 100)
    A, B = _zero_behind(A, k), _zero_behind(B, k)
    full = A.double() @ B.double().T + bias.double()
    A[m:] = 0
    C = torch.full((M + 1, ldc), 7.0, device=DEV)
    ops.gemm_tn(A, B, C[:M, :N], bias=bias, m_rows=_word(m), k_rows=_word(k))
    _check_m_hint(C, M, N, m, full, bias.double(), K, (M, N, K, dt))


@pytest.mark.parametrize("split_k", [1, 2])
@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_rows_hint_k_rows_zero_without_accumulate(ops, split_k, has_bias, dt):
    """k_rows = 0 on a product that does NOT accumulate, at a shape where the hinted kernel runs (one slice, and split-K): C is the bias (or
    zero), which is what every kernel that ignores the hint gives for all-zero operands and what include/multinn_hip.h promises.  (The
    hinted kernel used to leave before its epilogue: C unwritten with one slice, zero without the bias under split-K.)  Second launch: the
    same with finite operands behind the count -- still exactly the bias, because the K loop reads nothing; this one pins the
    implementation, like the witnesses above."""
    M, N, K, ldc = 16384, 704, 512, 712
    A, B, bias = _hint_operands(M, N, K, dt, 0)
    want = (bias if has_bias else torch.zeros(N, device=DEV)).expand(M, N)
    for Ak, Bk in ((torch.zeros_like(A), torch.zeros_like(B)), (A, B)):
        C = torch.full((M + 1, ldc), 7.0, device=DEV)
        ops.gemm_tn(Ak, Bk, C[:M, :N], bias=bias if has_bias else None, split_k=split_k, k_rows=_word(0))
        assert torch.equal(C[:M, :N], want)
        assert bool((C[M] == 7.0).all()) and bool((C[:, N:] == 7.0).all())


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_rows_hint_fall_through(ops, dt):
    """Shapes below the dispatch threshold of the 256 x 256 tile: the other kernels ignore the hints, write all of C, and give the un-hinted
    call's result bit for bit ((1536, 696, 256) is the largest ragged window of tests/test_gpu_generators.py before the 65 k-row one)."""
    M, N, K, ldc, m = 1536, 696, 256, 704, 700
    A, B, bias = _hint_operands(M, N, K, dt, K // 2)
    A[m:] = 0
    Ch, Cu = torch.full((M + 1, ldc), 7.0, device=DEV), torch.full((M + 1, ldc), 7.0, device=DEV)
    ops.gemm_tn(A, B, Ch[:M, :N], bias=bias, m_rows=_word(m))
    ops.gemm_tn(A, B, Cu[:M, :N], bias=bias)
    assert torch.equal(Ch, Cu) and bool((Ch[m:M, :N] == bias).all())
    ref = A.double() @ B.double().T + bias.double()
    assert float((Ch[:M, :N] - ref).abs().max()) < 2e-5 * float(ref.abs().max())
    assert bool((Ch[M] == 7.0).all()) and bool((Ch[:, N:] == 7.0).all())
    # k_rows, one slice (split-K sums its slices with atomics in no fixed order: nothing to compare bit for bit there)
    M, N, K, k = 512, 704, 4096, 1000
    A, B, _ = _hint_operands(M, N, K, dt, 0)
    A, B = _zero_behind(A, k), _zero_behind(B, k)
    C0 = torch.randn((M, N), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    Ch, Cu = C0.clone(), C0.clone()
    ops.gemm_tn(A, B, Ch, accumulate=True, k_rows=_word(k))
    ops.gemm_tn(A, B, Cu, accumulate=True)
    assert torch.equal(Ch, Cu)
    ref = C0.double() + A.double() @ B.double().T
    assert float((Ch - ref).abs().max()) < 2e-5 * float(ref.abs().max()) * max(1, k // 1024)


def test_gemm_strided_views_and_errors(ops):
    R = np.random.default_rng(0)
    A = dev(R.standard_normal((50, 96)).astype(np.float32))
    B = dev(R.standard_normal((30, 96)).astype(np.float32))
    C = torch.zeros((50, 64), device=DEV)
    ops.gemm_tn(A[:, :32], B[:, 32:64], C[:, 8:38])
    ref = A[:, :32].cpu().numpy() @ B[:, 32:64].cpu().numpy().T
    assert rel(C[:, 8:38].cpu().numpy(), ref) < 1e-5 and float(C[:, :8].abs().max()) == 0
    with pytest.raises(RuntimeError):
        ops.gemm_tn(A[:, :30], B[:, :30], torch.zeros((50, 30), device=DEV))      # K % 4 != 0


def test_transpose_convert(ops):
    R = np.random.default_rng(1)
    x = R.standard_normal((77, 45)).astype(np.float32)
    out = torch.zeros((45, 80), device=DEV, dtype=torch.bfloat16)
    ops.transpose(dev(x), out)
    assert rel(out[:, :77].float().cpu().numpy(), x.T) < 1e-2 and float(out[:, 77:].abs().max()) == 0
    u8 = (R.random((33, 65)) < .3).astype(np.uint8)
    o2 = torch.zeros((65, 33), device=DEV)
    ops.transpose(dev(u8), o2)
    assert np.array_equal(o2.cpu().numpy(), u8.T.astype(np.float32))
    o3 = torch.zeros((77, 48), device=DEV, dtype=torch.bfloat16)
    ops.convert2d(dev(x), o3[:, :45])
    assert rel(o3[:, :45].float().cpu().numpy(), x) < 1e-2


@pytest.mark.parametrize("ragged", [False, True])
def test_pianoroll_shift(ops, ragged):
    R = np.random.default_rng(2)
    B, T, P, M = 5, 7, 6, 3
    x = (R.random((B, T, P, M)) < .3).astype(np.uint8)
    D = P * M
    inp_ref, tgt_ref = G.joint_inputs(x.astype(np.float32))
    lengths = np.array([7, 3, 5, 1, 7], np.int32) if ragged else None
    ld = 24
    inputs = torch.full((T, B, ld), 9.0, device=DEV)
    targets = torch.zeros((T, B, D), device=DEV, dtype=torch.uint8)
    rw = torch.zeros(T * B, device=DEV)
    ops.pianoroll_shift_timemajor(dev(x.reshape(B, T, D)), None if lengths is None else dev(lengths), inputs, targets, rw,
                                  int(lengths.sum()) if ragged else 0)
    assert np.array_equal(inputs[:, :, :D].cpu().numpy(), inp_ref.transpose(1, 0, 2))
    assert float(inputs[:, :, D:].abs().max()) == 0
    assert np.array_equal(targets.cpu().numpy(), tgt_ref.transpose(1, 0, 2).astype(np.uint8))
    m = S.sequence_mask(lengths, T) if ragged else np.ones((B, T), bool)
    assert np.allclose(rw.cpu().numpy().reshape(T, B), m.T / m.sum())
    out = torch.zeros((M, T, B, P), device=DEV, dtype=torch.uint8)
    ops.pianoroll_split_tracks(dev(x), out)
    assert np.array_equal(out.cpu().numpy(), x.transpose(3, 1, 0, 2))


@pytest.mark.parametrize("shape", [(5, 7, 6, 3, 24), (16, 9, 8, 5, 40), (3, 50, 11, 2, 24)])
@pytest.mark.parametrize("ragged", [False, True])
def test_pianoroll_shift_with_transposed_copy(ops, shape, ragged):
    """The tiled bf16 form (mnn_pianoroll_shift_timemajor_t) against the oracle's joint_inputs: inputs, inputs^T, targets, row weights
    (D a multiple of 8 -> 8-byte loads, and not -> byte loads; row counts that are not multiples of 64; velocities > 1 stay exact)."""
    B, T, P, M, ld = shape
    R = np.random.default_rng(4)
    x = ((R.random((B, T, P, M)) < .3) * R.integers(1, 128, (B, T, P, M))).astype(np.uint8)
    D = P * M
    inp_ref, tgt_ref = G.joint_inputs(x.astype(np.float32))
    lengths = R.integers(1, T + 1, B).astype(np.int32) if ragged else None
    N, Np = T * B, ops.round_up(T * B, 64)
    inputs = torch.full((T, B, ld), 9.0, device=DEV, dtype=torch.bfloat16)
    inputs_t = torch.zeros((ld, Np), device=DEV, dtype=torch.bfloat16)
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


@pytest.mark.parametrize("shape", [(48, 40, 33, 40), (200, 704, 696, 704), (64, 64, 64, 64), (130, 24, 17, 28)])
def test_grad_rows_fanout(ops, shape):
    """mnn_grad_rows_fanout = bf16 copy + bf16 transpose + column sums of an f32 gradient block in one pass."""
    rows, cols_c, cols_t, ld = shape
    R = np.random.default_rng(6)
    full = torch.from_numpy(R.standard_normal((rows, ld)).astype(np.float32)).to(DEV)
    dY = full[:, :cols_c]
    Np = ops.round_up(rows, 64)
    out_c = torch.full((rows, cols_c), 7.0, device=DEV, dtype=torch.bfloat16)
    out_t = torch.zeros((cols_t, Np), device=DEV, dtype=torch.bfloat16)
    db = torch.full((cols_t,), 0.5, device=DEV)
    ops.grad_rows_fanout(dY, cols_t, out_c, out_t, db)
    ref = dY.to(torch.bfloat16)
    ref[:, cols_t:] = 0                        # padding columns [cols_t, cols_c) are written as zeros whatever dY holds there
    assert torch.equal(out_c, ref)
    assert torch.equal(out_t[:, :rows], ref[:, :cols_t].t()) and float(out_t[:, rows:].abs().max()) == 0 if Np > rows else True
    assert torch.allclose(db, 0.5 + dY[:, :cols_t].double().sum(0).float(), atol=1e-4, rtol=1e-5)


# ------------------------------------------------------------------------------------------------
def _lstm_setup(ops, B, T, n_in, u, dt, seed=3):
    R = np.random.default_rng(seed)
    x = (R.random((B, T, n_in)) < .3).astype(np.float32)
    W = (R.standard_normal((n_in + u, 4 * u)) * 0.2).astype(np.float32)
    b = (R.standard_normal(4 * u) * 0.1).astype(np.float32)
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dt]
    ld = ops.round_up(n_in, 8)
    wx_t = torch.empty((4 * u, ld), device=DEV, dtype=tdt)
    wh_t = torch.empty((4 * u, u), device=DEV, dtype=tdt)
    wh_p = torch.empty((u, 4 * u), device=DEV, dtype=tdt)
    wx_p = torch.empty((n_in, 4 * u), device=DEV, dtype=tdt)
    bias_p = torch.empty(4 * u, device=DEV)
    ops.lstm_pack_weights(dev(W), dev(b), n_in, u, wx_t, wh_t, wh_p, wx_p, bias_p)
    xin = torch.zeros((T, B, ld), device=DEV, dtype=tdt)
    xin[:, :, :n_in] = dev(x.transpose(1, 0, 2)).to(tdt)
    return x, W, b, (wx_t, wh_t, wh_p, wx_p, bias_p), xin, tdt


def _unperm(z, u):
    """gate-interleaved [.., 4u] -> natural TF [.., 4u]"""
    idx = np.empty(4 * u, np.int64)
    for g in range(4):
        for j in range(u):
            idx[g * u + j] = (j // 32) * 128 + g * 32 + j % 32
    return z[..., idx]


@pytest.mark.parametrize("dt,B,T,n_in,u", [("f32", 5, 6, 12, 32), ("f32", 70, 4, 20, 64), ("bf16", 33, 5, 16, 64),
                                          ("bf16", 40, 3, 24, 128), ("bf16", 33, 3, 16, 256), ("bf16", 70, 3, 8, 512), ("f32", 9, 2, 8, 128),
                                          ("bf16", 520, 3, 8, 128), ("bf16", 640, 2, 16, 512),
                                          ("f16", 33, 5, 16, 64), ("f16", 40, 3, 24, 128), ("f16", 70, 3, 8, 512)])
def test_lstm_layer_fwd_bwd(ops, dt, B, T, n_in, u):
    x, W, b, (wx_t, wh_t, wh_p, wx_p, bias_p), xin, tdt = _lstm_setup(ops, B, T, n_in, u, dt)
    # f16 (the generic step kernels at every width): the bf16 tolerance scaled by the ratio of the unit roundoffs, 2^-11 against 2^-8
    tol = {"f32": 2e-5, "bf16": 3e-2, "f16": 3e-2 / 8}[dt]
    # packing
    assert rel(_unperm(wx_t.float().cpu().numpy().T[:n_in], u), W[:n_in]) < (1e-7 if dt == "f32" else 1e-2)
    assert rel(_unperm(wh_p.float().cpu().numpy(), u), W[n_in:]) < (1e-7 if dt == "f32" else 1e-2)
    # forward
    xproj = torch.empty((T, B, 4 * u), device=DEV)
    ops.gemm_tn(xin.view(T * B, -1), wx_t, xproj.view(T * B, -1), bias=bias_p)
    gates = torch.empty((T, B, 4 * u), device=DEV)
    c = torch.empty((T, B, u), device=DEV)
    h = torch.empty((T, B, u), device=DEV, dtype=tdt)
    ops.lstm_seq_fwd(xproj, wh_t, None, None, gates, c, h)
    y, st, cache = olstm.seq_fwd(x.astype(np.float64), [(W.astype(np.float64), b.astype(np.float64))])
    assert rel(h.float().cpu().numpy().transpose(1, 0, 2), y) < tol
    assert rel(c.cpu().numpy()[-1], st[0][0]) < tol
    gi = np.stack([np.concatenate(cache['gates'][0][t], axis=1) for t in range(T)])
    assert rel(_unperm(gates.cpu().numpy(), u), gi) < tol
    # backward
    R = np.random.default_rng(9)
    dy = R.standard_normal((B, T, u)).astype(np.float32)
    dz = torch.empty((T, B, 4 * u), device=DEV)
    dzT = dz if dt == "f32" else torch.empty((T, B, 4 * u), device=DEV, dtype=tdt)
    ops.lstm_seq_bwd(dev(dy.transpose(1, 0, 2)), wh_p, gates, c, None, dz, dzT)
    dx_ref, grads = olstm.seq_bwd(dy.astype(np.float64), cache)
    # dW = [x,h_prev]^T dz ; check through the GEMM path the model uses
    dzf = dz.view(T * B, 4 * u)
    dwx_t = torch.zeros((4 * u, wx_t.shape[1]), device=DEV)
    dzT_t = torch.empty((4 * u, ops.round_up(T * B, 8)), device=DEV, dtype=tdt).zero_()
    ops.transpose(dzf, dzT_t)
    xT = torch.zeros((wx_t.shape[1], ops.round_up(T * B, 8)), device=DEV, dtype=tdt)
    ops.transpose(xin.view(T * B, -1), xT)
    ops.gemm_tn(dzT_t, xT, dwx_t, split_k=2)
    hprev = torch.zeros((T, B, u), device=DEV, dtype=tdt)
    hprev[1:] = h[:-1]
    hT = torch.zeros((u, ops.round_up(T * B, 8)), device=DEV, dtype=tdt)
    ops.transpose(hprev.view(T * B, u), hT)
    dwh_t = torch.zeros((4 * u, u), device=DEV)
    ops.gemm_tn(dzT_t, hT, dwh_t)
    db_p = torch.zeros(4 * u, device=DEV)
    ops.bias_grad(dzf, db_p)
    dW = torch.zeros((n_in + u, 4 * u), device=DEV)
    db = torch.zeros(4 * u, device=DEV)
    ops.lstm_unpack_grads(dwx_t, dwh_t, db_p, n_in, u, dW, db)
    assert rel(dW.cpu().numpy(), grads[0][0]) < tol * 3
    assert rel(db.cpu().numpy(), grads[0][1]) < tol * 3
    # the consuming form adds the same values and leaves every source it read at zero (persistent split-K accumulators)
    dW2, db2 = torch.zeros_like(dW), torch.zeros_like(db)
    ops.lstm_unpack_grads(dwx_t, dwh_t, db_p, n_in, u, dW2, db2, consume=True)
    assert torch.equal(dW2, dW) and torch.equal(db2, db)
    assert float(dwx_t[:, :n_in].abs().max()) == 0 and float(dwh_t.abs().max()) == 0 and float(db_p.abs().max()) == 0
    dx = torch.empty((T * B, n_in), device=DEV)
    ops.gemm_tn(dzT.view(T * B, -1), wx_p.view(n_in, -1), dx)
    assert rel(dx.view(T, B, n_in).cpu().numpy().transpose(1, 0, 2), dx_ref) < tol * 3


def test_lstm_chunked_calls_equal_full_sequence(ops):
    B, T, n_in, u = 20, 7, 8, 128
    x, W, b, (wx_t, wh_t, wh_p, wx_p, bias_p), xin, tdt = _lstm_setup(ops, B, T, n_in, u, "bf16", seed=8)
    xproj = torch.empty((T, B, 4 * u), device=DEV)
    ops.gemm_tn(xin.view(T * B, -1), wx_t, xproj.view(T * B, -1), bias=bias_p)
    mk = lambda: (torch.zeros((T, B, 4 * u), device=DEV), torch.zeros((T, B, u), device=DEV), torch.zeros((T, B, u), device=DEV, dtype=tdt))
    g1, c1, h1 = mk(); g2, c2, h2 = mk()
    ops.lstm_seq_fwd(xproj, wh_t, None, None, g1, c1, h1)
    for t0, t1 in [(0, 3), (3, 4), (4, 7)]:
        ops.lstm_seq_fwd(xproj, wh_t, None, None, g2, c2, h2, t0, t1)
    assert torch.equal(h1, h2) and torch.equal(c1, c2) and torch.equal(g1, g2)
    dy = dev(np.random.default_rng(1).standard_normal((T, B, u)).astype(np.float32))
    dz1 = torch.zeros((T, B, 4 * u), device=DEV); dzb1 = torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt)
    dz2 = torch.zeros_like(dz1); dzb2 = torch.zeros_like(dzb1)
    ops.lstm_seq_bwd(dy, wh_p, g1, c1, None, dz1, dzb1)
    ws = ops.lstm_seq_bwd_workspace(B, u, DEV)
    for t0, t1 in [(5, 7), (2, 5), (0, 2)]:
        ops.lstm_seq_bwd(dy, wh_p, g1, c1, None, dz2, dzb2, None, None, t0, t1, ws)
    assert torch.equal(dz1, dz2) and torch.equal(dzb1, dzb2)
    with pytest.raises(ValueError):
        ops.lstm_seq_bwd(dy, wh_p, g1, c1, None, dz2, dzb2, None, None, 2, 5)      # chunked call without a shared workspace
    # fused epilogue outputs of the bf16 step kernels: h_prev^T, dz^T and sum(dz)
    assert ops.lstm_fused_outputs(torch.bfloat16, u) and not ops.lstm_fused_outputs(torch.float32, u)
    Np = ops.round_up(T * B, 64)
    hT = torch.zeros((u, Np), device=DEV, dtype=tdt)
    g3, c3, h3 = mk()
    ops.lstm_seq_fwd(xproj, wh_t, None, None, g3, c3, h3, 0, T, hT)
    ref_hT = torch.zeros((u, Np), device=DEV, dtype=tdt)
    ref_hT[:, B:T * B] = h1[:-1].reshape((T - 1) * B, u).t()
    assert torch.equal(hT, ref_hT)
    dzT = torch.zeros((4 * u, Np), device=DEV, dtype=tdt); db = torch.zeros(4 * u, device=DEV)
    dzb3 = torch.zeros_like(dzb1)
    ws = ops.lstm_seq_bwd_workspace(B, u, DEV)
    for t0, t1 in [(4, 7), (0, 4)]:
        ops.lstm_seq_bwd(dy, wh_p, g1, c1, None, None, dzb3, None, None, t0, t1, ws, dzT, db)     # no f32 dz at all
    assert torch.equal(dzb3, dzb1)
    assert torch.equal(dzT[:, :T * B], dzb1.view(T * B, 4 * u).t()) and float(dzT[:, T * B:].abs().max()) == 0
    # the bias gradient is the row sum of the bf16 dz^T (one pass, off the per-step chain)
    assert rel(db.cpu().numpy(), dzb1.float().view(T * B, -1).sum(0).cpu().numpy()) < 1e-5
    assert rel(db.cpu().numpy(), dz1.view(T * B, -1).sum(0).cpu().numpy()) < 1e-2


@pytest.mark.parametrize("dt,u", [("f32", 32), ("f16", 64)])
def test_lstm_generic_path_epilogue_outputs(ops, dt, u):
    """The generic step kernels' epilogue (mnn_transpose / mnn_bias_grad at pointer offsets, one call per chunk): hT, dzT_t and db_p of
    chunked lstm_seq_fwd / lstm_seq_bwd calls."""
    B, T, n_in = 20, 7, 8
    x, W, b, (wx_t, wh_t, wh_p, wx_p, bias_p), xin, tdt = _lstm_setup(ops, B, T, n_in, u, dt, seed=8)
    assert not ops.lstm_fused_outputs(tdt, u)
    xproj = torch.empty((T, B, 4 * u), device=DEV)
    ops.gemm_tn(xin.view(T * B, -1), wx_t, xproj.view(T * B, -1), bias=bias_p)
    gates, c, h = torch.zeros((T, B, 4 * u), device=DEV), torch.zeros((T, B, u), device=DEV), torch.zeros((T, B, u), device=DEV, dtype=tdt)
    Np = ops.round_up(T * B, 64)
    hT = torch.full((u, Np), 7.0, device=DEV, dtype=tdt)
    for t0, t1 in [(0, 3), (3, 4), (4, 7)]:
        ops.lstm_seq_fwd(xproj, wh_t, None, None, gates, c, h, t0, t1, hT)
    assert torch.equal(hT[:, B:T * B], h[:-1].reshape((T - 1) * B, u).t())
    assert bool((hT[:, :B] == 7.0).all()) and bool((hT[:, T * B:] == 7.0).all())          # columns [0, B) (and the padding) stay as given
    dy = dev(np.random.default_rng(1).standard_normal((T, B, u)).astype(np.float32))
    dz = torch.zeros((T, B, 4 * u), device=DEV)
    dz16 = dz if dt == "f32" else torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt)
    dzT_t = torch.full((4 * u, Np), 7.0, device=DEV, dtype=tdt)
    db_p = torch.zeros(4 * u, device=DEV)
    ws = ops.lstm_seq_bwd_workspace(B, u, DEV)
    chunks = [(5, 7), (2, 5), (0, 2)]
    for t0, t1 in chunks:
        ops.lstm_seq_bwd(dy, wh_p, gates, c, None, dz, dz16, None, None, t0, t1, ws, dzT_t, db_p)
    assert torch.equal(dzT_t[:, :T * B], dz16.view(T * B, 4 * u).t()) and bool((dzT_t[:, T * B:] == 7.0).all())
    # column sums of the f32 dz, one mnn_bias_grad per chunk accumulating into db_p: a term passes through at most k roundings of its
    # thread's chain (k = the longest chunk's rows / 4 waves; one row slab per call), 8 of the workgroup's tree and g atomics (one per call)
    dzf = dz.view(T * B, 4 * u).double().cpu().numpy()
    k, g = max(-(-(t1 - t0) * B // 4) for t0, t1 in chunks), len(chunks)
    assert (np.abs(db_p.cpu().numpy() - dzf.sum(0)) <= (k + 8 + g) * 2.0 ** -24 * np.abs(dzf).sum(0)).all()
    assert float(db_p.abs().max()) > 0


def test_lstm_initial_state_and_dh0(ops):
    B, T, n_in, u = 9, 3, 8, 32
    x, W, b, (wx_t, wh_t, wh_p, wx_p, bias_p), xin, tdt = _lstm_setup(ops, B, T, n_in, u, "f32", seed=5)
    R = np.random.default_rng(6)
    h0 = (R.standard_normal((B, u)) * .5).astype(np.float32)
    c0 = (R.standard_normal((B, u)) * .5).astype(np.float32)
    xproj = torch.empty((T, B, 4 * u), device=DEV)
    ops.gemm_tn(xin.view(T * B, -1), wx_t, xproj.view(T * B, -1), bias=bias_p)
    gates = torch.empty((T, B, 4 * u), device=DEV); c = torch.empty((T, B, u), device=DEV); h = torch.empty((T, B, u), device=DEV)
    ops.lstm_seq_fwd(xproj, wh_t, dev(h0), dev(c0), gates, c, h)
    layers = [(W.astype(np.float64), b.astype(np.float64))]
    y, st, cache = olstm.seq_fwd(x.astype(np.float64), layers, init_state=[(c0.astype(np.float64), h0.astype(np.float64))])
    assert rel(h.cpu().numpy().transpose(1, 0, 2), y) < 2e-5
    # d h0 / d c0 by finite differences of sum(y * dy)
    dy = R.standard_normal((B, T, u))
    dz = torch.empty((T, B, 4 * u), device=DEV); dh0 = torch.empty((B, u), device=DEV); dc0 = torch.empty((B, u), device=DEV)
    ops.lstm_seq_bwd(dev(dy.transpose(1, 0, 2).astype(np.float32)), wh_p, gates, c, dev(c0), dz, dz, dh0, dc0)
    f = lambda hh, cc: float((olstm.seq_fwd(x.astype(np.float64), layers, init_state=[(cc, hh)])[0] * dy).sum())
    for (bi, j) in [(0, 0), (3, 7), (8, 31)]:
        e = np.zeros((B, u)); e[bi, j] = 1e-5
        fdh = (f(h0 + e, c0.astype(np.float64)) - f(h0 - e, c0.astype(np.float64))) / 2e-5
        fdc = (f(h0.astype(np.float64), c0 + e) - f(h0.astype(np.float64), c0 - e)) / 2e-5
        assert abs(fdh - float(dh0[bi, j])) < 1e-4 * max(1, abs(fdh))
        assert abs(fdc - float(dc0[bi, j])) < 1e-4 * max(1, abs(fdc))


def test_dropout_matches_contract(ops):
    T, B, u = 3, 5, 32
    R = np.random.default_rng(4)
    h = R.standard_normal((T, B, u)).astype(np.float32)
    y = torch.empty((T, B, u), device=DEV)
    ops.dropout_fwd(dev(h), y, 0.9, seed=23, row0=100, layer=1)
    uu = np.stack([philox.uniform_block(23, philox.STREAM_DROPOUT, np.arange(100, 100 + B), (t << 8) | 1, u) for t in range(T)])
    ref, keep = S.dropout_output(h, 0.9, uu)
    assert np.array_equal(y.cpu().numpy(), ref)
    dh = torch.ones((T, B, u), device=DEV)
    ops.dropout_bwd(dev(h), dh, 0.9, 23, 100, 1, accumulate=True)
    # device-side step counter: seed_eff = seed + *step_dev
    y3 = torch.empty((T, B, u), device=DEV)
    ops.dropout_fwd(dev(h), y3, 0.9, seed=20, row0=100, layer=1, step_dev=torch.tensor([3], device=DEV, dtype=torch.int32))
    assert torch.equal(y3, y)
    y4 = torch.empty((T - 1, B, u), device=DEV)
    ops.dropout_fwd(dev(h[1:]), y4, 0.9, seed=23, row0=100, layer=1, t_offset=1)       # chunk starting at t = 1
    assert torch.equal(y4, y[1:])
    assert np.allclose(dh.cpu().numpy(), 1 + h / np.float32(0.9) * keep, rtol=1e-6)
    y2 = torch.empty((T, B, u), device=DEV)
    ops.dropout_fwd(dev(h), y2, 1.0, 23, 100, 1)
    assert np.array_equal(y2.cpu().numpy(), h)
    # the keep masks the recurrences read: 16 flags per thread (u % 16 == 0) and 4 per thread (u = 20) against the same counters
    for uw in (32, 20):
        mk = torch.zeros((T, B, uw), device=DEV, dtype=torch.uint8)
        ops.dropout_mask(mk, 0.9, 23, 100, 1)
        uw_u = np.stack([philox.uniform_block(23, philox.STREAM_DROPOUT, np.arange(100, 100 + B), (t << 8) | 1, uw) for t in range(T)])
        assert np.array_equal(mk.cpu().numpy(), np.floor(np.float32(0.9) + uw_u).astype(np.uint8))
    assert np.array_equal(mk.cpu().numpy() * 0 + keep[:, :, :20].astype(np.uint8), np.floor(np.float32(0.9) + uu[:, :, :20]).astype(np.uint8))


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,Hn,tracks", [(70, 24, 16, 1), (130, 88, 256, 1), (64, 20, 100, 3), (5, 440, 256, 1), (33, 17, 7, 2)])
def test_nade_logprob_fwd_bwd(ops, N, D, Hn, tracks):
    R = np.random.default_rng(N + D)
    ld = tracks * (Hn + D) + 3
    bias = (R.standard_normal((N, ld)) * .5).astype(np.float32)
    we = (R.standard_normal((tracks, D, Hn)) * .3).astype(np.float32)
    wd = (R.standard_normal((tracks, D, Hn)) * .3).astype(np.float32)
    v = (R.random((tracks, N, D)) < .2).astype(np.uint8)
    rw = R.random(N).astype(np.float32) / N
    bt = dev(bias)
    nll = torch.zeros((tracks, N), device=DEV); cp = torch.zeros((tracks, N, D), device=DEV)
    d_bias = torch.zeros_like(bt)
    a_fin = torch.zeros((tracks, N, Hn), device=DEV)
    ops.nade_logprob_fwd(dev(v), bt, dev(we), dev(wd), tracks, D, Hn, dev(rw), nll, cp, d_bias, a_fin)
    dwe = torch.zeros((tracks, D, Hn), device=DEV); dwd = torch.zeros((tracks, D, Hn), device=DEV)
    ops.nade_logprob_bwd(dev(v), bt, dev(we), dev(wd), tracks, D, Hn, a_fin, d_bias, dwe, dwd)
    f8 = np.float64
    for m in range(tracks):
        be = bias[:, m * Hn:(m + 1) * Hn].astype(f8)
        bd = bias[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D].astype(f8)
        n_ref, c_ref = onade.log_prob(v[m].astype(f8), be, bd, we[m].astype(f8), wd[m].astype(f8))
        assert rel(nll[m].cpu().numpy(), n_ref) < 2e-5
        assert np.abs(cp[m].cpu().numpy() - c_ref).max() < 1e-6
        g = onade.log_prob_bwd(v[m].astype(f8), be, bd, we[m].astype(f8), wd[m].astype(f8), rw.astype(f8))
        db = d_bias.cpu().numpy()
        assert rel(db[:, m * Hn:(m + 1) * Hn], g[0]) < 1e-4
        assert rel(db[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D], g[1]) < 1e-4
        assert rel(dwe[m].cpu().numpy(), g[2]) < 1e-4
        assert rel(dwd[m].cpu().numpy(), g[3]) < 1e-4


@pytest.mark.parametrize("N,D,tracks,rho", [(70, 100, 1, 0.05), (64, 440, 1, 0.03), (33, 31, 2, 0.5), (40, 65, 1, 1.0), (5, 440, 1, 0.0)])
def test_nade_mfma_forward_matches_f32_kernel(ops, N, D, tracks, rho):
    """Matrix-core NADE forward (bf16 states and decoder weights, f32 accumulation) against the f32 VALU kernel on the
    same inputs: p within bf16 rounding of the logits, a_final identical up to f32 summation order; dense rows (rho = 1:
    more than 32 flips per column tile) exercise the chunked flip path."""
    Hn = 256
    g = torch.Generator(device="cuda").manual_seed(N + D)
    v = (torch.rand((tracks, N, D), device="cuda", generator=g) < rho).to(torch.uint8)
    bias = torch.randn((N, tracks * (Hn + D)), device="cuda", generator=g) * 0.5
    we = torch.randn((tracks, D, Hn), device="cuda", generator=g) * 0.1
    wd = torch.randn((tracks, D, Hn), device="cuda", generator=g) * 0.1
    rw = torch.rand(N, device="cuda", generator=g)
    z = lambda *s: torch.zeros(s, device="cuda")
    nll0, cp0, db0, af0 = z(tracks, N), z(tracks, N, D), torch.zeros_like(bias), z(tracks, N, Hn)
    ops.nade_logprob_fwd(v, bias, we, wd, tracks, D, Hn, rw, nll0, cp0, db0, af0)
    nll1, cp1, db1, af1 = z(tracks, N), z(tracks, N, D), torch.zeros_like(bias), z(tracks, N, Hn)
    ops.nade_logprob_fwd_mfma(v, bias, we, wd.to(torch.bfloat16), tracks, D, Hn, rw, nll1, cp1, db1, af1)
    assert float((cp0 - cp1).abs().max()) < 1.5e-2
    assert torch.allclose(nll0, nll1, rtol=5e-3, atol=5e-2)
    assert float((db0 - db1).abs().max()) < 1.5e-2
    assert torch.allclose(af0, af1, rtol=1e-5, atol=1e-5)
    ops.nade_logprob_fwd_mfma(v, bias, we, wd.to(torch.bfloat16), tracks, D, Hn, rw, nll0, cp0, db0, af0)
    assert torch.equal(nll0, nll1) and torch.equal(cp0, cp1)            # deterministic


@pytest.mark.parametrize("N,D,tracks,rho", [(70, 100, 1, 0.05), (96, 440, 1, 0.03), (64, 440, 1, 0.5), (33, 31, 2, 0.5), (40, 65, 1, 1.0), (5, 440, 1, 0.0)])
def test_nade_mfma_exact_forward_vs_oracle(ops, N, D, tracks, rho):
    """Split-operand matrix-core NADE forward (precision "fp16": hidden states and decoder weights as f16 hi + lo pairs, three 16-bit MFMA
    products per logit, f32 accumulation) against the float64 oracle (nade.py:155-229): every conditional within 1e-5 absolute, per-row NLL
    within 2e-5 relative (the f32 vector scan's own level), d nll / d b_dec within 1e-4 of its scale, a_final as exact as the f32 kernel's;
    the pack kernel splits w_dec into hi = f16(w) and lo = f16(w - hi)."""
    Hn = 256
    R = np.random.default_rng(N + D)
    ld = tracks * (Hn + D)
    bias = (R.standard_normal((N, ld)) * .5).astype(np.float32)
    we = (R.standard_normal((tracks, D, Hn)) * .1).astype(np.float32)
    wd = (R.standard_normal((tracks, D, Hn)) * .1).astype(np.float32)
    v = (R.random((tracks, N, D)) < rho).astype(np.uint8)
    rw = (R.random(N) / N).astype(np.float32)
    wpk = torch.empty((tracks * D, Hn), device=DEV)
    ops.nade_f32_pack(dev(wd).view(tracks * D, Hn), wpk)
    q = wpk.view(torch.float16).view(tracks * D, 2, Hn).float().cpu().numpy()       # f16 [row][hi | lo][Hn]: hi = f16(w), lo = f16(w - hi)
    assert np.array_equal(q[:, 0], wd.reshape(-1, Hn).astype(np.float16).astype(np.float32))
    assert np.abs(q[:, 0] + q[:, 1] - wd.reshape(-1, Hn)).max() < 2.0 ** -21 * np.abs(wd).max()
    z = lambda *s_: torch.zeros(s_, device=DEV)
    nll, cp, db, af = z(tracks, N), z(tracks, N, D), z(N, ld), z(tracks, N, Hn)
    ops.nade_logprob_fwd_auto(dev(v), dev(bias), dev(we), dev(wd), wpk.view(tracks, D, Hn), tracks, D, Hn, None, None, 1.0, dev(rw), nll, cp, db, af,
                              exact=True)
    f8 = np.float64
    for m in range(tracks):
        be = bias[:, m * Hn:(m + 1) * Hn].astype(f8)
        bd = bias[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D].astype(f8)
        n_ref, c_ref = onade.log_prob(v[m].astype(f8), be, bd, we[m].astype(f8), wd[m].astype(f8))
        e_cp = np.abs(cp[m].cpu().numpy() - c_ref).max()
        e_nll = np.abs(nll[m].cpu().numpy() - n_ref).max() / np.abs(n_ref).max()
        print(f"\n[exact N={N} D={D} rho={rho} track {m}] cond_p abs {e_cp:.2e}  nll rel {e_nll:.2e}")
        assert e_cp < 1e-5 and e_nll < 2e-5
        g = onade.log_prob_bwd(v[m].astype(f8), be, bd, we[m].astype(f8), wd[m].astype(f8), rw.astype(f8))
        assert rel(db.cpu().numpy()[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D], g[1]) < 1e-4
        a_ref = be + (v[m].astype(f8) @ we[m].astype(f8))
        assert np.abs(af[m].cpu().numpy() - a_ref).max() < 1e-4
    nll2, cp2 = z(tracks, N), z(tracks, N, D)
    ops.nade_logprob_fwd_auto(dev(v), dev(bias), dev(we), dev(wd), wpk.view(tracks, D, Hn), tracks, D, Hn, None, None, 1.0, None, nll2, cp2, None, None,
                              exact=True)
    assert torch.equal(nll, nll2) and torch.equal(cp, cp2)              # deterministic


@pytest.mark.parametrize("rho,expect", [(0.03, 0), (0.3, 1)])
def test_nade_forward_density_gate(ops, rho, expect):
    """mnn_density_gate + the two gated launches: a sparse batch runs the matrix-core form (bit-identical to calling it directly), a dense
    one the f32 vector form (the same exact pre-activations; its hidden states advanced multiplicatively since round 6, so conditionals and NLL
    agree with the direct-sigmoid entry point to 2e-5: test_nade_dense_forward_multiplicative_states_vs_direct_form); the scratch count word is
    left zero and the decision is taken on the device at every call."""
    N, D, Hn, tracks = 96, 120, 256, 1
    g = torch.Generator(device="cuda").manual_seed(int(rho * 100))
    v = (torch.rand((tracks, N, D), device="cuda", generator=g) < rho).to(torch.uint8)
    bias = torch.randn((N, tracks * (Hn + D)), device="cuda", generator=g) * 0.5
    we = torch.randn((tracks, D, Hn), device="cuda", generator=g) * 0.1
    wd = torch.randn((tracks, D, Hn), device="cuda", generator=g) * 0.1
    wdb = wd.to(torch.bfloat16)
    rw = torch.rand(N, device="cuda", generator=g)
    z = lambda *s_: torch.zeros(s_, device="cuda")
    gate = torch.full((1 + ops.DENSITY_SLOTS,), 7, device="cuda", dtype=torch.int32)          # [gate | partial counts (zeroed scratch, left zero)]
    gate[1:] = 0
    nll, cp, db, af = z(tracks, N), z(tracks, N, D), torch.zeros_like(bias), z(tracks, N, Hn)
    ops.nade_logprob_fwd_auto(v, bias, we, wd, wdb, tracks, D, Hn, gate[:1], gate[1:], 0.07, rw, nll, cp, db, af)
    assert int(gate[0]) == expect and not bool(gate[1:].any())
    nll2, cp2, db2, af2 = z(tracks, N), z(tracks, N, D), torch.zeros_like(bias), z(tracks, N, Hn)
    if expect:
        ops.nade_logprob_fwd(v, bias, we, wd, tracks, D, Hn, rw, nll2, cp2, db2, af2)
        assert torch.equal(af, af2) and float((cp - cp2).abs().max()) < 2e-5 and float((nll - nll2).abs().max()) < 2e-5 * float(nll2.abs().max())
        assert float((db - db2).abs().max()) < 1e-4 * float(db2.abs().max())
    else:
        ops.nade_logprob_fwd_mfma(v, bias, we, wdb, tracks, D, Hn, rw, nll2, cp2, db2, af2)
        assert torch.equal(nll, nll2) and torch.equal(cp, cp2) and torch.equal(db, db2) and torch.equal(af, af2)
    # the same buffers, the other kind of batch: the decision follows the data
    v2 = (torch.rand((tracks, N, D), device="cuda", generator=g) < (0.3 if not expect else 0.02)).to(torch.uint8)
    ops.nade_logprob_fwd_auto(v2, bias, we, wd, wdb, tracks, D, Hn, gate[:1], gate[1:], 0.07, rw, nll, cp, db, af)
    assert int(gate[0]) == 1 - expect and not bool(gate[1:].any())
    # counts taken elsewhere (the piano-roll pass): only the decision runs, from the partial counts
    gate[1:4] = torch.tensor([int(0.05 * v.numel()), int(0.05 * v.numel()), 3], device="cuda", dtype=torch.int32)
    ops.nade_logprob_fwd_auto(v2, bias, we, wd, wdb, tracks, D, Hn, gate[:1], gate[1:], 0.07, rw, nll, cp, db, af, counted=True)
    assert int(gate[0]) == 1 and not bool(gate[1:].any())


def test_nade_edge_cases(ops):
    # K1: zero weights -> p = .5 and NLL = -D log(0.500001); all-ones / all-zeros visibles
    N, D, Hn = 3, 440, 256
    z = lambda *s: torch.zeros(s, device=DEV)
    for fill in (0, 1):
        v = torch.full((1, N, D), fill, device=DEV, dtype=torch.uint8)
        nll, cp = z(1, N), z(1, N, D)
        ops.nade_logprob_fwd(v, z(N, Hn + D), z(1, D, Hn), z(1, D, Hn), 1, D, Hn, None, nll, cp)
        assert np.allclose(cp.cpu().numpy(), 0.5, atol=1e-7)
        assert np.allclose(nll.cpu().numpy(), 304.98388, rtol=1e-6)
    with pytest.raises(ValueError):
        ops.nade_logprob_fwd(v, z(N, Hn + D), z(1, D, 300), z(1, D, 300), 1, D, 300)   # Hn > 256


@pytest.mark.parametrize("N,D,Hn,tracks,temp", [(9, 40, 64, 1, 1.0), (6, 88, 256, 2, 1.0), (5, 30, 100, 1, 0.7), (4, 25, 20, 1, None),
                                                (7, 440, 256, 1, 1.0), (5, 333, 256, 3, 1.0), (4, 88, 256, 5, 0.5), (3, 130, 252, 1, None), (3, 61, 30, 2, 1.0),
                                                (4, 12, 64, 1, 1.0), (4, 7, 256, 2, 1.0), (300, 24, 256, 1, 1.0)])
def test_nade_sample_bit_exact(ops, N, D, Hn, tracks, temp):
    """Hn % 4 == 0: the eight-visibles-per-pass kernel (nade_sample_chunk_kernel; D = 333 x 3 tracks: chunks, track offsets and Philox windows
    that do not line up; 440 x 256: the joint generator's shape; D = 12 / 7: less than one chunk; 300 rows: more rows than CUs, the chunks of 8);
    other widths: the visible-at-a-time kernel."""
    R = np.random.default_rng(Hn)
    ld = tracks * (Hn + D)
    bias = (R.standard_normal((N, ld)) * .5).astype(np.float32)
    we = (R.standard_normal((tracks, D, Hn)) * .3).astype(np.float32)
    wd = (R.standard_normal((tracks, D, Hn)) * .3).astype(np.float32)
    out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
    nll = torch.zeros((tracks, N), device=DEV)
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, temp, seed=77, row0=1000, sub=5, samples=out, nll=nll)
    got = out.cpu().numpy()
    u = philox.uniform_block(77, philox.STREAM_NADE, np.arange(1000, 1000 + N), 5, tracks * D)
    for m in range(tracks):
        s_ref, p_ref = det.nade_sample(bias, we[m], wd[m], tracks, m, D, Hn, temp, u[:, m * D:(m + 1) * D])
        assert np.array_equal(got[:, m * D:(m + 1) * D], s_ref), "Bernoulli draws must be bit-exact"
        be = bias[:, m * Hn:(m + 1) * Hn].astype(np.float64)
        bd = bias[:, tracks * Hn + m * D: tracks * Hn + (m + 1) * D].astype(np.float64)
        n64, _ = onade.log_prob(s_ref.astype(np.float64), be, bd, we[m].astype(np.float64), wd[m].astype(np.float64))
        assert rel(nll[m].cpu().numpy(), n64) < 1e-5
    # track-minor output layout (rnn_multinade.py:313-314)
    out2 = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
    ops.nade_sample(dev(bias), dev(we), dev(wd), tracks, D, Hn, temp, 77, 1000, 5, out2, track_minor=True)
    assert np.array_equal(out2.cpu().numpy().reshape(N, D, tracks).transpose(0, 2, 1).reshape(N, tracks * D), got)


@pytest.mark.parametrize("scale", [0.3, 3.0])
def test_nade_sample_chunked_passes_equal_the_visible_at_a_time_scan(ops, monkeypatch, scale):
    """The three forms of the sampling scan on the same inputs (MNN_SAMPLE_G8 / MNN_SAMPLE_NO_CHUNK select the narrower pass / the
    visible-at-a-time kernel, read per call): draws and
    NLL bit for bit, at the joint generator's shape with piano-roll-like (b_dec ~ -3.5) and coin-flip conditionals, all three temperature modes.
    scale 3: half the visibles flip the state -- most passes restart inside their chunk."""
    N, D, Hn, tracks = 40, 440, 256, 2
    g = torch.Generator(device=DEV).manual_seed(5)
    ld = tracks * (Hn + D)
    bias = torch.randn((N, ld), device=DEV, generator=g) * 0.5
    if scale < 1:
        bias[:, tracks * Hn:] -= 3.5
    we = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1 * scale
    wd = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1 * scale
    for temp in (1.0, 0.8, None):
        res = []
        for form in ("chunks of 16", "chunks of 8", "visible at a time"):
            monkeypatch.delenv("MNN_SAMPLE_NO_CHUNK", raising=False)
            monkeypatch.delenv("MNN_SAMPLE_G8", raising=False)
            if form == "chunks of 8":
                monkeypatch.setenv("MNN_SAMPLE_G8", "1")
            elif form == "visible at a time":
                monkeypatch.setenv("MNN_SAMPLE_NO_CHUNK", "1")
            out = torch.zeros((N, tracks * D), device=DEV, dtype=torch.uint8)
            nll = torch.zeros((tracks, N), device=DEV)
            ops.nade_sample(bias, we, wd, tracks, D, Hn, temp, seed=9, row0=77, sub=3, samples=out, nll=nll)
            torch.cuda.synchronize()
            res.append((out, nll))
        assert torch.equal(res[0][0], res[2][0]) and torch.equal(res[0][1], res[2][1]), temp
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), temp
        m = float(res[0][0].float().mean())
        assert (0.005 < m < 0.2) if scale < 1 and temp is not None else True, m


def test_nade_sample_near_ties_take_the_exact_comparison(ops):
    """The sampling kernel settles a draw from the hardware exp2 / rcp probability unless the decision is within 1e-4 of a tie and
    then compares exactly.  Force the tie path: threshold draws (temperature None -> p >= 0.5, nade.py:278-279) with all-zero weights
    and b_dec in {0, +-1e-7, +-3e-6, +-1}: the logit IS b_dec and det_sigmoid(+-tiny) rounds to exactly 0.5 or not -- the oracle's
    float32 restatement decides, the kernel must agree on every visible (Hn = 256: the specialised kernel; Hn = 40: the generic one)."""
    N, D = 6, 64
    vals = np.array([0.0, 1e-7, -1e-7, 3e-6, -3e-6, 1.0, -1.0, 5.9e-8, -5.9e-8, 2e-5, -2e-5], np.float32)
    R = np.random.default_rng(2)
    for Hn in (256, 40):
        bias = np.zeros((N, Hn + D), np.float32)
        bias[:, Hn:] = vals[R.integers(0, len(vals), (N, D))]
        we = np.zeros((1, D, Hn), np.float32)
        wd = np.zeros((1, D, Hn), np.float32)
        out = torch.zeros((N, D), device=DEV, dtype=torch.uint8)
        ops.nade_sample(dev(bias), dev(we), dev(wd), 1, D, Hn, None, seed=1, row0=0, sub=0, samples=out)
        u = np.zeros((N, D), np.float32)
        s_ref, _ = det.nade_sample(bias, we[0], wd[0], 1, 0, D, Hn, None, u)
        assert np.array_equal(out.cpu().numpy(), s_ref)
        assert 0 < s_ref.mean() < 1


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,Hn,k,bcast", [(20, 88, 256, 10, False), (9, 30, 20, 3, True), (17, 440, 64, 2, False), (5, 12, 7, 0, False),
                                            (2101, 88, 256, 2, False), (2050, 40, 100, 2, True), (33, 200, 130, 2, False), (2049, 130, 200, 1, False),
                                            (40, 200, 100, 2, False), (2060, 200, 100, 1, True), (2053, 13, 21, 3, False), (2048, 12, 7, 0, False),
                                            (4096, 88, 256, 10, False), (2050, 300, 280, 1, False)])
def test_rbm_gibbs_bit_exact(ops, N, D, Hn, k, bcast):
    """Below 2048 rows with D, Hn <= 256: W resident in LDS, two rows per workgroup (rows split over spare threads when a phase has
    at most 128 outputs); from 2048 rows on the chain runs on the f32 matrix cores (v_mfma_f32_32x32x2_f32 = the same ascending fmaf chain:
    odd widths, widths that are no multiple of the 32-unit tile, a shared bias row, k = 0) while W and the byte states fit LDS, else the
    streaming kernel (the last shape).  Every form must reproduce the oracle's draws and probabilities."""
    R = np.random.default_rng(D)
    W = (R.standard_normal((D, Hn)) * .3).astype(np.float32)
    bh = (R.standard_normal((1 if bcast else N, Hn)) * .3).astype(np.float32)
    bv = (R.standard_normal((1 if bcast else N, D)) * .3).astype(np.float32)
    v0 = (R.random((N, D)) < .1).astype(np.uint8)
    rows = np.arange(500, 500 + N)
    u_h, u_v = G.gibbs_uniforms(11, rows, k, Hn, D, sub0=3)
    p_ref, v_ref = det.rbm_gibbs(v0, W, bh, bv, k, u_h, u_v)
    p_v = torch.zeros((N, D), device=DEV); v_out = torch.zeros((N, D), device=DEV, dtype=torch.uint8)
    ops.rbm_gibbs(dev(v0), dev(W), dev(bh), dev(bv), k, seed=11, row0=500, sub0=3, p_v=p_v, v_out=v_out)
    assert np.array_equal(v_out.cpu().numpy(), v_ref), "Gibbs samples must be bit-exact"
    assert np.array_equal(p_v.cpu().numpy(), p_ref)
    if N <= 64:
        p64, v64 = orbm.gibbs(v0.astype(np.float64), W.astype(np.float64), bh.astype(np.float64), bv.astype(np.float64), k, u_h, u_v)
        assert np.abs(p_v.cpu().numpy() - p64).max() < 1e-6 or not np.array_equal(v_ref, v64.astype(np.uint8))
    # row_ids path
    ids = dev(rows.astype(np.int32))
    v2 = torch.zeros((N, D), device=DEV, dtype=torch.uint8)
    ops.rbm_gibbs(dev(v0), dev(W), dev(bh), dev(bv), k, seed=11, row0=0, row_ids=ids, sub0=3, v_out=v2)
    assert np.array_equal(v2.cpu().numpy(), v_ref)


def test_rbm_half_steps_and_free_energy(ops):
    R = np.random.default_rng(8)
    N, D, Hn = 21, 88, 256
    W = (R.standard_normal((D, Hn)) * .3).astype(np.float32)
    bh = (R.standard_normal((N, Hn)) * .3).astype(np.float32)
    bv = (R.standard_normal((1, D)) * .3).astype(np.float32)
    v = (R.random((N, D)) < .2).astype(np.uint8)
    p_h = torch.zeros((N, Hn), device=DEV); h = torch.zeros((N, Hn), device=DEV, dtype=torch.uint8)
    ops.rbm_hidden(dev(v), dev(W), dev(bh), philox.STREAM_DBN_ENC, 5, 40, 2, p_h, h)
    ph_ref = det.rbm_hidden(v, W, bh)
    assert np.array_equal(p_h.cpu().numpy(), ph_ref)
    u = philox.uniform_block(5, philox.STREAM_DBN_ENC, np.arange(40, 40 + N), 2, Hn)
    assert np.array_equal(h.cpu().numpy(), (u < ph_ref).astype(np.uint8))
    p_v = torch.zeros((N, D), device=DEV); vs = torch.zeros((N, D), device=DEV, dtype=torch.uint8)
    ops.rbm_visible(h, dev(W), dev(bv), philox.STREAM_DBN_DEC, 5, 40, 2, p_v, vs)
    pv_ref = det.rbm_visible(h.cpu().numpy(), W, bv)
    assert np.array_equal(p_v.cpu().numpy(), pv_ref)
    u = philox.uniform_block(5, philox.STREAM_DBN_DEC, np.arange(40, 40 + N), 2, D)
    assert np.array_equal(vs.cpu().numpy(), (u < pv_ref).astype(np.uint8))
    # float input path (probabilities as input)
    p_h2 = torch.zeros((N, Hn), device=DEV)
    ops.rbm_hidden(p_v, dev(W), dev(bh), 0, 0, 0, 0, p_h2, None)
    assert rel(p_h2.cpu().numpy(), orbm.cond_prob_h(pv_ref.astype(np.float64), W.astype(np.float64), bh.astype(np.float64))) < 1e-5
    F = torch.zeros(N, device=DEV)
    ops.rbm_free_energy(dev(v), dev(W), dev(bh), dev(bv), F)
    F_ref = orbm.free_energy(v.astype(np.float64), W.astype(np.float64), bh.astype(np.float64), bv.astype(np.float64))
    assert rel(F.cpu().numpy(), F_ref) < 1e-5
    # K7: W = 0, bh = 0 -> F = -Hn log 2 - v.bv
    ops.rbm_free_energy(dev(v), torch.zeros((D, Hn), device=DEV), torch.zeros((1, Hn), device=DEV), dev(bv), F)
    assert rel(F.cpu().numpy(), -Hn * np.log(2) - (v * bv).sum(1)) < 1e-6


@pytest.mark.parametrize("N,D,Hn", [(2100, 88, 168), (2049, 168, 84), (2051, 13, 21)])
def test_rbm_half_steps_on_the_matrix_cores_bit_exact(ops, N, D, Hn):
    """From 2048 rows on the half-steps run on v_mfma_f32_32x32x2_f32 (rbm_half_mfma_kernel): probabilities and draws bit-identical to the
    deterministic checker -- byte and float inputs, per-row and shared bias rows, widths that are odd / no multiple of the 32-unit tile."""
    R = np.random.default_rng(N)
    W = (R.standard_normal((D, Hn)) * .3).astype(np.float32)
    bh = (R.standard_normal((N, Hn)) * .3).astype(np.float32)
    bv = (R.standard_normal((1, D)) * .3).astype(np.float32)
    v = (R.random((N, D)) < .2).astype(np.uint8)
    p_h = torch.zeros((N, Hn), device=DEV); h = torch.zeros((N, Hn), device=DEV, dtype=torch.uint8)
    ops.rbm_hidden(dev(v), dev(W), dev(bh), philox.STREAM_DBN_ENC, 5, 40, 2, p_h, h)
    ph_ref = det.rbm_hidden(v, W, bh)
    assert np.array_equal(p_h.cpu().numpy(), ph_ref)
    u = philox.uniform_block(5, philox.STREAM_DBN_ENC, np.arange(40, 40 + N), 2, Hn)
    assert np.array_equal(h.cpu().numpy(), (u < ph_ref).astype(np.uint8))
    p_v = torch.zeros((N, D), device=DEV); vs = torch.zeros((N, D), device=DEV, dtype=torch.uint8)
    ops.rbm_visible(h, dev(W), dev(bv), philox.STREAM_DBN_DEC, 5, 40, 2, p_v, vs)
    pv_ref = det.rbm_visible(h.cpu().numpy(), W, bv)
    assert np.array_equal(p_v.cpu().numpy(), pv_ref)
    u = philox.uniform_block(5, philox.STREAM_DBN_DEC, np.arange(40, 40 + N), 2, D)
    assert np.array_equal(vs.cpu().numpy(), (u < pv_ref).astype(np.uint8))
    p_h2 = torch.zeros((N, Hn), device=DEV); h2 = torch.zeros((N, Hn), device=DEV, dtype=torch.uint8)      # float inputs (probabilities)
    ops.rbm_hidden(p_v, dev(W), dev(bh), philox.STREAM_DBN_ENC, 5, 40, 3, p_h2, h2)
    assert np.array_equal(p_h2.cpu().numpy(), det.rbm_hidden(pv_ref, W, bh))
    p_h3 = torch.zeros((N, Hn), device=DEV)                                # probabilities only: the vector kernel, same bits
    ops.rbm_hidden(p_v, dev(W), dev(bh), 0, 0, 0, 0, p_h3, None)
    assert torch.equal(p_h3, p_h2)


# ------------------------------------------------------------------------------------------------
def test_reductions_and_adam(ops):
    R = np.random.default_rng(10)
    n = 100003
    g = R.standard_normal(n).astype(np.float32) * 3
    th = R.standard_normal(n).astype(np.float32)
    out = torch.zeros(1, device=DEV)
    ops.sumsq(dev(g), out)
    assert rel(out.cpu().numpy(), (g.astype(np.float64) ** 2).sum()) < 1e-5
    w = R.random(n).astype(np.float32)
    o2 = torch.zeros(1, device=DEV)
    ops.weighted_sum(dev(g), dev(w), o2)
    assert abs(float(o2) - float((g.astype(np.float64) * w).sum())) < 1e-2
    tht, m, v = dev(th), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ref_th, ref_m, ref_v = th.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        clipped, gn = S.clip_by_global_norm([g.astype(np.float64)], 5.0)
        ref_th, ref_m, ref_v = S.adam_tf_step(ref_th, clipped[0], ref_m, ref_v, step, 0.01)
        ops.clip_adam_step(tht, dev(g), m, v, out, 5.0, 0.01, 0.9, 0.999, 1e-4, step)
    th_d, m_d, v_d = dev(th), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sd = torch.zeros(1, device=DEV, dtype=torch.int32)
    for step in (1, 2, 3):          # same three steps with the counter on the device
        ops.clip_adam_step(th_d, dev(g), m_d, v_d, out, 5.0, 0.01, 0.9, 0.999, 1e-4, 0, step_dev=sd)
        ops.step_increment(sd)
    assert int(sd) == 3 and rel(th_d.cpu().numpy(), tht.cpu().numpy()) < 1e-6
    assert rel(tht.cpu().numpy(), ref_th) < 1e-5 and rel(m.cpu().numpy(), ref_m) < 1e-5 and rel(v.cpu().numpy(), ref_v) < 5e-5   # beta2 = 0.999f carries a 1.3e-5 relative error in (1-beta2), as in TF's f32 kernel
    th2 = dev(th)
    ops.clip_adam_step(th2, dev(g), None, None, None, 0.0, 0.1, 0.9, 0.999, 1e-4, 1, sgd=True)
    assert rel(th2.cpu().numpy(), th - 0.1 * g) < 1e-6
    dY = R.standard_normal((1000, 70)).astype(np.float32)
    db = torch.ones(70, device=DEV)
    ops.bias_grad(dev(dY), db, accumulate=True)
    assert rel(db.cpu().numpy(), 1 + dY.astype(np.float64).sum(0)) < 1e-5


def test_eval_counts_and_log_loss_rows(ops):
    """N1: the raw sums behind tf.metrics.accuracy / precision / recall (statistical.py:28-32) and tf.losses.log_loss summed over
    the visibles (pass_encoder.py:81-86): integer counts exact, costs to f32 rounding against float64 NumPy."""
    rng = np.random.default_rng(5)
    N, D = 1000, 440
    t = (rng.random((N, D)) < 0.1).astype(np.uint8)
    p = (rng.random((N, D)) < 0.12).astype(np.uint8)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    ops.eval_counts(dev(t), dev(p), cnt)
    ops.eval_counts(dev(t), dev(p), cnt)                                           # accumulates
    tb, pb = t.astype(bool), p.astype(bool)
    ref = np.array([(tb & pb).sum(), (~tb & pb).sum(), (tb & ~pb).sum(), (tb == pb).sum()]) * 2
    assert np.array_equal(cnt.cpu().numpy(), ref)
    probs = rng.random((N, D)).astype(np.float32)
    probs[0, :5] = [0.0, 1.0, 1e-9, 1 - 1e-7, 0.5]
    out = torch.empty(N, device="cuda")
    ops.log_loss_rows(dev(t), dev(probs), out)
    pd = probs.astype(np.float64)
    want = (-(t * np.log(pd + 1e-7)) - (1 - t) * np.log(1 - pd + 1e-7)).sum(1)
    assert np.allclose(out.cpu().numpy(), want, rtol=2e-5, atol=1e-3)
    from multinn_amd.metrics import base_metrics
    loss = torch.rand(N, device="cuda")
    m, upd, _ = base_metrics(loss, dev(t), dev(p), out)
    assert abs(m["accuracy"] - (tb == pb).mean()) < 1e-12
    assert abs(m["precision"] - (tb & pb).sum() / max(1, pb.sum())) < 1e-12 and abs(m["recall"] - (tb & pb).sum() / max(1, tb.sum())) < 1e-12
    assert abs(float(m["batch/loss"]) - float(loss.mean())) < 1e-6 and abs(m["f1_score"] - m["precision"]) < 1e-12        # R5: f1 uses precision twice


def test_det_lstm_step_and_dense_bit_exact():
    """mnn_lstm_step_det / mnn_dense_det (csrc/det_step.hip; rnn.py:124, rnn_nade.py:54-57) against oracle/det_ref.c: every bit of c, h and of
    the Dense outputs -- u8 and f32 inputs, a second (feedback) input block, a zero state, row counts that are not a multiple of the
    rows per workgroup, unit counts of 32 .. 512, and several jobs in one launch."""
    from multinn_amd import ops
    rng = np.random.default_rng(77)
    jobs, refs = [], []
    B = 13
    # (the last two: K = 1112 and 1059 > 1024 -- two staging chunks, each quartered on its own; an odd K: a zero pad column)
    for (n_x, n_x2, u, u8, zero) in [(20, 0, 32, True, True), (440, 0, 512, True, False), (88, 128, 256, True, False), (96, 0, 96, False, False),
                                     (600, 0, 512, False, False), (900, 31, 128, True, False)]:
        W = (rng.standard_normal((n_x + n_x2 + u, 4 * u)) * 0.2).astype(np.float32)
        b = (rng.standard_normal(4 * u) * 0.1).astype(np.float32)
        x = (rng.random((B, n_x)) < 0.3).astype(np.uint8) if u8 else rng.standard_normal((B, n_x)).astype(np.float32)
        x2 = rng.standard_normal((B, n_x2)).astype(np.float32) if n_x2 else None
        c0 = None if zero else rng.standard_normal((B, u)).astype(np.float32)
        h0 = None if zero else np.tanh(rng.standard_normal((B, u))).astype(np.float32)
        xin = x.astype(np.float32) if x2 is None else np.concatenate([x.astype(np.float32), x2], 1)
        _, st = det.lstm_step(xin, None if zero else [(c0, h0)], [(W, b)])
        refs.append(st[0])
        if u == 256:                                       # one track of a [B, n_x, 3] step: element stride 3 (the feedback scan's sample views)
            x3 = torch.zeros((B, n_x, 3), dtype=torch.uint8 if u8 else torch.float32, device=DEV)
            x3[:, :, 1] = dev(x)
            xd = x3[:, :, 1]
        else:
            xd = torch.zeros((B, n_x + 3), dtype=torch.uint8 if u8 else torch.float32, device=DEV)    # a padded row pitch
            xd[:, :n_x] = dev(x)
        jobs.append(dict(x=xd, n_x=n_x, x2=None if x2 is None else dev(x2), h_prev=None if zero else dev(h0), c_prev=None if zero else dev(c0),
                         W=dev(W), bias=dev(b), c_out=torch.empty((B, u), device=DEV), h_out=torch.empty((B, u), device=DEV)))
    ops.lstm_step_det(jobs)                                            # six jobs of different widths: ONE launch
    for j, (c_ref, h_ref) in zip(jobs, refs):
        assert np.array_equal(j["c_out"].cpu().numpy(), c_ref) and np.array_equal(j["h_out"].cpu().numpy(), h_ref)
    # the same six steps from PACKED weights (mnn_det_lstm_pack: the numbers of W in the kernel's load order -- what mnn_generate_scan runs on):
    # the same bits, also with packed and in-place jobs mixed in one launch
    for mixed in (False, True):
        for i, j in enumerate(jobs):
            j["c_out"].fill_(-3.0); j["h_out"].fill_(-3.0)
            j.pop("Wp", None)
            if not (mixed and i % 2):
                j["Wp"] = ops.det_lstm_pack(j["W"], j["c_out"].shape[1])
        ops.lstm_step_det(jobs)
        for j, (c_ref, h_ref) in zip(jobs, refs):
            assert np.array_equal(j["c_out"].cpu().numpy(), c_ref) and np.array_equal(j["h_out"].cpu().numpy(), h_ref), (mixed, j["W"].shape)
    djobs, drefs = [], []
    for (K, N, with_bias) in [(256, 696, True), (32, 5, False), (512, 344, True), (1101, 40, True), (7, 33, False)]:
        x = rng.standard_normal((B, K)).astype(np.float32)
        W = (rng.standard_normal((K, N)) * 0.1).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32) if with_bias else None
        out = torch.full((B, N + 8), -7.0, device=DEV)
        djobs.append(dict(x=dev(x), W=dev(W), bias=None if b is None else dev(b), out=out[:, :N]))
        drefs.append((det.dense(x, W, b), out))
    ops.dense_det(djobs)
    for j, (ref, full) in zip(djobs, drefs):
        assert np.array_equal(j["out"].cpu().numpy(), ref)
        assert bool((full[:, ref.shape[1]:] == -7.0).all())            # nothing written past N
    for i, j in enumerate(djobs):                                      # ... and from packed weights (mnn_det_dense_pack), packed and in-place jobs mixed
        j["out"].fill_(-5.0)
        if i != 2:
            j["Wp"] = ops.det_dense_pack(j["W"])
    ops.dense_det(djobs)
    for j, (ref, full) in zip(djobs, drefs):
        assert np.array_equal(j["out"].cpu().numpy(), ref)
        assert bool((full[:, ref.shape[1]:] == -7.0).all())


def test_nade_sample_multi_equals_per_generator_launches():
    """mnn_nade_sample_multi: M single-NADE generators sampled in ONE launch, straight into the tracks of a [B, P, M] step, == M separate
    mnn_nade_sample launches (and therefore the deterministic checker, test_nade_sample_bit_exact)."""
    from multinn_amd import ops
    rng = np.random.default_rng(91)
    N, D, Hn, M = 9, 88, 256, 5
    step = torch.zeros((N, 3, D, M), dtype=torch.uint8, device=DEV)          # [B, steps, P, M]; sample into step 1
    jobs, refs = [], []
    for m in range(M):
        bias = dev((rng.standard_normal((N, Hn + D + 8)) * 0.5).astype(np.float32))
        we = dev((rng.standard_normal((D, Hn)) * 0.1).astype(np.float32)); wd = dev((rng.standard_normal((D, Hn)) * 0.1).astype(np.float32))
        nll = torch.zeros(N, device=DEV)
        jobs.append(dict(bias=bias, w_enc=we, w_dec=wd, seed=70 + m, samples=step[:, 1, :, m], nll=nll))
        ref = torch.zeros((N, D), dtype=torch.uint8, device=DEV); rn = torch.zeros((1, N), device=DEV)
        ops.nade_sample(bias, we, wd, 1, D, Hn, 1.0, 70 + m, 4, 6, ref, nll=rn)
        refs.append((ref, rn[0]))
    ops.nade_sample_multi(jobs, D, Hn, 1.0, 4, 6)
    for m, (ref, rn) in enumerate(refs):
        assert torch.equal(step[:, 1, :, m], ref) and torch.equal(jobs[m]["nll"], rn)
        assert 0 < float(ref.float().mean()) < 1
    assert not bool(step[:, 0].any()) and not bool(step[:, 2].any())


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("B,T,keep,layout,save", [(8, 6, 0.9, "plain", True), (64, 5, 0.9, "kblock", True), (36, 4, 1.0, "plain", True), (12, 7, 0.9, None, False),
                                                   (2048, 2, 0.9, "kblock", True)])
def test_lstm_resident_recurrence_vs_float64(ops, B, T, keep, layout, save, dt):
    """The CU-resident recurrence of a 256-unit layer (lstm_resident.hip: four rows per workgroup, the whole recurrent matrix on the CU) against
    a float64 restatement of rnn.py:104-145 on the SAME 16-bit operands (gate order i, g, f, o; the state it feeds back is the rounded h; the saved
    gates are the rounded activations): forward h / y / c / gates and both transposed copies, backward dz in all three layouts and the bias
    gradient.  B = 36 runs nine workgroups off the XCD-contiguous row mapping, B = 2048 twice as many workgroups as the device has CUs (no
    co-residency requirement: they run in rounds), save = False is the inference variant (nothing saved)."""
    u = 256
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    eps = 2.0 ** -10 if dt == "fp16" else 2.0 ** -7
    rng = np.random.default_rng(11)
    r16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt)            # noqa: E731
    wh_t = r16(rng.normal(0, 0.06, (4 * u, u)))                                     # [gate-interleaved row][k]
    xproj = r16(rng.normal(0, 1.2, (T, B, u, 4)))                                    # gate-minor
    mask = (rng.random((T, B, u)) < keep).astype(np.uint8) if keep < 1.0 else None
    N = T * B
    Np = N
    d = lambda t_: t_.to(DEV)                                                        # noqa: E731
    gates = torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt) if save else None
    c = torch.zeros((T, B, u), device=DEV)
    h = torch.zeros((T, B, u), device=DEV, dtype=tdt)
    y = torch.zeros((T, B, u), device=DEV, dtype=tdt) if mask is not None else None
    hT = torch.zeros((u, Np), device=DEV, dtype=tdt) if save else None
    yT = torch.zeros((u, Np), device=DEV, dtype=tdt) if save else None
    md = dev(mask) if mask is not None else None
    assert ops.lstm_resident_ok(B, u) and not ops.lstm_resident_ok(B + 1, u) and not ops.lstm_resident_ok(B, 512)
    L = ops.lstm2_fwd_layer(d(xproj).view(T, B, 4 * u), d(wh_t), None, None, gates, c, h, hT, y, md, yT=yT, gates_dtype=tdt, xproj_dtype=tdt)
    ops.lstm_resident_fwd(T, B, L, keep)
    torch.cuda.synchronize()
    # ---- float64 forward on the same operands ----
    W = wh_t.double().numpy()                                                        # z[n] += sum_k h[k] W[n][k]
    hk = h.double().cpu().numpy()
    # the 16-bit state the kernel feeds back
    ref = L64.forward(W, xproj.double().numpy(), lambda t, hv: hk[t] if (mask is None or t + 1 == T) else r16(hv).double().numpy())
    got_c = c.cpu().numpy()
    assert np.abs(got_c - ref["c"]).max() < 4 * eps, np.abs(got_c - ref["c"]).max()
    if mask is None:
        assert np.abs(h.double().cpu().numpy() - ref["h"]).max() < 2 * eps
        out16 = h
    else:
        assert np.abs(h[-1].double().cpu().numpy() - ref["h"][-1]).max() < 2 * eps          # only the final state leaves through h
        yref = r16(ref["h"]).double().numpy() / keep * mask
        assert np.abs(y.double().cpu().numpy() - yref).max() < 3 * eps
        out16 = y
    if save:
        assert np.abs(gates.double().cpu().numpy().reshape(T, B, u, 4) - ref["g"]).max() < 2 * eps
        # h^T[unit][(t + 1) B + row] = h[t] (column block 0 untouched: h_{-1}), y^T[unit][t B + row] = the layer's output
        assert torch.equal(yT.view(u, T, B), out16.permute(2, 0, 1))
        hh = r16(ref["h"]).double().numpy()
        assert np.abs(hT.view(u, T, B)[:, 1:].double().cpu().numpy() - np.transpose(hh, (2, 0, 1))[:, :-1]).max() < 2 * eps
        assert float(hT.view(u, T, B)[:, 0].abs().max()) == 0.0
    if not save:
        return
    # ---- backward on the kernel's own saved tensors ----
    dh = torch.from_numpy(rng.normal(0, 0.02, (T, B, u)).astype(np.float32)).to(DEV)
    wh_p = wh_t.t().contiguous().to(DEV)                                             # [k][gate-interleaved column]
    kb = layout == "kblock"
    dzc = torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt)
    dzT = torch.zeros((N // 32, 4 * u, 32), device=DEV, dtype=tdt) if kb else torch.zeros((4 * u, Np), device=DEV, dtype=tdt)
    db = torch.zeros(4 * u, device=DEV)
    E = ops.lstm2_bwd_layer(dh, wh_p, gates, c, None, dzc, ops.lstm_seq_bwd_workspace(B, u, DEV), dzT, db, md, gates_dtype=tdt)
    ops.lstm_resident_bwd(T, B, E, keep)
    torch.cuda.synchronize()
    Gs = gates.double().cpu().numpy().reshape(T, B, u, 4)
    Cs = c.double().cpu().numpy()
    dzk = dzc.double().cpu().numpy()
    dz_ref = L64.backward(W, Gs, Cs, dh.double().cpu().numpy(), mask, keep, lambda t, dz: dzk[t])      # the 16-bit values the kernel feeds back
    scale = np.abs(dz_ref).max()
    got = dzc.double().cpu().numpy()
    assert np.abs(got - dz_ref).max() < 3 * eps * scale, (np.abs(got - dz_ref).max(), scale)
    flat = dzc.view(N, 4 * u)
    if kb:
        assert torch.equal(dzT.permute(0, 2, 1).reshape(N, 4 * u), flat)
    else:
        assert torch.equal(dzT[:, :N].t(), flat)
    db_ref = flat.double().sum(0).cpu().numpy()
    assert np.abs(db.cpu().numpy() - db_ref).max() < 1e-5 * max(1.0, np.abs(db_ref).max()) + 1e-6


@pytest.mark.parametrize("N,D,tracks,rho,scale", [(512, 440, 1, 0.5, 1.0), (300, 84, 5, 0.5, 1.0), (256, 440, 1, 0.9, 1.0), (256, 440, 1, 0.5, 12.0), (130, 60, 1, 0.5, 60.0)])
def test_nade_dense_forward_multiplicative_states_vs_direct_form(ops, N, D, tracks, rho, scale):
    """The density-gated DENSE launch of the vector forward (`mnn_nade_logprob_fwd_gated`, gate word 1, Hn = 256) advances the hidden states
    multiplicatively -- u = exp(-a), one multiply by exp(-w_enc[i]) per flip, h = 1 / (1 + u), the exact `a` summed beside it -- against the
    direct sigmoid form of the same kernel: NLL, conditionals, d nll / d b_dec and the final pre-activation handed to the backward pass.
    scale > 1 multiplies the encoder weights and biases so that |a| runs past the guard's bound of 40 and back (scale 12) and past the f32
    range of exp (scale 60: u saturates, h is 0 / 1, every u is re-derived from its exact a): the guarded form stays with the direct one."""
    Hn = 256
    g = torch.Generator(device=DEV).manual_seed(11)
    v = (torch.rand((tracks, N, D), device=DEV, generator=g) < rho).to(torch.uint8)
    ld = (tracks * (Hn + D) + 63) // 64 * 64
    bias = (torch.randn((N, ld), device=DEV, generator=g) * 0.5)[:, :tracks * (Hn + D)]
    bias[:, :tracks * Hn] *= scale
    we = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1 * scale
    wd = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1
    rw = torch.rand(N, device=DEV, generator=g)

    def run(gate):
        nll = torch.zeros((tracks, N), device=DEV)
        cp = torch.zeros((tracks, N, D), device=DEV)
        db = torch.zeros((N, ld), device=DEV)[:, :tracks * (Hn + D)]
        af = torch.zeros((tracks, N, Hn), device=DEV)
        ops.nade_logprob_fwd(v, bias, we, wd, tracks, D, Hn, rw, nll, cp, db, af, gate=gate, run_if=1)
        return nll, cp, db[:, tracks * Hn:].clone(), af

    n0, c0, d0, a0 = run(None)                                                 # the direct form (ungated entry)
    n1, c1, d1, a1 = run(torch.tensor([1], device=DEV, dtype=torch.int32))     # gate word 1 = dense: the multiplicative form
    assert torch.equal(a1, a0)                                                 # `a` is the same exact sum in both
    ec, en = float((c1 - c0).abs().max()), float(((n1 - n0).abs() / n0.abs().clamp_min(1.0)).max())
    ed = float((d1 - d0).abs().max()) / max(float(d0.abs().max()), 1e-30)
    print(f"\n[dense forward, multiplicative vs direct, N={N} D={D} tracks={tracks} rho={rho} scale={scale}] conditionals {ec:.2e}  NLL {en:.2e}  d b_dec {ed:.2e}")
    assert ec < 2e-5 and en < 2e-5 and ed < 1e-4, (ec, en, ed)
    n2, c2, _, _ = run(torch.tensor([0], device=DEV, dtype=torch.int32))       # gate word 0: this launch leaves at once, nothing is written
    assert float(n2.abs().max()) == 0.0 and float(c2.abs().max()) == 0.0


@pytest.mark.parametrize("N,D,tracks,rho,scale", [(512, 440, 1, 0.5, 1.0), (320, 84, 5, 0.5, 1.0), (256, 200, 1, 0.9, 1.0), (256, 440, 1, 0.5, 12.0), (300, 60, 1, 0.5, 1.0)])
def test_nade_dense_backward_multiplicative_states_vs_direct_form(ops, N, D, tracks, rho, scale):
    """The reverse scan on a DENSE batch: when the forward's density-gated dense launch ran and none of its waves passed |a| = 40 (it leaves a
    zero in the `unsafe` counter), `mnn_nade_logprob_bwd(..., unsafe)` runs the instantiation that carries exp(-a) instead of a -- a flip is one
    multiply by exp(+w_enc[i]) and a reciprocal -- against the direct form (no counter) on the same inputs: d w_enc, d w_dec, d b_enc.  scale 12:
    the forward's guard trips, waves count themselves unsafe, the backward keeps its exact path (bit-identical to the direct form, summation
    order of the atomics aside); N = 300: a ragged last wave; a gated-out forward launch (gate word 0, sparse) counts itself: direct path."""
    Hn = 256
    g = torch.Generator(device=DEV).manual_seed(13)
    v = (torch.rand((tracks, N, D), device=DEV, generator=g) < rho).to(torch.uint8)
    ld = (tracks * (Hn + D) + 63) // 64 * 64
    bias = (torch.randn((N, ld), device=DEV, generator=g) * 0.5)[:, :tracks * (Hn + D)]
    bias[:, :tracks * Hn] *= scale
    we = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1 * scale
    wd = torch.randn((tracks, D, Hn), device=DEV, generator=g) * 0.1
    rw = torch.rand(N, device=DEV, generator=g)
    one = torch.tensor([1], device=DEV, dtype=torch.int32)
    d0 = torch.zeros((N, ld), device=DEV)[:, :tracks * (Hn + D)]
    af = torch.zeros((tracks, N, Hn), device=DEV)
    unsafe = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    ops.nade_logprob_fwd(v, bias, we, wd, tracks, D, Hn, rw, torch.zeros((tracks, N), device=DEV), None, d0, af, gate=one, run_if=1, unsafe=unsafe)
    assert (int(unsafe) == 0) == (scale == 1.0), int(unsafe)

    def run(word):
        dwe, dwd = torch.zeros_like(we), torch.zeros_like(wd)
        d1 = torch.zeros((N, ld), device=DEV)[:, :tracks * (Hn + D)]
        d1.copy_(d0)
        ops.nade_logprob_bwd(v, bias, we, wd, tracks, D, Hn, af, d1, dwe, dwd, unsafe=word)
        return dwe, dwd, d1[:, :tracks * Hn].clone()

    def rel(x, y):
        return float((x.double() - y.double()).abs().max() / y.double().abs().max().clamp_min(1e-30))

    e0, w0, b0 = run(None)
    e1, w1, b1 = run(unsafe)
    errs = (rel(e1, e0), rel(w1, w0), rel(b1, b0))
    print(f"\n[dense backward, multiplicative vs direct, N={N} D={D} tracks={tracks} rho={rho} scale={scale}] d w_enc {errs[0]:.2e}  d w_dec {errs[1]:.2e}  d b_enc {errs[2]:.2e}")
    assert errs[0] < 2e-5 and errs[1] < 2e-5 and errs[2] < 2e-5, errs
    if scale != 1.0:
        assert torch.equal(b1, b0)                       # unsafe rows: the exact path, bit for bit
    gated_out = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    zero = torch.tensor([0], device=DEV, dtype=torch.int32)
    ops.nade_logprob_fwd(v, bias, we, wd, tracks, D, Hn, None, torch.zeros((tracks, N), device=DEV), None, None, None, gate=zero, run_if=1,
                         unsafe=gated_out)
    assert int(gated_out) == 1                           # the dense launch did not run: nothing vouched for
    e2, w2, b2 = run(gated_out)
    assert torch.equal(b2, b0) and rel(w2, w0) < 1e-6


@pytest.mark.parametrize("u,njobs,B,T,keep", [(256, 5, 256, 6, 0.9), (256, 3, 64, 5, 1.0), (512, 5, 256, 6, 0.9), (512, 2, 512, 4, 1.0)])
def test_lstm_recurrence_multi_job_launch_equals_single_launches(ops, u, njobs, B, T, keep):
    """ONE launch for several independent layers (mnn_lstm_resident_*_multi, mnn_lstm_cluster_*_multi: the per-track generators of the jamming
    mode share the grid of the CU-resident / cluster recurrences) against one launch per layer on the same inputs: every output of the forward
    (h, y, c, gates, both transposed copies) and of the backward (dz row-major, K-blocked dz^T, bias gradient) bit for bit.  The 512-unit case
    with five jobs is 40 clusters = 320 workgroups: more than the device holds at once, the last eight clusters run in a second round."""
    tdt = torch.float16
    kind = "resident" if u == 256 else "cluster"
    assert (ops.lstm_resident_ok if u == 256 else ops.lstm_cluster_ok)(B, u)
    N = T * B
    g = torch.Generator(device=DEV).manual_seed(7)

    def job():
        j = dict(wh_t=(torch.randn((4 * u, u), device=DEV, generator=g) * 0.04).to(tdt), xproj=(torch.randn((T, B, 4 * u), device=DEV, generator=g) * 1.2).to(tdt),
                 mask=(torch.rand((T, B, u), device=DEV, generator=g) < keep).to(torch.uint8) if keep < 1.0 else None,
                 dh=torch.randn((T, B, u), device=DEV, generator=g) * 0.02)
        j["wh_p"] = j["wh_t"].t().contiguous()
        return j

    def outs():
        o = dict(gates=torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt), c=torch.zeros((T, B, u), device=DEV), h=torch.zeros((T, B, u), device=DEV, dtype=tdt),
                 y=torch.zeros((T, B, u), device=DEV, dtype=tdt) if keep < 1.0 else None, hT=torch.zeros((u, N), device=DEV, dtype=tdt),
                 yT=torch.zeros((u, N), device=DEV, dtype=tdt), dzc=torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt),
                 dzT=torch.zeros((N // 32, 4 * u, 32), device=DEV, dtype=tdt), db=torch.zeros(4 * u, device=DEV))
        o["ws"] = ops.lstm_rowpar_workspace(T, B, u, DEV) if kind == "cluster" else None
        return o

    def fdesc(j, o):
        return ops.lstm2_fwd_layer(j["xproj"], j["wh_t"], None, None, o["gates"], o["c"], o["h"], o["hT"], o["y"], j["mask"], yT=o["yT"], gates_dtype=tdt, xproj_dtype=tdt)

    def bdesc(j, o):
        return ops.lstm2_bwd_layer(j["dh"], j["wh_p"], o["gates"], o["c"], None, o["dzc"], ops.lstm_seq_bwd_workspace(B, u, DEV), o["dzT"], o["db"], j["mask"], gates_dtype=tdt)

    jobs = [job() for _ in range(njobs)]
    single, multi = [outs() for _ in jobs], [outs() for _ in jobs]
    for j, o in zip(jobs, single):
        if kind == "resident":
            ops.lstm_resident_fwd(T, B, fdesc(j, o), keep)
            ops.lstm_resident_bwd(T, B, bdesc(j, o), keep)
        else:
            ops.lstm_cluster_fwd(T, B, fdesc(j, o), keep, o["ws"])
            ops.lstm_cluster_bwd(T, B, bdesc(j, o), keep, o["ws"])
    wss = [o["ws"] for o in multi] if kind == "cluster" else None
    ops.lstm_recurrence_multi(kind + "_fwd", T, B, [fdesc(j, o) for j, o in zip(jobs, multi)], keep, wss)
    if kind == "cluster":
        assert ops.lstm_cluster_bwd_multi_ok(B, u, njobs)
    ops.lstm_recurrence_multi(kind + "_bwd", T, B, [bdesc(j, o) for j, o in zip(jobs, multi)], keep, wss)
    torch.cuda.synchronize()
    for o in single + multi:
        if o["ws"] is not None:
            ops.lstm_rowpar_check(o["ws"])
    for a, b in zip(single, multi):
        for k in ("gates", "c", "h", "y", "hT", "yT", "dzc", "dzT", "db"):
            if a[k] is not None:
                assert torch.equal(a[k], b[k]), k
    assert float(single[0]["dzc"].float().abs().max()) > 0 and not torch.equal(single[0]["h"], single[1]["h"])


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("B,T,keep,layout,save,nolocal", [(256, 5, 0.9, "kblock", True, False), (512, 4, 1.0, "plain", True, False), (256, 6, 0.9, None, False, False),
                                                           (256, 4, 0.9, "kblock", True, True)])
def test_lstm_cluster_recurrence_vs_float64(ops, monkeypatch, B, T, keep, layout, save, nolocal, dt):
    """The cluster form of the CU-resident recurrence (lstm_cluster.hip: eight CUs share 32 rows of a 512-unit layer, all weights in registers,
    h exchanged through the XCD's L2; backward: K split by column ownership + a reduce-scatter of 16-bit partial sums) against a float64
    restatement of rnn.py:104-145 on the SAME 16-bit operands: forward h / y / c / gates and both transposed copies, backward dz in all three
    layouts and the bias gradient.  nolocal = the write-through hand-off policy (one exchange slot per timestep in the forward)."""
    u = 512
    if nolocal:
        monkeypatch.setenv("MNN_PERSIST_NO_LOCAL", "1")
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    eps = 2.0 ** -10 if dt == "fp16" else 2.0 ** -7
    rng = np.random.default_rng(13)
    r16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt)            # noqa: E731
    wh_t = r16(rng.normal(0, 0.04, (4 * u, u)))                                     # [gate-interleaved row][k]
    xproj = r16(rng.normal(0, 1.2, (T, B, u, 4)))                                    # gate-minor
    mask = (rng.random((T, B, u)) < keep).astype(np.uint8) if keep < 1.0 else None
    N = T * B
    d = lambda t_: t_.to(DEV)                                                        # noqa: E731
    gates = torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt) if save else None
    c = torch.zeros((T, B, u), device=DEV)
    h = torch.zeros((T, B, u), device=DEV, dtype=tdt)
    y = torch.zeros((T, B, u), device=DEV, dtype=tdt) if mask is not None else None
    hT = torch.zeros((u, N), device=DEV, dtype=tdt) if save else None
    yT = torch.zeros((u, N), device=DEV, dtype=tdt) if save else None
    md = dev(mask) if mask is not None else None
    assert ops.lstm_cluster_ok(B, u) and not ops.lstm_cluster_ok(B + 32, u) and not ops.lstm_cluster_ok(B, 256)
    ws = ops.lstm_rowpar_workspace(T, B, u, DEV)
    L = ops.lstm2_fwd_layer(d(xproj).view(T, B, 4 * u), d(wh_t), None, None, gates, c, h, hT, y, md, yT=yT, gates_dtype=tdt, xproj_dtype=tdt)
    ops.lstm_cluster_fwd(T, B, L, keep, ws)
    torch.cuda.synchronize()
    ops.lstm_rowpar_check(ws)
    # ---- float64 forward on the same operands ----
    W = wh_t.double().numpy()                                                        # z[n] += sum_k h[k] W[n][k]
    hk = h.double().cpu().numpy()
    # the 16-bit state the kernel feeds back
    ref = L64.forward(W, xproj.double().numpy(), lambda t, hv: hk[t] if (mask is None or t + 1 == T) else r16(hv).double().numpy())
    got_c = c.cpu().numpy()
    assert np.abs(got_c - ref["c"]).max() < 4 * eps, np.abs(got_c - ref["c"]).max()
    if mask is None:
        assert np.abs(h.double().cpu().numpy() - ref["h"]).max() < 2 * eps
        out16 = h
    else:
        assert np.abs(h[-1].double().cpu().numpy() - ref["h"][-1]).max() < 2 * eps          # only the final state leaves through h
        yref = r16(ref["h"]).double().numpy() / keep * mask
        assert np.abs(y.double().cpu().numpy() - yref).max() < 3 * eps
        out16 = y
    if not save:
        return
    assert np.abs(gates.double().cpu().numpy().reshape(T, B, u, 4) - ref["g"]).max() < 2 * eps
    # h^T[unit][(t + 1) B + row] = h[t] (column block 0 untouched: h_{-1}), y^T[unit][t B + row] = the layer's output
    assert torch.equal(yT.view(u, T, B), out16.permute(2, 0, 1))
    hh = r16(ref["h"]).double().numpy()
    assert np.abs(hT.view(u, T, B)[:, 1:].double().cpu().numpy() - np.transpose(hh, (2, 0, 1))[:, :-1]).max() < 2 * eps
    assert float(hT.view(u, T, B)[:, 0].abs().max()) == 0.0
    # ---- backward on the kernel's own saved tensors ----
    dh = torch.from_numpy(rng.normal(0, 0.02, (T, B, u)).astype(np.float32)).to(DEV)
    wh_p = wh_t.t().contiguous().to(DEV)                                             # [k][gate-interleaved column]
    kb = layout == "kblock"
    dzc = torch.zeros((T, B, 4 * u), device=DEV, dtype=tdt)
    dzT = torch.zeros((N // 32, 4 * u, 32), device=DEV, dtype=tdt) if kb else torch.zeros((4 * u, N), device=DEV, dtype=tdt)
    db = torch.zeros(4 * u, device=DEV)
    E = ops.lstm2_bwd_layer(dh, wh_p, gates, c, None, dzc, ops.lstm_seq_bwd_workspace(B, u, DEV), dzT, db, md, gates_dtype=tdt)
    ops.lstm_cluster_bwd(T, B, E, keep, ws)
    torch.cuda.synchronize()
    ops.lstm_rowpar_check(ws)
    Gs = gates.double().cpu().numpy().reshape(T, B, u, 4)
    Cs = c.double().cpu().numpy()
    dzk = dzc.double().cpu().numpy()
    dz_ref = L64.backward(W, Gs, Cs, dh.double().cpu().numpy(), mask, keep, lambda t, dz: dzk[t])      # the 16-bit values the kernel feeds back
    scale = np.abs(dz_ref).max()
    got = dzc.double().cpu().numpy()
    assert np.abs(got - dz_ref).max() < 3 * eps * scale, (np.abs(got - dz_ref).max(), scale)
    flat = dzc.view(N, 4 * u)
    if kb:
        assert torch.equal(dzT.permute(0, 2, 1).reshape(N, 4 * u), flat)
    else:
        assert torch.equal(dzT[:, :N].t(), flat)
    db_ref = flat.double().sum(0).cpu().numpy()
    assert np.abs(db.cpu().numpy() - db_ref).max() < 1e-5 * max(1.0, np.abs(db_ref).max()) + 1e-6


def test_lstm_cluster_entry_points_refuse_what_they_do_not_cover(ops):
    """Error behaviour of the cluster entries through the C ABI (no launch): other widths, a batch off the 256-row grid of eight clusters, an f32
    input projection, saved gates without the transposed copies, a mask without keep_prob < 1, a backward window shorter than four steps."""
    from multinn_amd._lib import MnnError
    T, B, u = 4, 256, 512
    dt = torch.float16
    mk = lambda *s, d=dt: torch.zeros(s, device=DEV, dtype=d)      # noqa: E731
    ws = ops.lstm_rowpar_workspace(T, B, u, DEV)
    wh, c, h = mk(4 * u, u), mk(T, B, u, d=torch.float32), mk(T, B, u)
    ok = ops.lstm2_fwd_layer(mk(T, B, 4 * u), wh, None, None, None, c, h, None, gates_dtype=dt, xproj_dtype=dt)
    ops.lstm_cluster_fwd(T, B, ok, 1.0, ws)                            # the inference form is fine
    torch.cuda.synchronize()
    ops.lstm_rowpar_check(ws)
    f32x = ops.lstm2_fwd_layer(mk(T, B, 4 * u, d=torch.float32), wh, None, None, None, c, h, None, gates_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_cluster_fwd(T, B, f32x, 1.0, ws)
    gates_only = ops.lstm2_fwd_layer(mk(T, B, 4 * u), wh, None, None, mk(T, B, 4 * u), c, h, None, gates_dtype=dt, xproj_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_cluster_fwd(T, B, gates_only, 1.0, ws)
    masked = ops.lstm2_fwd_layer(mk(T, B, 4 * u), wh, None, None, None, c, h, None, mk(T, B, u), mk(T, B, u, d=torch.uint8), gates_dtype=dt, xproj_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_cluster_fwd(T, B, masked, 1.0, ws)
    B2 = 288                                                           # a multiple of 32 (row-parallel: fine) but not of 256
    assert not ops.lstm_cluster_ok(B2, u) and not ops.lstm_cluster_ok(B, 256) and not ops.lstm_cluster_ok(2048, u)
    c2, h2 = mk(T, B2, u, d=torch.float32), mk(T, B2, u)
    off = ops.lstm2_fwd_layer(mk(T, B2, 4 * u), wh, None, None, None, c2, h2, None, gates_dtype=dt, xproj_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_cluster_fwd(T, B2, off, 1.0, ops.lstm_rowpar_workspace(T, B2, u, DEV))
    T3 = 3
    c3 = mk(T3, B, u, d=torch.float32)
    e3 = ops.lstm2_bwd_layer(mk(T3, B, u, d=torch.float32), mk(u, 4 * u), mk(T3, B, 4 * u), c3, None, mk(T3, B, 4 * u), ops.lstm_seq_bwd_workspace(B, u, DEV),
                             mk(4 * u, T3 * B), mk(4 * u, d=torch.float32), None, gates_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_cluster_bwd(T3, B, e3, 1.0, ops.lstm_rowpar_workspace(T3, B, u, DEV))
    em = ops.lstm2_bwd_layer(mk(T, B, u, d=torch.float32), mk(u, 4 * u), mk(T, B, 4 * u), c, None, mk(T, B, 4 * u), ops.lstm_seq_bwd_workspace(B, u, DEV),
                             mk(4 * u, T * B), mk(4 * u, d=torch.float32), mk(T, B, u, d=torch.uint8), gates_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_cluster_bwd(T, B, em, 1.0, ws)                         # a mask with keep_prob = 1


def test_lstm_resident_entry_points_refuse_what_they_do_not_cover(ops):
    """Error behaviour of the CU-resident entries through the C ABI (no launch): other widths, a batch off the 4-row workgroups, an f32
    input projection, saved gates without the transposed copies (they leave together), a mask without keep_prob < 1."""
    from multinn_amd._lib import MnnError
    T, B, u = 3, 8, 256
    dt = torch.float16
    mk = lambda *s, d=dt: torch.zeros(s, device=DEV, dtype=d)      # noqa: E731
    wh, c, h = mk(4 * u, u), mk(T, B, u, d=torch.float32), mk(T, B, u)
    ok = ops.lstm2_fwd_layer(mk(T, B, 4 * u), wh, None, None, None, c, h, None, gates_dtype=dt, xproj_dtype=dt)
    ops.lstm_resident_fwd(T, B, ok, 1.0)                               # the inference form is fine
    f32x = ops.lstm2_fwd_layer(mk(T, B, 4 * u, d=torch.float32), wh, None, None, None, c, h, None, gates_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_resident_fwd(T, B, f32x, 1.0)
    gates_only = ops.lstm2_fwd_layer(mk(T, B, 4 * u), wh, None, None, mk(T, B, 4 * u), c, h, None, gates_dtype=dt, xproj_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_resident_fwd(T, B, gates_only, 1.0)
    masked = ops.lstm2_fwd_layer(mk(T, B, 4 * u), wh, None, None, None, c, h, None, mk(T, B, u), mk(T, B, u, d=torch.uint8), gates_dtype=dt, xproj_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_resident_fwd(T, B, masked, 1.0)
    u5 = 512
    wide = ops.lstm2_fwd_layer(mk(T, B, 4 * u5), mk(4 * u5, u5), None, None, None, mk(T, B, u5, d=torch.float32), mk(T, B, u5), None, gates_dtype=dt,
                               xproj_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_resident_fwd(T, B, wide, 1.0)
    odd = ops.lstm2_fwd_layer(mk(T, 6, 4 * u), wh, None, None, None, mk(T, 6, u, d=torch.float32), mk(T, 6, u), None, gates_dtype=dt, xproj_dtype=dt)
    with pytest.raises(MnnError):
        ops.lstm_resident_fwd(T, 6, odd, 1.0)
    torch.cuda.synchronize()


def test_clip_adam_skips_a_non_finite_step_and_the_step_counter_with_it(ops):
    """a gradient whose norm is not finite leaves theta, m, v AND the device step counter untouched (the Adam bias correction
    counts applied steps), and the skip is counted."""
    n = 4099
    R = np.random.default_rng(3)
    th, g = dev(R.standard_normal(n).astype(np.float32)), dev(R.standard_normal(n).astype(np.float32))
    m, v = dev(R.random(n).astype(np.float32)), dev(R.random(n).astype(np.float32))
    th0, m0, v0 = th.clone(), m.clone(), v.clone()
    sd = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    skipped = torch.zeros(1, device=DEV, dtype=torch.int32)
    gbad = g.clone()
    gbad[17] = float("inf")
    for bad in (gbad, torch.full_like(g, float("nan"))):
        ss = torch.zeros(1, device=DEV)
        ops.sumsq(bad, ss)
        ops.clip_adam_step(th, bad, m, v, ss, 5.0, 0.01, 0.9, 0.999, 1e-4, 0, step_dev=sd, skipped=skipped)
        ops.step_increment(sd, ss, 5.0)
    assert torch.equal(th, th0) and torch.equal(m, m0) and torch.equal(v, v0) and int(sd) == 7 and int(skipped) == 2
    ss = torch.zeros(1, device=DEV)
    ops.sumsq(g, ss)
    ops.clip_adam_step(th, g, m, v, ss, 5.0, 0.01, 0.9, 0.999, 1e-4, 0, step_dev=sd, skipped=skipped)
    ops.step_increment(sd, ss, 5.0)
    assert int(sd) == 8 and int(skipped) == 2 and not torch.equal(th, th0)
    ops.step_increment(sd)                      # without the norm: always advances
    assert int(sd) == 9
    # the dynamic part of the f16 loss scale rides on the same outcome: a skipped step halves m, `grow_after` applied steps in a row double it
    # back, never past 1; [m, 1 / m] stay exact powers of two
    dyn, good = torch.ones(2, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32)
    inf, fin = torch.full((1,), float("inf"), device=DEV), torch.ones(1, device=DEV)
    for _ in range(3):
        ops.step_increment(sd, inf, 5.0, dyn, good, 2)
    assert int(sd) == 9 and dyn.tolist() == [0.125, 8.0] and int(good) == 0
    ops.step_increment(sd, fin, 5.0, dyn, good, 2)
    assert int(sd) == 10 and dyn.tolist() == [0.125, 8.0] and int(good) == 1
    ops.step_increment(sd, fin, 5.0, dyn, good, 2)
    assert dyn.tolist() == [0.25, 4.0] and int(good) == 0
    ops.step_increment(sd, inf, 5.0, dyn, good, 2)
    assert dyn.tolist() == [0.125, 8.0]
    for _ in range(12):
        ops.step_increment(sd, fin, 5.0, dyn, good, 2)
    assert dyn.tolist() == [1.0, 1.0] and int(sd) == 23


@pytest.mark.parametrize("M,N,K,cdt,hb", [(1000, 696, 256, torch.float32, True), (512, 200, 64, torch.float16, True), (768, 2048, 448, torch.float16, True),
                                           (300, 128, 96, torch.bfloat16, False), (2048, 256, 704, torch.float32, True), (4096, 512, 1024, torch.float32, False)])
def test_gemm_tn_short_k_activation_shapes_vs_f32_product(ops, M, N, K, cdt, hb):
    """The step's short-K activation GEMM shapes (M not a multiple of the row tile, an N edge inside a wave tile, K = 64 .. 1024, f32 and 16-bit
    C, with and without bias) through mnn_gemm_tn's own dispatch against an f32 product of the same 16-bit operands; padding columns of C stay
    untouched.  (Round 5's "pair" kernel, which this test used to force on, left the library in round 6: profiles/tools/gemm_pair_kernel.hip.frag.)"""
    g = torch.Generator(device=DEV).manual_seed(1)
    for dt in (torch.float16, torch.bfloat16):
        if cdt != torch.float32 and cdt != dt:
            continue
        A = (torch.randn(M, K, device=DEV, generator=g) * 0.5).to(dt)
        Bm = (torch.randn(N, K, device=DEV, generator=g) * 0.5).to(dt)
        bias = torch.randn(N, device=DEV, generator=g) if hb else None
        ref = A.float() @ Bm.float().t() + (bias if hb else 0.0)
        ldc = (N + 63) // 64 * 64
        Cfull = torch.full((M, ldc), 7.0, device=DEV, dtype=cdt)
        ops.gemm_tn(A, Bm, Cfull[:, :N], bias=bias)
        tol = 2e-3 if cdt == torch.float32 else (0.25 if cdt == torch.bfloat16 else 0.03)
        assert float((Cfull[:, :N].float() - ref).abs().max()) < tol, dt
        assert bool((Cfull[:, N:] == 7.0).all()), dt


@pytest.mark.parametrize("M,N,K,dt,hb", [(8192, 2048, 448, torch.float16, True), (16384, 1024, 512, torch.bfloat16, True), (8192 + 128 * 5, 256, 448, torch.float16, False),
                                          (8192 * 3 + 128, 256, 512, torch.float16, True)])
def test_gemm_weight_resident_kernel_matches_the_product(ops, M, N, K, dt, hb, monkeypatch):
    """The weight-resident persistent form of the input projections (csrc/gemm_bres.hip: B in AGPR-pinned registers, the rows streamed through
    an 8-slot LDS ring, the epilogue's stores counted into the stream's vmcnt waits) against an f32 product of the same 16-bit operands and
    against the LDS-staged kernels (MNN_GEMM_BRES=0): both K, both flavours, row counts that leave the last slab short, padding untouched."""
    g = torch.Generator(device=DEV).manual_seed(2)
    A = (torch.randn(M, K, device=DEV, generator=g) * 0.5).to(dt)
    Bm = (torch.randn(N, K, device=DEV, generator=g) * 0.5).to(dt)
    bias = torch.randn(N, device=DEV, generator=g) if hb else None
    ref = A.float() @ Bm.float().t() + (bias if hb else 0.0)
    ldc = N + 64
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MNN_GEMM_BRES", mode)
        Cfull = torch.full((M, ldc), 7.0, device=DEV, dtype=dt)
        for _ in range(2):                                   # twice: the second launch finds the caches warm and other workgroup timings
            ops.gemm_tn(A, Bm, Cfull[:, :N], bias=bias)
        assert float((Cfull[:, :N].float() - ref).abs().max()) < (0.25 if dt == torch.bfloat16 else 0.03), mode
        assert bool((Cfull[:, N:] == 7.0).all()), mode
        outs[mode] = Cfull[:, :N].clone()
    assert float((outs["1"].float() - outs["0"].float()).abs().max()) <= (0.07 if dt == torch.bfloat16 else 0.01)
