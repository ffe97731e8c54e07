"""Torch-tensor front end of the C ABI (include/multinn_hip.h).

Every function validates shapes/dtypes/devices on the host (a mis-sized operand must never reach
a kernel), extracts raw device pointers and the current HIP stream, and calls the library.
There is no CPU path: tensors must be on a ROCm device.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import F32, BF16, U8, F16, GEMM_ACCUMULATE, GEMM_A_KBLOCK32


def call(name, *args):
    return _lib.call(name, *args)

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.uint8: U8, torch.float16: F16}
H16 = (torch.bfloat16, torch.float16)          # the two 16-bit operand flavours (precision "bf16" / "fp16")
DENSITY_SLOTS = 256                             # MNN_DENSITY_SLOTS: u32 partial counts of mnn_density_gate / the piano-roll pass


def dtype_code(t):
    return _DT[t.dtype if isinstance(t, torch.Tensor) else t]


def _stream():
    if not torch.cuda.is_available():
        raise _lib.MnnError("multinn_amd has no CPU path: no ROCm device is available")
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.MnnError("multinn_amd has no CPU path: tensor is on %s" % t.device)
    return C.c_void_p(t.data_ptr())


def _req(cond, msg):
    if not cond:
        raise ValueError(msg)


def _rowmajor(t, what):
    _req(t.dim() == 2 and t.stride(1) == 1, f"{what}: need a 2-D tensor with unit inner stride, got {tuple(t.shape)} {t.stride()}")


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------
def gemm_tn(A, B, C_out, bias=None, accumulate=False, split_k=1, a_kblock=False, m_rows=None, k_rows=None):
    """C[M,N] (+)= A[M,K] . B[N,K]^T (+bias).  A,B same dtype (f32/bf16/f16), K-contiguous views.  a_kblock: A is
    given K-blocked, a contiguous [K/32, rows >= M, 32] tensor (element (m, k) at [k // 32, m, k % 32]), 16-bit, K % 64 == 0.
    m_rows / k_rows (int32 device words, compacted ragged batches): how many rows of A / how much of K carry data -- a hint the large-tile
    kernels use to skip the padding (mnn_gemm_tn_rows); A / both operands must be zero behind the count.  Rows of C past the 256-row tile
    that holds m_rows may then be left unwritten; k_rows = 0 gives C (+)= bias (or zeros), like all-zero operands do."""
    _rowmajor(B, "gemm B"); _rowmajor(C_out, "gemm C")
    _req(A.dtype == B.dtype and A.dtype in (torch.float32,) + H16, "gemm: A/B must both be f32, bf16 or f16")
    if a_kblock:
        _req(A.dim() == 3 and A.is_contiguous() and A.shape[2] == 32 and A.dtype in H16, "gemm: a K-blocked A is a contiguous 16-bit [K/32, rows, 32]")
        K, M, lda = A.shape[0] * 32, C_out.shape[0], A.shape[1]
        _req(M <= lda and K % 64 == 0, "gemm: K-blocked A: rows >= M, K % 64 == 0")
    else:
        _rowmajor(A, "gemm A")
        M, K = A.shape
        lda = A.stride(0)
    N, K2 = B.shape
    _req(K == K2 and C_out.shape == (M, N), f"gemm: shape mismatch A{tuple(A.shape)} B{tuple(B.shape)} C{tuple(C_out.shape)}")
    _req(C_out.dtype in (torch.float32,) + H16, "gemm: C must be f32/bf16/f16")
    if bias is not None:
        _req(bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous(), "gemm: bias must be f32[N]")
    flags = (GEMM_ACCUMULATE if accumulate else 0) | (GEMM_A_KBLOCK32 if a_kblock else 0)
    if m_rows is not None or k_rows is not None:
        for t in (m_rows, k_rows):
            _req(t is None or (t.dtype == torch.int32 and t.numel() >= 1 and t.is_cuda), "gemm: m_rows / k_rows are int32 device words")
        call("mnn_gemm_tn_rows", _stream(), dtype_code(A), M, N, K, _ptr(A), lda, _ptr(B), B.stride(0), _ptr(C_out), C_out.stride(0),
             dtype_code(C_out), _ptr(bias), flags, split_k, _ptr(m_rows), _ptr(k_rows))
        return C_out
    call("mnn_gemm_tn", _stream(), dtype_code(A), M, N, K, _ptr(A), lda, _ptr(B), B.stride(0), _ptr(C_out), C_out.stride(0),
         dtype_code(C_out), _ptr(bias), flags, split_k)
    return C_out


def transpose(src, out):
    """out[C,R] = src[R,C]^T with conversion."""
    _rowmajor(src, "transpose src"); _rowmajor(out, "transpose out")
    R, Cc = src.shape
    _req(out.shape[0] == Cc and out.shape[1] >= R, "transpose: out must be [C, >=R]")
    call("mnn_transpose", _stream(), _ptr(src), dtype_code(src), R, Cc, src.stride(0), _ptr(out), dtype_code(out), out.stride(0))
    return out


def convert2d(src, dst):
    _rowmajor(src, "convert src"); _rowmajor(dst, "convert dst")
    _req(src.shape == dst.shape, "convert2d: shape mismatch")
    call("mnn_convert2d", _stream(), _ptr(src), dtype_code(src), src.stride(0), _ptr(dst), dtype_code(dst), dst.stride(0), src.shape[0], src.shape[1])
    return dst


def ragged_index(lengths, B, T, n_total_dev=None, scale_rows=0.0):
    """Compaction index of a ragged window, built on the device (mnn_ragged_index): returns (idx, inv, hdr) -- idx[k] = time-major row at compact
    position k (valid rows first, time-major order kept), inv = its inverse, hdr int32 [4] = [n_valid | 1 / n_total | loss scale | 1 / loss scale]
    (words 1..3 are f32 bits: hdr.view(torch.float32)).  n_total_dev: f32 [1] valid rows of ALL ranks (None: this rank's)."""
    _req(lengths.dtype == torch.int32 and lengths.numel() == B and lengths.is_cuda and lengths.is_contiguous(), "ragged_index: lengths int32 [B] on the device")
    _req(n_total_dev is None or (n_total_dev.dtype == torch.float32 and n_total_dev.numel() == 1), "ragged_index: n_total_dev f32 [1]")
    dev = lengths.device
    idx = torch.empty(B * T, device=dev, dtype=torch.int32)
    inv = torch.empty(B * T, device=dev, dtype=torch.int32)
    hdr = torch.empty(4, device=dev, dtype=torch.int32)
    call("mnn_ragged_index", _stream(), _ptr(lengths), int(B), int(T), _ptr(n_total_dev), float(scale_rows), _ptr(idx), _ptr(inv), _ptr(hdr))
    return idx, inv, hdr


def rows_gather16(src, idx, hdr, dst, dst_t=None):
    """dst[k] = src[idx[k]] for k < hdr[0], zeros behind (16-bit [N, C] rows); dst_t [C, >= N] (optional): the transposed copy."""
    N, Cc = src.shape
    _req(src.dtype in H16 and dst.dtype == src.dtype and dst.shape == src.shape and src.stride(1) == 1 and dst.stride(1) == 1, "rows_gather16: 16-bit [N, C]")
    _req(dst_t is None or (dst_t.dtype == src.dtype and dst_t.shape[0] == Cc and dst_t.shape[1] >= N and dst_t.stride(1) == 1), "rows_gather16: dst_t [C, >= N]")
    call("mnn_rows_gather16", _stream(), _ptr(src), src.stride(0), _ptr(idx), _ptr(hdr), N, Cc, _ptr(dst), dst.stride(0), _ptr(dst_t),
         dst_t.stride(0) if dst_t is not None else 0)
    return dst


def rows_scatter_f32(src, inv, hdr, dst):
    """dst[row] = src[inv[row]] where inv[row] < hdr[0], zeros elsewhere (f32 [N, C], both contiguous)."""
    _req(src.dtype == torch.float32 and dst.dtype == torch.float32 and src.shape == dst.shape and src.is_contiguous() and dst.is_contiguous(),
         "rows_scatter_f32: contiguous f32 [N, C]")
    call("mnn_rows_scatter_f32", _stream(), _ptr(src), _ptr(inv), _ptr(hdr), src.shape[0], src.shape[1], _ptr(dst))
    return dst


def pianoroll_shift_timemajor(x, lengths, inputs, targets, row_weight, n_valid_total=0, inputs_t=None, count=None, compact=None):
    """x u8 [B,T,D] -> inputs [T,B,ld] (shifted, zero first step), targets u8 [T,B,D], row_weight f32 [T*B];
    inputs_t (bf16 [ld, >= T*B], optional): the transposed copy of inputs, written by the same pass.
    compact = (inv, hdr) of ragged_index (tiled 16-bit pass only): targets and row_weight are written in COMPACT row order, the weights from the
    device-side header (no host-side row count)."""
    _req(x.dtype == torch.uint8 and x.dim() == 3 and x.is_contiguous(), "pianoroll: x must be contiguous u8 [B,T,D]")
    B, T, D = x.shape
    _req(inputs.dim() == 3 and inputs.shape[0] == T and inputs.shape[1] == B and inputs.shape[2] >= D and inputs.is_contiguous(),
         "pianoroll: inputs must be contiguous [T,B,>=D]")
    if targets is not None:
        _req(targets.dtype == torch.uint8 and targets.shape == (T, B, D) and targets.is_contiguous(), "pianoroll: targets u8 [T,B,D]")
    if row_weight is not None:
        _req(row_weight.dtype == torch.float32 and row_weight.numel() == T * B, "pianoroll: row_weight f32 [T*B]")
    _req(compact is None or inputs_t is not None, "pianoroll: compact row order needs the tiled 16-bit pass (inputs_t)")
    if lengths is not None:
        _req(lengths.dtype == torch.int32 and lengths.numel() == B, "pianoroll: lengths int32 [B]")
        _req(n_valid_total > 0 or compact is not None, "pianoroll: n_valid_total required with lengths")
    if inputs_t is not None:
        _req(inputs.dtype in H16 and inputs_t.dtype == inputs.dtype and inputs_t.dim() == 2 and inputs_t.stride(1) == 1
             and inputs_t.shape[0] == inputs.shape[2] and inputs_t.shape[1] >= T * B, "pianoroll: inputs_t must be 16-bit [ld, >=T*B] like inputs")
        call("mnn_pianoroll_shift_timemajor_t", _stream(), _ptr(x), B, T, D, _ptr(lengths), _ptr(inputs), inputs.shape[2], _ptr(inputs_t),
             inputs_t.stride(0), _ptr(targets), _ptr(row_weight), int(n_valid_total), dtype_code(inputs), _ptr(count),
             _ptr(compact[0]) if compact is not None else None, _ptr(compact[1]) if compact is not None else None)
        return count is not None                    # True: `count` now holds the number of set target cells
    call("mnn_pianoroll_shift_timemajor", _stream(), _ptr(x), B, T, D, _ptr(lengths), _ptr(inputs), dtype_code(inputs), inputs.shape[2],
         _ptr(targets), _ptr(row_weight), int(n_valid_total))
    return False


def pianoroll_split_tracks(x, out):
    _req(x.dtype == torch.uint8 and x.dim() == 4 and x.is_contiguous(), "split_tracks: x must be contiguous u8 [B,T,P,M]")
    B, T, P, M = x.shape
    _req(out.dtype == torch.uint8 and out.shape == (M, T, B, P) and out.is_contiguous(), "split_tracks: out u8 [M,T,B,P]")
    call("mnn_pianoroll_split_tracks", _stream(), _ptr(x), B, T, P, M, _ptr(out))
    return out


def window_gather(X, ids, j, Tw, out, lengths=None, out_len=None, track=None, tracks=1):
    """out[b, t, :] = X[ids[b], j + t, :] (mnn_window_gather): X u8 [S, T, D] on the device, ids int32 [B] on the device, out u8 [B, Tw, D].
    track = m with tracks = M: feature p * M + m of every p instead, out u8 [B, Tw, D / M].  lengths int32 [S] with out_len int32 [B]:
    out_len[b] = clamp(lengths[ids[b]] - j, 0, Tw)."""
    _req(X.dtype == torch.uint8 and X.dim() == 3 and X.is_contiguous(), "window_gather: X must be contiguous u8 [S,T,D]")
    S, T, D = X.shape
    _req(ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous() and ids.numel() > 0, "window_gather: ids int32 [B]")
    B = ids.numel()
    if track is None:
        e0, es, Dout = 0, 1, D
    else:
        _req(tracks >= 1 and D % tracks == 0 and 0 <= track < tracks, f"window_gather: track {track} of {tracks} tracks over D = {D}")
        e0, es, Dout = int(track), int(tracks), D // tracks
    _req(out.dtype == torch.uint8 and tuple(out.shape) == (B, Tw, Dout) and out.is_contiguous(), f"window_gather: out must be contiguous u8 [{B},{Tw},{Dout}]")
    _req(lengths is None or (lengths.dtype == torch.int32 and lengths.numel() == S and lengths.is_contiguous()), "window_gather: lengths int32 [S]")
    _req(out_len is None or (lengths is not None and out_len.dtype == torch.int32 and out_len.numel() == B and out_len.is_contiguous()),
         "window_gather: out_len int32 [B], with lengths")
    call("mnn_window_gather", _stream(), _ptr(X), S, T, D, _ptr(ids), B, int(j), int(Tw), e0, es, Dout, _ptr(lengths), _ptr(out), _ptr(out_len))
    return out


def _moving_mask(moving, tracks, D, what):
    _req(isinstance(tracks, int) and 1 <= tracks <= 32 and D % tracks == 0, f"{what}: tracks = {tracks} must lie in 1..32 and divide D = {D}")
    _req(isinstance(moving, int) and not isinstance(moving, bool) and 0 <= moving < (1 << tracks), f"{what}: moving must be a bit mask over {tracks} tracks, got {moving!r}")
    return moving


def window_gather_shift(X, ids, j, Tw, out, shifts, tracks, moving, lengths=None, out_len=None, track=None):
    """window_gather with a pitch shift per output row (mnn_window_gather_shift): X u8 [S, T, P * tracks], shifts int32 [B] on X's device,
    moving a bit mask (bit m: track m is transposed).  An element of a moving track reads pitch p - shifts[b] of its track, 0 where that
    leaves 0..P-1; the other tracks are the plain gather's.  track = m: that track alone, out u8 [B, Tw, P]."""
    _req(X.dtype == torch.uint8 and X.dim() == 3 and X.is_contiguous(), "window_gather_shift: X must be contiguous u8 [S,T,D]")
    S, T, D = X.shape
    _req(ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous() and ids.numel() > 0, "window_gather_shift: ids int32 [B]")
    B = ids.numel()
    moving = _moving_mask(moving, tracks, D, "window_gather_shift")
    _req(isinstance(shifts, torch.Tensor) and shifts.dtype == torch.int32 and tuple(shifts.shape) == (B,) and shifts.is_contiguous()
         and shifts.device == X.device, f"window_gather_shift: shifts must be contiguous int32 [{B}] on {X.device}")
    if track is None:
        e0, es, Dout = 0, 1, D
    else:
        _req(0 <= track < tracks, f"window_gather_shift: track {track} of {tracks} tracks over D = {D}")
        e0, es, Dout = int(track), int(tracks), D // tracks
    _req(out.dtype == torch.uint8 and tuple(out.shape) == (B, Tw, Dout) and out.is_contiguous(), f"window_gather_shift: out must be contiguous u8 [{B},{Tw},{Dout}]")
    _req(lengths is None or (lengths.dtype == torch.int32 and lengths.numel() == S and lengths.is_contiguous()), "window_gather_shift: lengths int32 [S]")
    _req(out_len is None or (lengths is not None and out_len.dtype == torch.int32 and out_len.numel() == B and out_len.is_contiguous()),
         "window_gather_shift: out_len int32 [B], with lengths")
    call("mnn_window_gather_shift", _stream(), _ptr(X), S, T, D, _ptr(ids), B, int(j), int(Tw), e0, es, Dout, _ptr(lengths), _ptr(out), _ptr(out_len),
         _ptr(shifts), tracks, moving)
    return out


def pitch_extent(X, tracks, moving, lengths=None):
    """(lo, hi) int32 [S] on X's device (mnn_pitch_extent): per song of X u8 [S, T, P * tracks] the smallest and largest pitch at which a moving
    track (bit mask `moving`) has a non-zero cell in a step t < lengths[song] (every step without lengths); (P, -1) for a song with none."""
    _req(X.dtype == torch.uint8 and X.dim() == 3 and X.is_contiguous(), "pitch_extent: X must be contiguous u8 [S,T,D]")
    S, T, D = X.shape
    moving = _moving_mask(moving, tracks, D, "pitch_extent")
    _req(lengths is None or (lengths.dtype == torch.int32 and lengths.numel() == S and lengths.is_contiguous() and lengths.device == X.device),
         "pitch_extent: lengths int32 [S] on X's device")
    lo = torch.empty(S, dtype=torch.int32, device=X.device)
    hi = torch.empty(S, dtype=torch.int32, device=X.device)
    call("mnn_pitch_extent", _stream(), _ptr(X), S, T, D, tracks, moving, _ptr(lengths), _ptr(lo), _ptr(hi))
    return lo, hi


# ------------------------------------------------------------------------------------------------
def lstm_pack_weights(W, b, n_in, units, wx_t, wh_t, wh_p, wx_p, bias_p):
    _req(W.dtype == torch.float32 and W.shape == (n_in + units, 4 * units) and W.is_contiguous(), "pack: W f32 [(in+u),4u]")
    _req(b.dtype == torch.float32 and b.numel() == 4 * units, "pack: b f32 [4u]")
    ld_in = wx_t.shape[1]
    _req(wx_t.shape == (4 * units, ld_in) and ld_in >= n_in and wx_t.is_contiguous(), "pack: wx_t [4u, ld_in]")
    _req(wh_t.shape == (4 * units, units) and wh_t.is_contiguous(), "pack: wh_t [4u,u]")
    _req(wh_p.shape == (units, 4 * units) and wh_p.is_contiguous(), "pack: wh_p [u,4u]")
    if wx_p is not None:
        _req(wx_p.shape == (n_in, 4 * units) and wx_p.is_contiguous() and wx_p.dtype == wx_t.dtype, "pack: wx_p [in,4u]")
    _req(wx_t.dtype == wh_t.dtype == wh_p.dtype, "pack: dtype mismatch")
    _req(bias_p.dtype == torch.float32 and bias_p.numel() == 4 * units, "pack: bias_p f32 [4u]")
    call("mnn_lstm_pack_weights", _stream(), _ptr(W), _ptr(b), n_in, units, dtype_code(wx_t), ld_in, _ptr(wx_t), _ptr(wh_t), _ptr(wh_p),
         _ptr(wx_p), _ptr(bias_p))


def lstm_rows_gate_minor(wx_t, bias_p, wx_gm, bias_gm):
    """Gate-minor (row unit*4+g) copy of a packed wx_t [4u, ld] and its bias: the layout the persistent recurrence reads xproj in."""
    N4, ld = wx_t.shape
    _req(N4 % 128 == 0 and wx_t.is_contiguous() and wx_gm.shape == wx_t.shape and wx_gm.dtype == wx_t.dtype and wx_gm.is_contiguous(),
         "rows_gate_minor: wx_t / wx_gm [4u, ld]")
    _req(bias_p.dtype == torch.float32 and bias_gm.dtype == torch.float32 and bias_p.numel() == N4 and bias_gm.numel() == N4, "rows_gate_minor: bias f32 [4u]")
    call("mnn_lstm_rows_gate_minor", _stream(), dtype_code(wx_t), N4 // 4, ld, _ptr(wx_t), _ptr(bias_p), _ptr(wx_gm), _ptr(bias_gm))


def lstm_unpack_grads(dwx_t, dwh_t, db_p, n_in, units, dW, db, consume=False):
    """consume=True: the packed sources are zeroed as they are read (persistent accumulators, see mnn_lstm_unpack_grads_consume)."""
    ld_in = dwx_t.shape[1]
    _req(dwx_t.dtype == torch.float32 and dwx_t.shape == (4 * units, ld_in) and dwx_t.is_contiguous(), "unpack: dwx_t f32 [4u,ld]")
    _req(dwh_t.dtype == torch.float32 and dwh_t.shape == (4 * units, units) and dwh_t.is_contiguous(), "unpack: dwh_t f32 [4u,u]")
    _req(dW.dtype == torch.float32 and dW.shape == (n_in + units, 4 * units) and dW.is_contiguous(), "unpack: dW f32 [(in+u),4u]")
    _req(db.numel() == 4 * units and db_p.numel() == 4 * units, "unpack: bias sizes")
    call("mnn_lstm_unpack_grads_consume" if consume else "mnn_lstm_unpack_grads", _stream(), _ptr(dwx_t), _ptr(dwh_t), _ptr(db_p), n_in, units, ld_in,
         _ptr(dW), _ptr(db))


def lstm_unpack_grads_cat(dw_cat, db_p, n_in, units, ld_in, dW, db):
    """dw_cat f32 [4u, ld_in + u] = [dWx^T | dWh^T] (one GEMM over the concatenated operand) -> dW [(in+u), 4u], db [4u], accumulating; the
    packed sources are zeroed as they are read."""
    _req(dw_cat.dtype == torch.float32 and dw_cat.shape == (4 * units, ld_in + units) and dw_cat.is_contiguous(), "unpack_cat: dw_cat f32 [4u, ld+u]")
    _req(dW.dtype == torch.float32 and dW.shape == (n_in + units, 4 * units) and dW.is_contiguous(), "unpack_cat: dW f32 [(in+u),4u]")
    _req(db.numel() == 4 * units and db_p.numel() == 4 * units and db_p.dtype == torch.float32, "unpack_cat: bias sizes")
    call("mnn_lstm_unpack_grads_cat", _stream(), _ptr(dw_cat), _ptr(db_p), n_in, units, ld_in, _ptr(dW), _ptr(db))


def lstm_fused_outputs(dtype, units):
    return bool(_lib.load().mnn_lstm_fused_outputs(dtype_code(dtype), int(units)))


def lstm_seq_fwd(xproj, wh_t, h0, c0, gates, c, h, t_begin=0, t_end=None, hT=None):
    T, B, N4 = xproj.shape
    units = N4 // 4
    _req(xproj.dtype == torch.float32 and xproj.is_contiguous() and units % 32 == 0, "lstm_fwd: xproj f32 [T,B,4u], u%32==0")
    _req(wh_t.shape == (N4, units) and wh_t.is_contiguous() and wh_t.dtype == h.dtype, "lstm_fwd: wh_t [4u,u] in the compute dtype")
    _req(c.dtype == torch.float32 and c.shape == (T, B, units) and c.is_contiguous(), "lstm_fwd: c f32 [T,B,u]")
    _req(h.shape == (T, B, units) and h.is_contiguous(), "lstm_fwd: h [T,B,u]")
    if gates is not None:
        _req(gates.dtype == torch.float32 and gates.shape == (T, B, N4) and gates.is_contiguous(), "lstm_fwd: gates f32 [T,B,4u]")
    if h0 is not None:
        _req(h0.shape == (B, units) and h0.dtype == h.dtype and h0.is_contiguous(), "lstm_fwd: h0")
    if c0 is not None:
        _req(c0.shape == (B, units) and c0.dtype == torch.float32 and c0.is_contiguous(), "lstm_fwd: c0")
    t_end = T if t_end is None else t_end
    _req(0 <= t_begin < t_end <= T, "lstm_fwd: bad step range")
    if hT is not None:
        _req(hT.dim() == 2 and hT.shape[0] == units and hT.stride(1) == 1 and hT.shape[1] >= T * B and hT.dtype == h.dtype, "lstm_fwd: hT [u, >=T*B]")
    call("mnn_lstm_seq_fwd", _stream(), dtype_code(h), T, B, units, int(t_begin), int(t_end), _ptr(xproj), _ptr(wh_t), _ptr(h0), _ptr(c0),
         _ptr(gates), _ptr(c), _ptr(h), _ptr(hT), hT.stride(0) if hT is not None else 0)


def lstm_seq_bwd_workspace(B, units, device):
    return torch.empty(_lib.load().mnn_lstm_seq_bwd_workspace_bytes(B, units), dtype=torch.uint8, device=device)


def lstm_seq_bwd(dh_ext, wh_p, gates, c, c0, dz, dz_T, dh0=None, dc0=None, t_begin=0, t_end=None, ws=None, dzT_t=None, db_p=None):
    T, B, units = dh_ext.shape
    N4 = 4 * units
    _req(dh_ext.dtype == torch.float32 and dh_ext.is_contiguous(), "lstm_bwd: dh_ext f32 [T,B,u]")
    _req(wh_p.shape == (units, N4) and wh_p.is_contiguous(), "lstm_bwd: wh_p [u,4u]")
    _req(gates.shape == (T, B, N4) and gates.dtype == torch.float32 and gates.is_contiguous(), "lstm_bwd: gates")
    _req(c.shape == (T, B, units) and c.dtype == torch.float32 and c.is_contiguous(), "lstm_bwd: c")
    if dz is not None:
        _req(dz.shape == (T, B, N4) and dz.dtype == torch.float32 and dz.is_contiguous(), "lstm_bwd: dz f32 [T,B,4u]")
    if dz_T is not None:
        _req(dz_T.shape == (T, B, N4) and dz_T.dtype == wh_p.dtype and dz_T.is_contiguous(), "lstm_bwd: dz_T")
    t_end = T if t_end is None else t_end
    _req(0 <= t_begin < t_end <= T, "lstm_bwd: bad step range")
    if ws is None:
        _req(t_begin == 0 and t_end == T, "lstm_bwd: chunked calls must share a workspace (lstm_seq_bwd_workspace)")
        ws = lstm_seq_bwd_workspace(B, units, dh_ext.device)
    if dzT_t is not None:
        _req(dzT_t.dim() == 2 and dzT_t.shape[0] == N4 and dzT_t.stride(1) == 1 and dzT_t.shape[1] >= T * B and dzT_t.dtype == wh_p.dtype,
             "lstm_bwd: dzT_t [4u, >=T*B]")
    if db_p is not None:
        _req(db_p.dtype == torch.float32 and db_p.numel() == N4 and db_p.is_contiguous(), "lstm_bwd: db_p f32 [4u]")
    call("mnn_lstm_seq_bwd", _stream(), dtype_code(wh_p), T, B, units, int(t_begin), int(t_end), _ptr(dh_ext), _ptr(wh_p), _ptr(gates),
         _ptr(c), _ptr(c0), _ptr(dz), _ptr(dz_T), _ptr(dh0), _ptr(dc0), _ptr(ws), _ptr(dzT_t), dzT_t.stride(0) if dzT_t is not None else 0,
         _ptr(db_p))


def _step_ok(step_dev):
    _req(step_dev is None or (step_dev.dtype == torch.int32 and step_dev.numel() == 1), "step_dev must be a device int32 scalar")


def _p0(t):
    return t.data_ptr() if t is not None else None


def lstm2_fwd_layer(xproj, wh_t, h0, c0, gates, c, h, hT, y=None, mask=None, wx_t=None, bias_p=None, yT=None, gates_dtype=torch.float32,
                    xproj_dtype=torch.float32):
    """Descriptor of one layer for lstm2_seq_fwd (same tensors as lstm_seq_fwd; bf16, contiguous, time-major).
    y/mask: dropped output and u8 keep mask (keep_prob < 1); wx_t/bias_p: this layer's input projection (layer 2)."""
    _req(h.dim() == 3 and h.dtype in H16 and h.is_contiguous(), "lstm2: h bf16 / f16 [T,B,u]")
    dt = h.dtype                                    # the layer's 16-bit flavour: every 16-bit tensor of the layer has it
    T, B, u = h.shape
    N4 = 4 * u
    _req(xproj is not None or wx_t is not None, "lstm2: xproj may be omitted only for a layer with its own input projection (persistent form)")
    _req(xproj is None or (xproj.dtype == xproj_dtype and xproj.is_contiguous() and xproj.shape == (T, B, N4)), "lstm2: xproj [T,B,4u] of the stated dtype")
    _req(xproj_dtype in (torch.float32, dt), "lstm2: xproj f32 (or the layer's 16-bit type: row-parallel form only)")
    _req(gates_dtype in (torch.float32, dt), "lstm2: gates f32 (or the layer's 16-bit type: row-parallel form)")
    _req(wh_t.shape == (N4, u) and wh_t.is_contiguous() and wh_t.dtype == dt, "lstm2: wh_t [4u,u] in the layer's 16-bit type")
    _req(c.dtype == torch.float32 and c.shape == (T, B, u) and c.is_contiguous(), "lstm2: c")
    _req(gates is None or (gates.dtype == gates_dtype and gates.shape == (T, B, N4) and gates.is_contiguous()), "lstm2: gates")
    _req(h0 is None or (h0.shape == (B, u) and h0.dtype == dt and h0.is_contiguous()), "lstm2: h0")
    _req(c0 is None or (c0.shape == (B, u) and c0.dtype == torch.float32 and c0.is_contiguous()), "lstm2: c0")
    _req(hT is None or (hT.dim() == 2 and hT.shape[0] == u and hT.stride(1) == 1 and hT.shape[1] >= T * B and hT.dtype == dt), "lstm2: hT")
    _req((y is None) == (mask is None), "lstm2: y and mask come together")
    if mask is not None:
        _req(mask.dtype == torch.uint8 and mask.shape == (T, B, u) and mask.is_contiguous(), "lstm2: mask u8 [T,B,u]")
        _req(y.dtype == dt and y.shape == (T, B, u) and y.is_contiguous(), "lstm2: y [T,B,u] in the layer's 16-bit type")
    ld_w = 0
    if wx_t is not None:
        _req(wx_t.dim() == 2 and wx_t.shape[0] == N4 and wx_t.stride(1) == 1 and wx_t.dtype == dt, "lstm2: wx_t [4u, ld] in the layer's 16-bit type")
        _req(bias_p is not None and bias_p.dtype == torch.float32 and bias_p.numel() == N4, "lstm2: bias_p f32 [4u]")
        ld_w = wx_t.stride(0)
    for t in (wh_t, c, h):
        _ptr(t)
    _req(yT is None or (yT.dim() == 2 and yT.shape[0] == u and yT.stride(1) == 1 and yT.shape[1] >= T * B and yT.dtype == dt), "lstm2: yT")
    return _lib.LstmFwdLayer(u, _p0(xproj), _p0(wh_t), _p0(h0), _p0(c0), _p0(gates), _p0(c), _p0(h), _p0(hT), hT.stride(0) if hT is not None else 0,
                             _p0(y), _p0(mask), _p0(wx_t), ld_w, _p0(bias_p), _p0(yT), yT.stride(0) if yT is not None else 0,
                             1 if xproj_dtype != torch.float32 else 0, 1 if dt == torch.float16 else 0)


def lstm2_seq_fwd(T, B, L1, L2, keep_prob, s_begin=0, s_end=None):
    s_end = T + 2 if s_end is None else s_end
    _req(0 <= s_begin < s_end <= T + 2, "lstm2_fwd: bad launch range")
    call("mnn_lstm2_seq_fwd", _stream(), T, B, C.byref(L1), C.byref(L2), float(keep_prob), int(s_begin), int(s_end))


def lstm2_bwd_layer(dh_ext, wh_p, gates, c, c0, dz_T, ws, dzT_t, db_p, mask=None, wx_p=None, gates_dtype=torch.float32):
    T, B, u = c.shape
    N4 = 4 * u
    _req(dh_ext is None or (dh_ext.dtype == torch.float32 and dh_ext.is_contiguous() and dh_ext.shape == (T, B, u)), "lstm2 bwd: dh_ext f32 [T,B,u]")
    _req(wh_p.shape == (u, N4) and wh_p.is_contiguous() and wh_p.dtype in H16, "lstm2 bwd: wh_p bf16 / f16 [u,4u]")
    dt = wh_p.dtype
    _req(gates_dtype in (torch.float32, dt), "lstm2 bwd: gates f32 (or the layer's 16-bit type: row-parallel form)")
    _req(gates.shape == (T, B, N4) and gates.dtype == gates_dtype and gates.is_contiguous(), "lstm2 bwd: gates")
    _req(c.shape == (T, B, u) and c.dtype == torch.float32 and c.is_contiguous(), "lstm2 bwd: c")
    _req(dz_T is None or (dz_T.shape == (T, B, N4) and dz_T.dtype == dt and dz_T.is_contiguous()), "lstm2 bwd: dz_T [T,B,4u] in the layer's 16-bit type")
    kblock = dzT_t is not None and dzT_t.dim() == 3         # [T*B/32, 4u, 32]: the K-blocked layout (row-parallel form only; ld_t = 0 in the ABI)
    _req(dzT_t is None or (kblock and dzT_t.shape == (T * B // 32, N4, 32) and dzT_t.is_contiguous() and dzT_t.dtype == dt and B % 32 == 0)
         or (dzT_t.dim() == 2 and dzT_t.shape[0] == N4 and dzT_t.stride(1) == 1 and dzT_t.shape[1] >= T * B and dzT_t.dtype == dt), "lstm2 bwd: dzT_t")
    _req(db_p is None or (db_p.dtype == torch.float32 and db_p.numel() == N4 and (dzT_t is not None or dz_T is not None)), "lstm2 bwd: db_p")
    _req(ws.numel() >= B * u * 4, "lstm2 bwd: workspace too small")
    _req(mask is None or (mask.dtype == torch.uint8 and mask.shape == (T, B, u) and mask.is_contiguous()), "lstm2 bwd: mask u8 [T,B,u]")
    _req(wx_p is None or (wx_p.dim() == 2 and wx_p.shape[1] == N4 and wx_p.is_contiguous() and wx_p.dtype == dt), "lstm2 bwd: wx_p [n_in,4u]")
    for t in (wh_p, gates, c, ws):
        _ptr(t)
    return _lib.LstmBwdLayer(u, _p0(dh_ext), _p0(wh_p), _p0(gates), _p0(c), _p0(c0), None, _p0(dz_T), _p0(ws), _p0(dzT_t),
                             dzT_t.stride(0) if (dzT_t is not None and not kblock) else 0, _p0(db_p), _p0(mask), _p0(wx_p), 1 if dt == torch.float16 else 0)


def lstm2_seq_bwd(T, B, L1, L2, keep_prob, k_begin=0, k_end=None):
    k_end = T + 2 if k_end is None else k_end
    _req(0 <= k_begin < k_end <= T + 2, "lstm2_bwd: bad launch range")
    call("mnn_lstm2_seq_bwd", _stream(), T, B, C.byref(L1), C.byref(L2), float(keep_prob), int(k_begin), int(k_end))


def lstm2_persist_ok(B, u1, u2):
    """True when the persistent (one launch for all T steps) recurrence can run this shape on this device."""
    return bool(_lib.load().mnn_lstm2_persist_ok(int(B), int(u1), int(u2)))


def lstm2_persist_workspace(T, B, u1, u2, device):
    """Progress flags + exchange area of the persistent recurrence (zeroed here, once)."""
    n = _lib.load().mnn_lstm2_persist_workspace_bytes(int(T), int(B), int(u1), int(u2))
    return torch.zeros(n, dtype=torch.uint8, device=device)


def _ws_ok(ws, T, B, L1, L2):
    _req(ws.dtype == torch.uint8 and ws.is_contiguous() and ws.data_ptr() % 256 == 0
         and ws.numel() >= _lib.load().mnn_lstm2_persist_workspace_bytes(int(T), int(B), L1.units, L2.units),
         "lstm2 persist: workspace must be the tensor of lstm2_persist_workspace(T, B, u1, u2)")


def lstm2_persist_fwd(T, B, L1, L2, keep_prob, ws):
    _ws_ok(ws, T, B, L1, L2)
    call("mnn_lstm2_persist_fwd", _stream(), T, B, C.byref(L1), C.byref(L2), float(keep_prob), _ptr(ws))


def lstm2_persist_bwd(T, B, L1, L2, keep_prob, ws):
    _ws_ok(ws, T, B, L1, L2)
    call("mnn_lstm2_persist_bwd", _stream(), T, B, C.byref(L1), C.byref(L2), float(keep_prob), _ptr(ws))


def lstm2_persist_check(ws, B, u1, u2):
    """Raise if any persistent launch that used this workspace gave up on a bounded spin (synchronises)."""
    st = C.c_int(0)
    call("mnn_lstm2_persist_status", _ptr(ws), int(B), int(u1), int(u2), C.byref(st))
    if st.value != 0:
        raise _lib.MnnError("persistent LSTM launch timed out waiting for a neighbouring workgroup (grid not co-resident?)")


def lstm_rowpar_ok(B, units):
    """True when the row-parallel persistent recurrence (one layer per launch, weights in LDS, a wave per row tile) covers this shape."""
    return bool(_lib.load().mnn_lstm_rowpar_ok(int(B), int(units)))


def lstm_rowpar_workspace(T, B, units, device):
    """Progress flags + exchange area of one layer's row-parallel launches (zeroed here, once; forward and backward share it)."""
    return torch.zeros(_lib.load().mnn_lstm_rowpar_workspace_bytes(int(T), int(B), int(units)), dtype=torch.uint8, device=device)


def _rp_ws_ok(ws, T, B, units):
    _req(ws.dtype == torch.uint8 and ws.is_contiguous() and ws.data_ptr() % 256 == 0
         and ws.numel() >= _lib.load().mnn_lstm_rowpar_workspace_bytes(int(T), int(B), int(units)),
         "lstm rowpar: workspace must be the tensor of lstm_rowpar_workspace(T, B, units)")


def lstm_rowpar_fwd(T, B, L, keep_prob, ws):
    """L: descriptor of lstm2_fwd_layer (xproj gate-minor incl. bias; no h0 / c0)."""
    _rp_ws_ok(ws, T, B, L.units)
    call("mnn_lstm_rowpar_fwd", _stream(), T, B, C.byref(L), float(keep_prob), _ptr(ws))


def lstm_rowpar_bwd(T, B, L, keep_prob, ws):
    """L: descriptor of lstm2_bwd_layer (dh_ext required; dz_T = optional row-major bf16 dz for the input-gradient GEMM)."""
    _rp_ws_ok(ws, T, B, L.units)
    call("mnn_lstm_rowpar_bwd", _stream(), T, B, C.byref(L), float(keep_prob), _ptr(ws))


def lstm_resident_ok(B, units):
    """True when the CU-resident recurrence (a 256-unit layer's whole recurrent matrix on every CU, four batch rows per workgroup) covers this shape."""
    return bool(_lib.load().mnn_lstm_resident_ok(int(B), int(units)))


def lstm_resident_fwd(T, B, L, keep_prob):
    """L: descriptor of lstm2_fwd_layer, as for lstm_rowpar_fwd with a 16-bit xproj; no workspace."""
    call("mnn_lstm_resident_fwd", _stream(), T, B, C.byref(L), float(keep_prob))


def _dc0_ok(dc0, B, units):
    _req(dc0.shape == (B, units) and dc0.dtype == torch.float32 and dc0.is_contiguous(), "lstm bwd: dc0 f32 [B,u]")


def lstm_resident_bwd(T, B, L, keep_prob, dc0=None):
    """L: descriptor of lstm2_bwd_layer, as for lstm_rowpar_bwd (its c0, when given, is the initial cell state); no workspace.
    dc0 (optional f32 [B,u]) receives the gradient wrt the initial cell state."""
    if dc0 is None:
        call("mnn_lstm_resident_bwd", _stream(), T, B, C.byref(L), float(keep_prob))
    else:
        _dc0_ok(dc0, B, L.units)
        call("mnn_lstm_resident_bwd_state", _stream(), T, B, C.byref(L), float(keep_prob), _ptr(dc0))


def lstm_cluster_ok(B, units):
    """True when the cluster form of the CU-resident recurrence (512 units: eight CUs share 32 rows, all weights in registers) covers this shape."""
    return bool(_lib.load().mnn_lstm_cluster_ok(int(B), int(units)))


def lstm_cluster_bwd_ok(B, units):
    """True when the cluster BACKWARD may run: the shape is covered and every cluster of the launch is dealt onto one XCD (asked on the host by one
    probe launch per device and batch size, cached in the library; False under MNN_PERSIST_NO_LOCAL).  False: take lstm_rowpar_bwd."""
    return bool(_lib.load().mnn_lstm_cluster_bwd_ok(int(B), int(units)))


def lstm_recurrence_multi(kind, T, B, descs, keep_prob, wss=None, dc0s=None):
    """One launch for several independent layers of one shape (the per-track generators of the jamming mode).  kind: 'resident_fwd' |
    'resident_bwd' | 'cluster_fwd' | 'cluster_bwd'; descs: the layers' descriptors (lstm2_fwd_layer / lstm2_bwd_layer); wss: cluster forms: one
    lstm_rowpar_workspace per job; dc0s (backward kinds): per job an f32 [B,u] tensor for the gradient wrt the initial cell state, or None."""
    n = len(descs)
    _req(1 <= n <= 8, "lstm_recurrence_multi: 1..8 jobs")
    fwd = kind.endswith("fwd")
    arr = ((_lib.LstmFwdLayer if fwd else _lib.LstmBwdLayer) * n)(*descs)
    dptr = None
    if dc0s is not None and any(d is not None for d in dc0s):
        _req(not fwd and len(dc0s) == n, "lstm_recurrence_multi: dc0s goes with a backward kind, one entry per job")
        for d, L in zip(dc0s, descs):
            if d is not None:
                _dc0_ok(d, B, L.units)
        dptr = (C.c_void_p * n)(*[_p0(d) for d in dc0s])
    if kind.startswith("resident"):
        if dptr is not None:
            call("mnn_lstm_resident_bwd_state_multi", _stream(), T, B, n, arr, float(keep_prob), dptr)
        else:
            call("mnn_lstm_resident_%s_multi" % ("fwd" if fwd else "bwd"), _stream(), T, B, n, arr, float(keep_prob))
    else:
        _req(wss is not None and len(wss) == n, "lstm_recurrence_multi: one workspace per job")
        for ws, d in zip(wss, descs):
            _rp_ws_ok(ws, T, B, d.units)
        ptrs = (C.c_void_p * n)(*[ws.data_ptr() for ws in wss])
        if dptr is not None:
            call("mnn_lstm_cluster_bwd_state_multi", _stream(), T, B, n, arr, float(keep_prob), ptrs, dptr)
        else:
            call("mnn_lstm_cluster_%s_multi" % ("fwd" if fwd else "bwd"), _stream(), T, B, n, arr, float(keep_prob), ptrs)
    return arr            # (keeps the by-value copies alive until the call has returned)


def lstm_cluster_bwd_multi_ok(B, units, njobs):
    return bool(_lib.load().mnn_lstm_cluster_bwd_multi_ok(int(B), int(units), int(njobs)))


def lstm_cluster_fwd(T, B, L, keep_prob, ws):
    """L: descriptor of lstm2_fwd_layer, as for lstm_rowpar_fwd with a 16-bit xproj; ws: the tensor of lstm_rowpar_workspace(T, B, 512)."""
    _rp_ws_ok(ws, T, B, L.units)
    call("mnn_lstm_cluster_fwd", _stream(), T, B, C.byref(L), float(keep_prob), _ptr(ws))


def lstm_cluster_bwd(T, B, L, keep_prob, ws, dc0=None):
    """L: descriptor of lstm2_bwd_layer, as for lstm_rowpar_bwd (its c0, when given, is the initial cell state); ws: the tensor of
    lstm_rowpar_workspace(T, B, 512); T >= 4.  dc0 (optional f32 [B,u]) receives the gradient wrt the initial cell state."""
    _rp_ws_ok(ws, T, B, L.units)
    if dc0 is None:
        call("mnn_lstm_cluster_bwd", _stream(), T, B, C.byref(L), float(keep_prob), _ptr(ws))
    else:
        _dc0_ok(dc0, B, L.units)
        call("mnn_lstm_cluster_bwd_state", _stream(), T, B, C.byref(L), float(keep_prob), _ptr(ws), _ptr(dc0))


def lstm_rowpar_check(ws):
    st = C.c_int(0)
    call("mnn_lstm_rowpar_status", _ptr(ws), C.byref(st))
    if st.value != 0:
        raise _lib.MnnError("row-parallel LSTM launch timed out waiting for a neighbouring wave (grid not co-resident?)")


def dropout_mask(mask, keep_prob, seed, row0, layer, step_dev=None):
    T, B, u = mask.shape
    _req(mask.dtype == torch.uint8 and mask.is_contiguous() and u % 4 == 0 and 0 < keep_prob < 1, "dropout_mask: u8 [T,B,u], 0<kp<1")
    _step_ok(step_dev)
    call("mnn_dropout_mask", _stream(), _ptr(mask), T, B, u, float(keep_prob), int(seed), _ptr(step_dev), int(row0), int(layer))


def dropout_fwd(h, y, keep_prob, seed, row0, layer, step_dev=None, t_offset=0):
    T, B, u = h.shape
    _req(h.is_contiguous() and y.is_contiguous() and h.shape == y.shape and h.dtype == y.dtype and u % 4 == 0, "dropout_fwd: shapes")
    _step_ok(step_dev)
    call("mnn_dropout_fwd", _stream(), dtype_code(h), _ptr(h), _ptr(y), T, B, u, float(keep_prob), int(seed), _ptr(step_dev), int(row0),
         int(layer), int(t_offset))


def dropout_bwd(dy, dh, keep_prob, seed, row0, layer, accumulate=False, step_dev=None, t_offset=0):
    T, B, u = dy.shape
    _req(dy.dtype == torch.float32 and dh.dtype == torch.float32 and dy.is_contiguous() and dh.is_contiguous() and dy.shape == dh.shape,
         "dropout_bwd: f32 [T,B,u]")
    _step_ok(step_dev)
    call("mnn_dropout_bwd", _stream(), _ptr(dy), _ptr(dh), T, B, u, float(keep_prob), int(seed), _ptr(step_dev), int(row0), int(layer),
         int(accumulate), int(t_offset))


# ------------------------------------------------------------------------------------------------
def _nade_check(tracks, N, D, Hn, v, bias, w_enc, w_dec):
    _req(v.dtype == torch.uint8 and v.is_contiguous() and v.numel() == tracks * N * D, "nade: v must be contiguous u8 [tracks,N,D]")
    _req(bias.dtype == torch.float32 and bias.dim() == 2 and bias.shape[0] == N and bias.stride(1) == 1
         and bias.shape[1] >= tracks * (Hn + D), "nade: bias f32 [N, >=tracks*(Hn+D)]")
    for w in (w_enc, w_dec):
        _req(w.dtype == torch.float32 and w.is_contiguous() and w.numel() == tracks * D * Hn, "nade: weights f32 [tracks,D,Hn]")
    _req(0 < Hn <= 256, "nade: Hn must be in 1..256")


def nade_logprob_fwd(v, bias, w_enc, w_dec, tracks, D, Hn, row_weight=None, nll=None, cond_p=None, d_bias=None, a_final=None, n_rows_dev=None,
                     gate=None, run_if=0, unsafe=None):
    N = bias.shape[0]
    _nade_check(tracks, N, D, Hn, v, bias, w_enc, w_dec)
    if nll is not None:
        _req(nll.dtype == torch.float32 and nll.numel() == tracks * N and nll.is_contiguous(), "nade: nll f32 [tracks,N]")
    if cond_p is not None:
        _req(cond_p.dtype == torch.float32 and cond_p.numel() == tracks * N * D and cond_p.is_contiguous(), "nade: cond_p f32 [tracks,N,D]")
    if d_bias is not None:
        _req(row_weight is not None and d_bias.shape == bias.shape and d_bias.stride() == bias.stride() and d_bias.dtype == torch.float32,
             "nade: d_bias must mirror bias and needs row_weight")
    if row_weight is not None:
        _req(row_weight.dtype == torch.float32 and row_weight.numel() == N, "nade: row_weight f32 [N]")
    if a_final is not None:
        _req(a_final.dtype == torch.float32 and a_final.numel() == tracks * N * Hn and a_final.is_contiguous(), "nade: a_final f32 [tracks,N,Hn]")
    _req(unsafe is None or (unsafe.dtype == torch.int32 and unsafe.numel() == 1), "nade: unsafe int32[1]")
    if n_rows_dev is not None or gate is not None or unsafe is not None:   # compacted ragged batch / a density-gated launch: the gated entry point (gate NULL: always runs)
        call("mnn_nade_logprob_fwd_gated", _stream(), tracks, N, D, Hn, _ptr(v), N * D, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec),
             _ptr(row_weight), _ptr(nll), _ptr(cond_p), _ptr(d_bias), _ptr(a_final), _ptr(gate), int(run_if), _ptr(n_rows_dev), _ptr(unsafe))
        return
    call("mnn_nade_logprob_fwd", _stream(), tracks, N, D, Hn, _ptr(v), N * D, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec),
         _ptr(row_weight), _ptr(nll), _ptr(cond_p), _ptr(d_bias), _ptr(a_final))


def nade_mfma_ok(Hn):
    """True when the matrix-core NADE kernels cover this hidden width."""
    return bool(_lib.load().mnn_nade_mfma_ok(int(Hn)))


def nade_logprob_fwd_mfma(v, bias, w_enc, w_dec_bf, tracks, D, Hn, row_weight=None, nll=None, cond_p=None, d_bias=None, a_final=None):
    """nade_logprob_fwd with the decoder dot products on MFMA (bf16 operands): w_dec_bf is the bf16 copy of w_dec."""
    N = bias.shape[0]
    _nade_check(tracks, N, D, Hn, v, bias, w_enc, w_enc)
    _req(w_dec_bf.dtype == torch.bfloat16 and w_dec_bf.is_contiguous() and w_dec_bf.numel() == tracks * D * Hn, "nade mfma: w_dec_bf bf16 [tracks,D,Hn]")
    if nll is not None:
        _req(nll.dtype == torch.float32 and nll.numel() == tracks * N and nll.is_contiguous(), "nade: nll f32 [tracks,N]")
    if cond_p is not None:
        _req(cond_p.dtype == torch.float32 and cond_p.numel() == tracks * N * D and cond_p.is_contiguous(), "nade: cond_p f32 [tracks,N,D]")
    if d_bias is not None:
        _req(row_weight is not None and d_bias.shape == bias.shape and d_bias.stride() == bias.stride() and d_bias.dtype == torch.float32,
             "nade: d_bias must mirror bias and needs row_weight")
    if row_weight is not None:
        _req(row_weight.dtype == torch.float32 and row_weight.numel() == N, "nade: row_weight f32 [N]")
    if a_final is not None:
        _req(a_final.dtype == torch.float32 and a_final.numel() == tracks * N * Hn and a_final.is_contiguous(), "nade: a_final f32 [tracks,N,Hn]")
    call("mnn_nade_logprob_fwd_mfma", _stream(), tracks, N, D, Hn, _ptr(v), N * D, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec_bf),
         _ptr(row_weight), _ptr(nll), _ptr(cond_p), _ptr(d_bias), _ptr(a_final))


def nade_f32_pack(w_dec, out):
    """w_dec f32 [rows, Hn] -> out (an f32 [rows, Hn] buffer holding f16 [rows][hi | lo][Hn], hi = f16(w), lo = f16(w - hi)): the decoder
    operand of the split-operand matrix-core NADE forward (precision "fp16")."""
    _rowmajor(w_dec, "f32_pack w_dec"); _rowmajor(out, "f32_pack out")
    rows, Hn = w_dec.shape
    _req(w_dec.dtype == torch.float32 and w_dec.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous()
         and out.shape == (rows, Hn) and Hn % 8 == 0, "f32_pack: w_dec f32 [rows,Hn] -> out f32 [rows,Hn], Hn % 8 == 0")
    call("mnn_nade_f32_pack", _stream(), _ptr(w_dec), rows, Hn, _ptr(out))
    return out


def nade_logprob_fwd_auto(v, bias, w_enc, w_dec, w_dec_bf, tracks, D, Hn, gate, count, dense_above=0.07, row_weight=None, nll=None,
                          cond_p=None, d_bias=None, a_final=None, exact=False, counted=False, n_rows_dev=None, unsafe=None):
    """16-bit compute modes (exact=True: the split-operand hi + lo form of fp16 mode): the matrix-core form of the scan when at most `dense_above` of the cells of v are active, the f32 vector
    form otherwise; decided on the device (mnn_density_gate), both launches issued (one returns at once).  gate int32[1], count: a zeroed
    int32[1] scratch word (left zero)."""
    N = bias.shape[0]
    _nade_check(tracks, N, D, Hn, v, bias, w_enc, w_dec)
    _req(w_dec_bf.dtype == (torch.float32 if exact else torch.bfloat16) and w_dec_bf.is_contiguous() and w_dec_bf.numel() == tracks * D * Hn,
         "nade auto: w_dec_bf bf16 [tracks,D,Hn] (exact form: the f32-sized [tracks,D,Hn] output of nade_f32_pack)")
    _req(gate is None or (gate.dtype == torch.int32 and gate.numel() == 1 and count.dtype == torch.int32 and count.numel() == DENSITY_SLOTS and count.is_contiguous()),
         "nade auto: gate int32[1], count int32[DENSITY_SLOTS]")
    for t, n in ((nll, tracks * N), (cond_p, tracks * N * D), (a_final, tracks * N * Hn)):
        _req(t is None or (t.dtype == torch.float32 and t.numel() == n and t.is_contiguous()), "nade auto: f32 outputs")
    if d_bias is not None:
        _req(row_weight is not None and d_bias.shape == bias.shape and d_bias.stride() == bias.stride() and d_bias.dtype == torch.float32,
             "nade: d_bias must mirror bias and needs row_weight")
    if row_weight is not None:
        _req(row_weight.dtype == torch.float32 and row_weight.numel() == N, "nade: row_weight f32 [N]")
    common = (tracks, N, D, Hn, _ptr(v), N * D, _ptr(bias), bias.stride(0), _ptr(w_enc))
    tail = (_ptr(row_weight), _ptr(nll), _ptr(cond_p), _ptr(d_bias), _ptr(a_final), _ptr(gate))
    mfma = "mnn_nade_logprob_fwd_mfma_f32" if exact else "mnn_nade_logprob_fwd_mfma_gated"
    nr = _ptr(n_rows_dev)                           # compacted ragged batch: the scans skip workgroups of padding (ragged_index)
    if gate is None:                                # gate off: always the matrix-core form
        call(mfma, _stream(), *common, _ptr(w_dec_bf), *tail, 0, nr)
        return
    # counted: `count` already holds the set cells of v (the piano-roll pass counted them while writing v): only the decision kernel runs
    call("mnn_density_gate", _stream(), None if counted else _ptr(v), v.numel(), int(dense_above * v.numel()), _ptr(gate), _ptr(count))
    call(mfma, _stream(), *common, _ptr(w_dec_bf), *tail, 0, nr)
    _req(unsafe is None or (unsafe.dtype == torch.int32 and unsafe.numel() == 1), "nade auto: unsafe int32[1]")
    call("mnn_nade_logprob_fwd_gated", _stream(), *common, _ptr(w_dec), *tail, 1, nr, _ptr(unsafe))


def nade_logprob_bwd(v, bias, w_enc, w_dec, tracks, D, Hn, a_final, d_bias, d_w_enc, d_w_dec, n_rows_dev=None, unsafe=None):
    """unsafe (int32[1]): the counter the forward's density-gated dense launch left (nade_logprob_fwd_auto / nade_logprob_fwd) -- 0 (the dense
    form ran and no wave passed |a| = 40): the scan advances exp(-a) multiplicatively (no exponential per flip; decided on the device, both
    instantiations launched); None: the direct form."""
    _req(unsafe is None or (unsafe.dtype == torch.int32 and unsafe.numel() == 1), "nade bwd: unsafe int32[1]")
    N = bias.shape[0]
    _nade_check(tracks, N, D, Hn, v, bias, w_enc, w_dec)
    _req(d_bias.shape == bias.shape and d_bias.stride() == bias.stride() and d_bias.dtype == torch.float32, "nade bwd: d_bias")
    for w in (d_w_enc, d_w_dec):
        _req(w.dtype == torch.float32 and w.is_contiguous() and w.numel() == tracks * D * Hn, "nade bwd: grad weights f32 [tracks,D,Hn]")
    _req(a_final.dtype == torch.float32 and a_final.numel() == tracks * N * Hn and a_final.is_contiguous(), "nade bwd: a_final f32 [tracks,N,Hn]")
    call("mnn_nade_logprob_bwd", _stream(), tracks, N, D, Hn, _ptr(v), N * D, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec),
         _ptr(a_final), _ptr(d_bias), _ptr(d_w_enc), _ptr(d_w_dec), _ptr(n_rows_dev), _ptr(unsafe))


def _temps(temperature, n_per_job, by_visible, what):
    """None (a float, or None: the entry point that takes one float serves it, as it always did) or the mnn_temps of a SEQUENCE of
    temperatures: one per track / job (n_per_job of them), or -- by_visible -- visible i draws at temperature[i % len(temperature)]."""
    if temperature is None or isinstance(temperature, (int, float)):
        return None
    t = tuple(float(x) for x in temperature)
    _req(1 <= len(t) <= _lib.TEMPS_MAX and all(math.isfinite(x) and x > 0.0 for x in t),
         f"{what}: 1..{_lib.TEMPS_MAX} positive finite temperatures")
    _req(by_visible or len(t) in (1, n_per_job), f"{what}: one temperature, or one per track / job ({n_per_job})")
    st = _lib.Temps()
    st.n, st.by_visible = len(t), 1 if by_visible else 0
    for i, x in enumerate(t):
        st.t[i] = x
    return st


def _temps_table(temperature, n_per_job, by_visible, what):
    """The mnn_temps of ANY temperature argument (the entry points that take only a table): None -> n = 0 (threshold draws), a float -> one entry."""
    if temperature is None:
        return _lib.Temps()
    return _temps((temperature,) if isinstance(temperature, (int, float)) else temperature, n_per_job, by_visible, what)


def _caps(max_notes, n_per_job, by_visible, what):
    """None (no cap: the entry points without one serve the call, as they always did) or the mnn_caps of a `max_notes`: an int >= 0 (one
    cap for every track / job) or a sequence of ints >= 0 / None (no cap for that one) -- one per track / job (n_per_job of them), or --
    by_visible -- visible i counts in max_notes[i % len(max_notes)]."""
    if max_notes is None:
        return None
    seq = (max_notes,) if isinstance(max_notes, int) else tuple(max_notes)
    _req(1 <= len(seq) <= _lib.TEMPS_MAX and all(k is None or (isinstance(k, int) and not isinstance(k, bool) and k >= 0) for k in seq),
         f"{what}: max_notes: 1..{_lib.TEMPS_MAX} integers >= 0 (None: no cap)")
    _req(by_visible or len(seq) in (1, n_per_job), f"{what}: one cap, or one per track / job ({n_per_job})")
    if all(k is None for k in seq):
        return None
    sc = _lib.Caps()
    sc.n, sc.by_visible = len(seq), 1 if by_visible else 0
    for i, k in enumerate(seq):
        sc.cap[i] = -1 if k is None else min(k, 0x3fffffff)
    return sc


def _redraw(redraws, redraw_stats, cc, temperature, ref, what):
    """None (no redraws, or no caps to violate: the entry points without them serve the call, as they always did) or the mnn_redraw of
    `redraws` tries; redraw_stats: None, or two int32 on the device of `ref` that the kernels add their (redrawn, fallback) scans to."""
    _req(isinstance(redraws, int) and not isinstance(redraws, bool) and 0 <= redraws <= _lib.REDRAWS_MAX,
         f"{what}: redraws: an integer 0..{_lib.REDRAWS_MAX}")
    if redraw_stats is not None:
        _req(torch.is_tensor(redraw_stats) and redraw_stats.dtype == torch.int32 and redraw_stats.numel() == 2 and redraw_stats.is_contiguous()
             and redraw_stats.device == ref.device, f"{what}: redraw_stats is int32[2] on the device")
    _req(redraws == 0 or temperature is not None, f"{what}: redraws need a temperature (threshold decoding would draw the same vector again)")
    if redraws == 0 or cc is None:
        return None
    rd = _lib.Redraw()
    rd.tries, rd.stats = redraws, _ptr(redraw_stats)
    return rd


def _sub_base(sub_base, ref, what):
    """A generation session's step cell: None, or ONE 32-bit integer on the device of `ref` that the sampling kernels add to their sub-counter."""
    if sub_base is not None:
        _req(torch.is_tensor(sub_base) and sub_base.dtype == torch.int32 and sub_base.numel() == 1 and sub_base.device == ref.device,
             f"{what}: sub_base is one int32 on the device")
    return _ptr(sub_base)


def nade_sample(bias, w_enc, w_dec, tracks, D, Hn, temperature, seed, row0, sub, samples, track_minor=False, nll=None, given=None,
                by_visible=False, sub_base=None, max_notes=None, redraws=0, redraw_stats=None):
    """samples u8 [N, tracks*D]; feature index m*D+i (track_minor False) or i*tracks+m (True, rnn_multinade.py:313-314).
    temperature: a float, None (threshold draws) or a sequence -- one temperature per track, or with by_visible the temperature of visible
    i is temperature[i % len] (a joint NADE over visibles p * M + m: one per track m).  nll stays the model's own at any temperature.
    given (optional): codes u8 [N, tracks*D] in the layout of samples -- 0 / 1 clamp the visible to that value, 255 leaves it to the draw
    (common.given_codes).  sub_base (optional, one int32 on the device): the draws use the sub-counter sub + *sub_base, read by the kernel
    (mnn_nade_sample_temps_at): a captured launch follows the cell.  max_notes (optional, mnn_nade_sample_caps_at): at most that many ones per
    track and row -- an int, or a sequence read like a temperature sequence (per track, or by visible index), None entries uncapped; given
    ones count, a free visible of an exhausted track is a settled 0 that uses no uniform.  None: the calls below, as without the argument.
    redraws (0..255, mnn_nade_sample_redraw_at): the cap by rejection -- a row that would emit a 1 past a cap is drawn again, up to `redraws`
    times, before the truncating scan above serves it; redraw_stats (optional int32[2] on the device) gains the (redrawn, fallback) scans.
    redraws = 0, or caps that cannot bind: the calls below."""
    N = bias.shape[0]
    _req(bias.dtype == torch.float32 and bias.dim() == 2 and bias.stride(1) == 1 and bias.shape[1] >= tracks * (Hn + D), "sample: bias")
    _req(samples.dtype == torch.uint8 and samples.shape == (N, tracks * D) and samples.is_contiguous(), "sample: samples u8 [N,tracks*D]")
    for w in (w_enc, w_dec):
        _req(w.dtype == torch.float32 and w.is_contiguous() and w.numel() == tracks * D * Hn, "sample: weights")
    if nll is not None:
        _req(nll.dtype == torch.float32 and nll.numel() == tracks * N, "sample: nll")
    if given is not None:
        _req(given.dtype == torch.uint8 and tuple(given.shape) == (N, tracks * D) and given.is_contiguous() and given.device == samples.device,
             "sample: given u8 [N, tracks*D], contiguous")
    ts, es = (1, tracks) if track_minor else (D, 1)
    cc = _caps(max_notes, tracks, by_visible, "sample")
    rd = _redraw(redraws, redraw_stats, cc, temperature, samples, "sample")
    if rd is not None:
        tt = _temps_table(temperature, tracks, by_visible, "sample")
        call("mnn_nade_sample_redraw_at", _stream(), tracks, N, D, Hn, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec), C.byref(tt), C.byref(cc),
             int(seed), int(row0), int(sub), _ptr(samples), ts, tracks * D, es, _ptr(nll), _ptr(given), _sub_base(sub_base, samples, "sample"),
             C.byref(rd))
        return
    if cc is not None:
        tt = _temps_table(temperature, tracks, by_visible, "sample")
        call("mnn_nade_sample_caps_at", _stream(), tracks, N, D, Hn, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec), C.byref(tt), C.byref(cc),
             int(seed), int(row0), int(sub), _ptr(samples), ts, tracks * D, es, _ptr(nll), _ptr(given), _sub_base(sub_base, samples, "sample"))
        return
    if sub_base is not None:
        tt = _temps_table(temperature, tracks, by_visible, "sample")
        call("mnn_nade_sample_temps_at", _stream(), tracks, N, D, Hn, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec), C.byref(tt), int(seed),
             int(row0), int(sub), _ptr(samples), ts, tracks * D, es, _ptr(nll), _ptr(given), _sub_base(sub_base, samples, "sample"))
        return
    tt = _temps(temperature, tracks, by_visible, "sample")
    if tt is not None:
        call("mnn_nade_sample_temps", _stream(), tracks, N, D, Hn, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec), C.byref(tt), int(seed),
             int(row0), int(sub), _ptr(samples), ts, tracks * D, es, _ptr(nll), _ptr(given))
        return
    call("mnn_nade_sample", _stream(), tracks, N, D, Hn, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec),
         float(-1.0 if temperature is None else temperature), int(seed), int(row0), int(sub), _ptr(samples), ts, tracks * D, es, _ptr(nll), _ptr(given))


def nade_sample_multi(jobs, D, Hn, temperature, row0, sub, max_notes=None, redraws=0, redraw_stats=None):
    """mnn_nade_sample for up to 8 single-NADE generators in ONE launch.  job = dict(bias f32 [N, >= Hn + D] (the generator's Dense output),
    w_enc / w_dec f32 [D, Hn], seed, samples = a u8 [N, D] VIEW (any strides, the same for every job: e.g. out[:, s, :, m] of a
    [B, steps, P, M] piano-roll), nll f32 [N] or None, given = None or a u8 [N, D] view of codes with the strides of samples).
    temperature: a float, None, or a sequence with one temperature per job.  max_notes: None, an int, or a sequence with one cap (or None)
    per job (nade_sample).  redraws / redraw_stats: nade_sample's (mnn_nade_sample_multi_redraw)."""
    _req(1 <= len(jobs) <= 8, "nade_sample_multi: 1..8 jobs")
    arr = (_lib.NadeSampleJob * len(jobs))()
    N = jobs[0]["bias"].shape[0]
    rs, es = jobs[0]["samples"].stride()
    for a, j in zip(arr, jobs):
        b, smp, nll = j["bias"], j["samples"], j.get("nll")
        _req(b.dtype == torch.float32 and b.dim() == 2 and b.stride(1) == 1 and b.shape == (N, b.shape[1]) and b.shape[1] >= Hn + D, "sample_multi: bias")
        _req(smp.dtype == torch.uint8 and tuple(smp.shape) == (N, D) and smp.stride() == (rs, es) and es >= 1, "sample_multi: samples u8 [N, D] views of equal strides")
        for w in (j["w_enc"], j["w_dec"]):
            _req(w.dtype == torch.float32 and w.is_contiguous() and w.numel() == D * Hn, "sample_multi: weights f32 [D, Hn]")
        _req(nll is None or (nll.dtype == torch.float32 and nll.is_contiguous() and nll.numel() == N), "sample_multi: nll f32 [N]")
        gv = j.get("given")
        _req(gv is None or (gv.dtype == torch.uint8 and tuple(gv.shape) == (N, D) and gv.stride() == (rs, es) and gv.device == smp.device),
             "sample_multi: given u8 [N, D] with the strides of samples")
        a.bias, a.ld_bias, a.w_enc, a.w_dec, a.seed, a.samples, a.nll = _ptr(b), b.stride(0), _ptr(j["w_enc"]), _ptr(j["w_dec"]), int(j["seed"]), _ptr(smp), _ptr(nll)
        a.given = _ptr(gv)
    cc = _caps(max_notes, len(jobs), False, "sample_multi")
    rd = _redraw(redraws, redraw_stats, cc, temperature, jobs[0]["samples"], "sample_multi")
    if rd is not None:
        tt = _temps_table(temperature, len(jobs), False, "sample_multi")
        call("mnn_nade_sample_multi_redraw", _stream(), len(jobs), arr, N, D, Hn, C.byref(tt), C.byref(cc), int(row0), int(sub), rs, es, C.byref(rd))
        return
    if cc is not None:
        tt = _temps_table(temperature, len(jobs), False, "sample_multi")
        call("mnn_nade_sample_multi_caps", _stream(), len(jobs), arr, N, D, Hn, C.byref(tt), C.byref(cc), int(row0), int(sub), rs, es)
        return
    tt = _temps(temperature, len(jobs), False, "sample_multi")
    if tt is not None:
        call("mnn_nade_sample_multi_temps", _stream(), len(jobs), arr, N, D, Hn, C.byref(tt), int(row0), int(sub), rs, es)
        return
    call("mnn_nade_sample_multi", _stream(), len(jobs), arr, N, D, Hn, float(-1.0 if temperature is None else temperature), int(row0), int(sub), rs, es)


def _sir(what, particles, ess, pick, shape, tracks, N, D, ref):
    """The mnn_sir of a call with particles = C >= 2 (and the workspace tensor that backs it, to be kept until the call is enqueued): ess f32 and
    pick int32 of `shape` on ref's device, written by the kernels."""
    _req(isinstance(particles, int) and not isinstance(particles, bool) and 2 <= particles <= _lib.PARTICLES_MAX,
         f"{what}: particles: an integer 2..{_lib.PARTICLES_MAX}")
    for t, dt, name in ((ess, torch.float32, "ess f32"), (pick, torch.int32, "pick int32")):
        _req(torch.is_tensor(t) and t.dtype == dt and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == ref.device,
             f"{what}: {name} {list(shape)} on the device")
    need = int(_lib.load().mnn_nade_sample_sir_workspace_bytes(tracks, N, D, particles))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=ref.device)
    sr = _lib.Sir()
    sr.particles, sr.ess, sr.pick = particles, _ptr(ess), _ptr(pick)
    sr.workspace, sr.workspace_bytes = C.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256), need
    return sr, ws


def nade_sample_sir_workspace_bytes(tracks, N, D, particles):
    """mnn_nade_sample_sir_workspace_bytes: what a step's particles take between its two launches (0 for particles <= 1)."""
    return int(_lib.load().mnn_nade_sample_sir_workspace_bytes(int(tracks), int(N), int(D), int(particles)))


def nade_sample_sir(bias, w_enc, w_dec, tracks, D, Hn, temperature, seed, row0, sub, samples, given, particles, track_minor=False, nll=None,
                    by_visible=False, sub_base=None, ess=None, pick=None, log_w=None, v_out=None):
    """nade_sample(given=) by importance resampling (mnn_nade_sample_sir_at; DESIGN.md section 4 "NADE importance resampling"): every scan
    (row, track) runs C = particles clamped scans -- particle 0 the scan of nade_sample, the others on Philox stream 13 -- weighs each by the
    probability of its given cells (at the scan's temperature) and emits one, picked with probability w_c / sum w (one uniform on stream 14).
    samples / given: u8 [N, tracks * D] contiguous as nade_sample takes them (track_minor likewise), or -- tracks == 1 -- two [N, D] VIEWS of
    equal strides (e.g. out[:, s, :, m] of a [B, steps, P, M] piano-roll).  temperature: a float or a sequence (nade_sample), not None.
    Outputs: nll f32 [tracks, N] (optional) the model's own of the emitted vector; ess f32 / pick int32 [tracks, N] (allocated if not given;
    returned; given None: nade_sample's launch, ess = C and pick = 0 written); log_w f32 [tracks, N, C] (optional): every particle's log weight; v_out u8 [tracks, N, C, D] (optional, for tests): the
    particles' vectors, copied out of the workspace.  A scan with no given cell behind a free one runs particle 0 alone: nade_sample's
    bits, ess = C, pick = 0 (and of v_out only its particle 0 is written)."""
    what = "nade_sample_sir"
    N = bias.shape[0]
    _req(bias.dtype == torch.float32 and bias.dim() == 2 and bias.stride(1) == 1 and bias.shape[1] >= tracks * (Hn + D), what + ": bias")
    _req(temperature is not None, what + ": particles need a temperature (threshold decoding draws nothing)")
    _req(torch.is_tensor(samples) and samples.dtype == torch.uint8 and samples.device == bias.device
         and (given is None or (torch.is_tensor(given) and given.dtype == torch.uint8 and given.device == samples.device)),
         what + ": samples and given are u8 tensors on bias's device")
    if given is not None and tracks == 1 and samples.dim() == 2 and tuple(samples.shape) == (N, D) and not samples.is_contiguous():
        rs, es = samples.stride()
        _req(es >= 1 and rs >= 1 and tuple(given.shape) == (N, D) and given.stride() == (rs, es), what + ": given u8 [N, D] with the strides of samples")
        ts = D
    else:
        _req(samples.shape == (N, tracks * D) and samples.is_contiguous(), what + ": samples u8 [N, tracks*D]")
        _req(given is None or (tuple(given.shape) == (N, tracks * D) and given.is_contiguous()), what + ": given u8 [N, tracks*D], contiguous")
        ts, es = (1, tracks) if track_minor else (D, 1)
        rs = tracks * D
    for w in (w_enc, w_dec):
        _req(w.dtype == torch.float32 and w.is_contiguous() and w.numel() == tracks * D * Hn, what + ": weights")
    if nll is not None:
        _req(nll.dtype == torch.float32 and nll.numel() == tracks * N and nll.is_contiguous(), what + ": nll")
    if ess is None:
        ess = torch.empty((tracks, N), device=bias.device)
    if pick is None:
        pick = torch.empty((tracks, N), dtype=torch.int32, device=bias.device)
    sr, ws = _sir(what, particles, ess, pick, (tracks, N), tracks, N, D, bias)
    if log_w is not None:
        _req(log_w.dtype == torch.float32 and tuple(log_w.shape) == (tracks, N, particles) and log_w.is_contiguous() and log_w.device == bias.device,
             what + ": log_w f32 [tracks, N, C]")
    tt = _temps_table(temperature, tracks, by_visible, what)
    call("mnn_nade_sample_sir_at", _stream(), tracks, N, D, Hn, _ptr(bias), bias.stride(0), _ptr(w_enc), _ptr(w_dec), C.byref(tt), int(seed),
         int(row0), int(sub), _ptr(samples), ts, rs, es, _ptr(nll), _ptr(given), _sub_base(sub_base, samples, what), C.byref(sr), _ptr(log_w))
    if v_out is not None and given is not None:      # the workspace's last block (mnn_nade_sample_sir_at): behind log w, nll and the flags, each 256-byte aligned
        _req(v_out.dtype == torch.uint8 and tuple(v_out.shape) == (tracks, N, particles, D) and v_out.is_contiguous() and v_out.device == bias.device,
             what + ": v_out u8 [tracks, N, C, D]")
        scans = tracks * N
        first = (-ws.data_ptr()) % 256 + 2 * round_up(scans * particles * 4, 256) + round_up(scans, 256)
        v_out.view(-1).copy_(ws[first:first + v_out.numel()])
    return ess, pick


def nade_given_is(bias, w_enc, w_dec, tracks, D, Hn, given, num_particles, seed, row0=0, row_ids=None, data=None, log_pg=None, log_w=None,
                  v_out=None, stats=None):
    """Importance-sampling estimate of log p(x_G) per (track, row) of a partly given NADE (mnn_nade_given_is; DESIGN.md section 4 "NADE
    importance estimator").  bias f32 [N, >= tracks * (Hn + D)] and the weights [tracks, D, Hn] as nade_sample takes them; given u8
    [tracks, N, D]: the codes, 0 / 1 given, 255 free (common.given_codes, one contiguous plane per track).  C = num_particles clamped scans
    per (row, track), keyed by (seed, row id, particle): row ids row0 + n, or row_ids int32 [N].  data None: the lower side -- log_pg =
    logsumexp_c(log w_c) - log C is biased LOW.  data u8 [tracks, N, D]: the upper side -- particle 0's free cells are data's, the others
    are drawn on a stream of their own; biased HIGH in expectation over data drawn from the model, not a bound per row.  Returns log_pg f32
    [tracks, N] (allocated if not given); optional outputs: log_w f32 [tracks, N, C], v_out u8 [tracks, N, C, D] the particles' vectors,
    stats f32 [tracks, N, 2] = (effective sample size, standard error of log_pg; inf with one particle)."""
    what = "nade_given_is"
    _req(isinstance(tracks, int) and isinstance(D, int) and isinstance(Hn, int) and tracks >= 1 and 1 <= D <= 1536 and 1 <= Hn <= 256,
         what + ": tracks >= 1, 1 <= D <= 1536, 1 <= Hn <= 256")
    _req(torch.is_tensor(bias) and bias.dtype == torch.float32 and bias.dim() == 2 and bias.stride(1) == 1 and bias.shape[0] >= 1
         and bias.shape[1] >= tracks * (Hn + D) and (bias.stride(0) >= bias.shape[1] or bias.shape[0] == 1), what + ": bias f32 [N, >= tracks * (Hn + D)]")
    N = bias.shape[0]
    for w in (w_enc, w_dec):
        _req(torch.is_tensor(w) and w.dtype == torch.float32 and w.is_contiguous() and w.numel() == tracks * D * Hn, what + ": weights f32 [tracks, D, Hn]")
    for t, name in ((given, "given"), (data, "data")):
        _req((t is None and name == "data") or (torch.is_tensor(t) and t.dtype == torch.uint8 and tuple(t.shape) == (tracks, N, D) and t.is_contiguous()),
             f"{what}: {name} u8 [tracks, N, D], contiguous")
    S = int(num_particles)
    _req(S >= 1, what + ": num_particles >= 1")
    _req(tracks * N * S * D < 2 ** 62, what + ": too many particles")
    if row_ids is not None:
        _req(torch.is_tensor(row_ids) and row_ids.dtype == torch.int32 and row_ids.numel() == N and row_ids.is_contiguous(), what + ": row_ids int32 [N]")
    dev = bias.device
    for t in (w_enc, w_dec, given, data, row_ids):
        _req(t is None or t.device == dev, what + ": every operand on bias's device")
    for t, shape, dt, name in ((log_pg, (tracks, N), torch.float32, "log_pg f32 [tracks, N]"), (log_w, (tracks, N, S), torch.float32, "log_w f32 [tracks, N, C]"),
                               (v_out, (tracks, N, S, D), torch.uint8, "v_out u8 [tracks, N, C, D]"),
                               (stats, (tracks, N, 2), torch.float32, "stats f32 [tracks, N, 2]")):
        if t is not None:
            _req(t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev, what + ": " + name)
    _ptr(bias)                                                       # no CPU path: refuse host tensors before allocating anything
    if log_pg is None:
        log_pg = torch.empty((tracks, N), device=dev)
    ws = torch.empty(_lib.load().mnn_nade_given_is_workspace_bytes(tracks, N, S), dtype=torch.uint8, device=dev)
    call("mnn_nade_given_is", _stream(), tracks, N, D, Hn, _ptr(bias), bias.stride(0) if N > 1 else bias.shape[1], _ptr(w_enc), _ptr(w_dec),
         _ptr(given), N * D, _ptr(data), N * D, S, int(seed), int(row0), _ptr(row_ids), _ptr(log_pg), _ptr(log_w), _ptr(v_out), _ptr(stats), _ptr(ws))
    return log_pg


# ------------------------------------------------------------------------------------------------
def _ldb(b, n):
    _req(b.dtype == torch.float32 and b.dim() == 2 and b.stride(1) == 1 and b.shape[1] >= n, "rbm: bias must be f32 [N or 1, n]")
    return 0 if b.shape[0] == 1 else b.stride(0)


def rbm_workspace(D, Hn, device):
    return torch.empty(_lib.load().mnn_rbm_workspace_bytes(D, Hn), dtype=torch.uint8, device=device)


def _rbm_temperature(t, what):
    _req(isinstance(t, (int, float)) and math.isfinite(t) and t > 0.0, f"{what}: the temperature of an RBM chain is a positive finite number")
    return float(t)


def rbm_gibbs(v0, W, bh, bv, k, seed, row0=0, row_ids=None, sub0=0, p_v=None, v_out=None, seed_step=None, given=None, temperature=1.0,
              sub_base=None):
    """temperature (a positive float; not with seed_step): the chain of the RBM with energy E / T -- every conditional is sigmoid(z / T), p_v
    the tempered probability; 1.0 is the untempered chain, kernels and bits.
    seed_step (int32 device scalar, optional): added to `seed` on the device (graph-replay safe step-dependent draws).
    given (optional): codes u8 [N, D] (row stride >= D: a step slice given[:, s] of a [B, steps, D] block is read in place) -- 0 / 1 clamp
    the visible to that value through the whole chain, 255 leaves it free (common.given_codes); not with seed_step (training's chain).
    sub_base (optional, one int32 on the device; not with seed_step): the chain's sub-counters start at sub0 + *sub_base * max(k, 1), read
    by the kernel (mnn_rbm_gibbs_at)."""
    N, D = v0.shape
    Hn = W.shape[1]
    _req(v0.dtype == torch.uint8 and v0.is_contiguous(), "gibbs: v0 u8 [N,D]")
    _req(W.dtype == torch.float32 and W.shape == (D, Hn) and W.is_contiguous(), "gibbs: W f32 [D,Hn]")
    _req(bh.shape[0] in (1, N) and bv.shape[0] in (1, N), "gibbs: bias rows")
    if p_v is not None:
        _req(p_v.dtype == torch.float32 and p_v.shape == (N, D) and p_v.is_contiguous(), "gibbs: p_v f32 [N,D]")
    if v_out is not None:
        _req(v_out.dtype == torch.uint8 and v_out.shape == (N, D) and v_out.is_contiguous(), "gibbs: v_out u8 [N,D]")
    if row_ids is not None:
        _req(row_ids.dtype == torch.int32 and row_ids.numel() == N, "gibbs: row_ids int32 [N]")
    if given is not None:
        _req(given.dtype == torch.uint8 and given.dim() == 2 and tuple(given.shape) == (N, D) and given.stride(1) == 1
             and (given.stride(0) >= D or N == 1) and given.device == v0.device, "gibbs: given u8 [N, D], unit column stride, row stride >= D")
        _req(seed_step is None, "gibbs: given with seed_step (the stepped chain is training's, unconditioned)")
    temperature = _rbm_temperature(temperature, "gibbs")
    _req(temperature == 1.0 or seed_step is None, "gibbs: a temperature with seed_step (the stepped chain is training's, untempered)")
    ws = rbm_workspace(D, Hn, v0.device)
    _req(sub_base is None or seed_step is None, "gibbs: sub_base with seed_step (the stepped chain is training's)")
    if seed_step is not None:
        _req(seed_step.dtype == torch.int32 and seed_step.numel() == 1, "gibbs: seed_step int32 [1]")
        call("mnn_rbm_gibbs_stepped", _stream(), N, D, Hn, int(k), _ptr(v0), _ptr(W), _ptr(bh), _ldb(bh, Hn), _ptr(bv), _ldb(bv, D), int(seed),
             int(row0), _ptr(row_ids), int(sub0), _ptr(p_v), _ptr(v_out), _ptr(ws), _ptr(seed_step))
        return
    ld_given = 0 if given is None else (given.stride(0) if N > 1 else D)
    if sub_base is not None:
        call("mnn_rbm_gibbs_at", _stream(), N, D, Hn, int(k), _ptr(v0), _ptr(W), _ptr(bh), _ldb(bh, Hn), _ptr(bv), _ldb(bv, D), int(seed), int(row0),
             _ptr(row_ids), int(sub0), _ptr(p_v), _ptr(v_out), _ptr(ws), _ptr(given), ld_given, temperature, _sub_base(sub_base, v0, "gibbs"))
        return
    if temperature != 1.0:
        call("mnn_rbm_gibbs_temp", _stream(), N, D, Hn, int(k), _ptr(v0), _ptr(W), _ptr(bh), _ldb(bh, Hn), _ptr(bv), _ldb(bv, D), int(seed), int(row0),
             _ptr(row_ids), int(sub0), _ptr(p_v), _ptr(v_out), _ptr(ws), _ptr(given), ld_given, temperature)
        return
    call("mnn_rbm_gibbs", _stream(), N, D, Hn, int(k), _ptr(v0), _ptr(W), _ptr(bh), _ldb(bh, Hn), _ptr(bv), _ldb(bv, D), int(seed), int(row0),
         _ptr(row_ids), int(sub0), _ptr(p_v), _ptr(v_out), _ptr(ws), _ptr(given), ld_given)


def _check_ladder(betas, what="rbm_ais"):
    """The AIS ladder: a float32 device vector, finite, non-decreasing, from exactly 0 to exactly 1, at least two values."""
    _req(isinstance(betas, torch.Tensor) and betas.dtype == torch.float32 and betas.dim() == 1 and betas.is_contiguous(), what + ": betas f32 [L]")
    _req(betas.numel() >= 2, what + ": the ladder needs at least two values (0 and 1)")
    b = betas.detach().to("cpu", copy=True).double()        # a host copy: the ladder is validated before anything runs
    _req(bool(torch.isfinite(b).all()), what + ": betas must be finite")
    _req(bool((b[1:] >= b[:-1]).all()), what + ": betas must be non-decreasing")
    _req(float(b[0]) == 0.0 and float(b[-1]) == 1.0, what + ": the ladder must start at 0 and end at 1")


def _rbm_anneal(what, W, bh, bv, v, betas, num_chains, seed, row0, row_ids, log_z, log_w, v_out, stats, given=None):
    """rbm_ais (v is None) and rbm_raise (v: the rows' data vectors): one set of checks, all before any allocation, and the call.
    given (optional): the rows' codes -- the clamped estimators' entries; None reaches mnn_rbm_ais / mnn_rbm_raise themselves."""
    D, Hn = W.shape
    _req(W.dtype == torch.float32 and W.dim() == 2 and W.is_contiguous(), what + ": W f32 [D,Hn]")
    N = max(bh.shape[0], bv.shape[0], 0 if log_z is None else log_z.shape[0], 0 if row_ids is None else row_ids.numel(),
            v.shape[0] if isinstance(v, torch.Tensor) and v.dim() == 2 else 0,
            given.shape[0] if isinstance(given, torch.Tensor) and given.dim() == 2 else 0)
    _req(bh.dim() == 2 and bv.dim() == 2 and bh.shape[0] in (1, N) and bv.shape[0] in (1, N), what + ": bias rows must be 1 or N")
    _ldb(bh, Hn), _ldb(bv, D)
    if what == "rbm_raise":
        _req(isinstance(v, torch.Tensor) and v.dtype == torch.uint8 and tuple(v.shape) == (N, D) and v.is_contiguous(),
             what + ": v u8 [N, D] (one data vector per row)")
    if given is not None:
        _req(isinstance(given, torch.Tensor) and given.dtype == torch.uint8 and given.dim() == 2 and tuple(given.shape) == (N, D)
             and given.stride(1) == 1 and (given.stride(0) >= D or N == 1),
             what + ": given u8 [N, D] codes (0 / 1 clamp, 255 free), unit column stride, row stride ld_given >= D")
    S = int(num_chains)
    _req(S >= 1, what + ": num_chains >= 1")
    _check_ladder(betas, what)
    L = betas.numel()
    _req(S * L < 2 ** 32, what + ": num_chains * len(betas) must be < 2^32 (the 32-bit sub counter)")
    if row_ids is not None:
        _req(row_ids.dtype == torch.int32 and row_ids.numel() == N and row_ids.is_contiguous(), what + ": row_ids int32 [N]")
    dev = W.device
    for t in (bh, bv, betas, row_ids, v, given):
        _req(t is None or t.device == dev, what + ": every operand on W's device")
    for t, shape, dt, name in ((log_z, (N,), torch.float32, "log_z f32 [N]"), (log_w, (N, S), torch.float32, "log_w f32 [N, S]"),
                               (v_out, (N, S, D), torch.uint8, "v_out u8 [N, S, D]"), (stats, (N, 2), torch.float32, "stats f32 [N, 2]")):
        if t is not None:
            _req(t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev, what + ": " + name)
    _ptr(W)                                                          # no CPU path: refuse host tensors before allocating anything
    if log_z is None:
        log_z = torch.empty(N, device=dev)
    ws = torch.empty(_lib.load().mnn_rbm_ais_workspace_bytes(N, D, Hn, S, L), dtype=torch.uint8, device=dev)
    head = (_stream(), N, D, Hn, S, L, _ptr(betas), _ptr(W), _ptr(bh), _ldb(bh, Hn), _ptr(bv), _ldb(bv, D))
    tail = (int(seed), int(row0), _ptr(row_ids), _ptr(log_z), _ptr(log_w), _ptr(v_out), _ptr(stats), _ptr(ws))
    clamp = () if given is None else (_ptr(given), given.stride(0) if N > 1 else D)
    if v is None:
        call("mnn_rbm_ais" if given is None else "mnn_rbm_ais_given", *head, *tail, *clamp)
    else:
        call("mnn_rbm_raise" if given is None else "mnn_rbm_raise_given", *head, _ptr(v), *tail, *clamp)
    return log_z


def rbm_ais(W, bh, bv, betas, num_chains, seed, row0=0, row_ids=None, log_z=None, log_w=None, v_out=None, stats=None, given=None):
    """Annealed importance sampling of log Z for each bias row (mnn_rbm_ais): N rows (the most of: bias rows, log_z, row_ids), bh and bv
    have 1 or N rows (one row: shared by all N, whose chains differ by their row ids).  betas: the
    ladder, f32 device [L] (0 = b_0 <= ... <= b_{L-1} = 1).  Returns log_z f32 [N] (allocated if not given); optional outputs: log_w f32
    [N, S], v_out u8 [N, S, D] final chain states, stats f32 [N, 2] = (effective sample size, standard error of log_z).  log Z^ is biased low.
    given (optional; mnn_rbm_ais_given, DESIGN.md section 4 "Clamped AIS"): codes u8 [N, D] (row stride >= D) as rbm_gibbs takes them -- 0 / 1
    clamp the visible, 255 leaves it free (common.given_codes).  log_z is then the log of the sum over the vectors that agree with the
    clamped cells, so free_energy(v) + log_z = -log p(v_free | v_clamped); all codes 255 gives the bits of the call without `given`."""
    return _rbm_anneal("rbm_ais", W, bh, bv, None, betas, num_chains, seed, row0, row_ids, log_z, log_w, v_out, stats, given)


def rbm_raise(W, bh, bv, v, betas, num_chains, seed, row0=0, row_ids=None, log_z=None, log_w=None, v_out=None, stats=None):
    """Reverse annealed importance sampling (mnn_rbm_raise; RAISE, Burda et al. 2015): rbm_ais's ladder run downwards from the rows' data
    vectors v u8 [N, D], S chains per row on Philox streams 8 / 9.  Operands, checks and outputs as rbm_ais; log_z = log Z_0 - (logsumexp_c
    log w_c - log S) is biased the other way from rbm_ais's: high in expectation over model-distributed data and, with a long enough
    ladder, an upper end to rbm_ais's lower one -- not a bound per row."""
    return _rbm_anneal("rbm_raise", W, bh, bv, v, betas, num_chains, seed, row0, row_ids, log_z, log_w, v_out, stats)


def rbm_raise_given(W, bh, bv, v, given, betas, num_chains, seed, row0=0, row_ids=None, log_z=None, log_w=None, v_out=None, stats=None):
    """rbm_raise with codes (mnn_rbm_raise_given; rbm_raise's own parameter list is fixed): given u8 [N, D] as rbm_ais takes them, or None =
    rbm_raise.  The chains start from v with every clamped cell at its code and hold it there; log_z estimates rbm_ais(given=)'s clamped
    log Z from the other side, with rbm_raise's statements about its bias and no more."""
    return _rbm_anneal("rbm_raise", W, bh, bv, v, betas, num_chains, seed, row0, row_ids, log_z, log_w, v_out, stats, given)


def rbm_hidden(v, W, bh, stream_id, seed, row0, sub, p_h=None, h=None):
    N, D = v.shape
    Hn = W.shape[1]
    _req(v.dtype in (torch.uint8, torch.float32) and v.is_contiguous() and W.shape == (D, Hn) and W.is_contiguous(), "rbm_hidden: shapes")
    _req(bh.shape[0] in (1, N), "rbm_hidden: bias rows")
    for t, dt in ((p_h, torch.float32), (h, torch.uint8)):
        if t is not None:
            _req(t.dtype == dt and t.shape == (N, Hn) and t.is_contiguous(), "rbm_hidden: outputs [N,Hn]")
    call("mnn_rbm_hidden", _stream(), N, D, Hn, _ptr(v), dtype_code(v), _ptr(W), _ptr(bh), _ldb(bh, Hn), int(stream_id), int(seed), int(row0),
         int(sub), _ptr(p_h), _ptr(h))


def rbm_visible(h, W, bv, stream_id, seed, row0, sub, p_v=None, v=None):
    N, Hn = h.shape
    D = W.shape[0]
    _req(h.dtype in (torch.uint8, torch.float32) and h.is_contiguous() and W.shape == (D, Hn) and W.is_contiguous(), "rbm_visible: shapes")
    _req(bv.shape[0] in (1, N), "rbm_visible: bias rows")
    for t, dt in ((p_v, torch.float32), (v, torch.uint8)):
        if t is not None:
            _req(t.dtype == dt and t.shape == (N, D) and t.is_contiguous(), "rbm_visible: outputs [N,D]")
    ws = rbm_workspace(D, Hn, h.device)
    call("mnn_rbm_visible", _stream(), N, D, Hn, _ptr(h), dtype_code(h), _ptr(W), _ptr(bv), _ldb(bv, D), int(stream_id), int(seed), int(row0),
         int(sub), _ptr(p_v), _ptr(v), _ptr(ws))


def rbm_free_energy(v, W, bh, bv, F, p_h=None):
    """p_h (optional, f32 [N, Hn]): also receives sigmoid(v W + bh) -- the hidden activations the free-energy gradient needs."""
    N, D = v.shape
    Hn = W.shape[1]
    _req(p_h is None or (p_h.dtype == torch.float32 and p_h.is_contiguous() and tuple(p_h.shape) == (N, Hn)), "free_energy: p_h f32 [N, Hn]")
    _req(v.dtype == torch.uint8 and v.is_contiguous() and W.shape == (D, Hn) and W.is_contiguous(), "free_energy: shapes")
    _req(F.dtype == torch.float32 and F.numel() == N, "free_energy: F f32 [N]")
    _req(bh.shape[0] in (1, N) and bv.shape[0] in (1, N), "free_energy: bias rows")
    call("mnn_rbm_free_energy", _stream(), N, D, Hn, _ptr(v), _ptr(W), _ptr(bh), _ldb(bh, Hn), _ptr(bv), _ldb(bv, D), _ptr(F), _ptr(p_h))
    return F


RBM_MULTI_MAX_JOBS = 8


def _multi_bias_ld(jobs, key, n, N, what):
    """The jobs' bias blocks share one leading dimension: all broadcast rows (0) or rows of one stride (slices of one Dense-output block)."""
    lds = set()
    for j in jobs:
        b = j[key]
        _req(torch.is_tensor(b) and b.dim() == 2 and b.shape[0] in (1, N), f"{what}: {key} rows must be 1 or N")
        lds.add(_ldb(b, n))
    _req(len(lds) == 1, f"{what}: the jobs' {key} must share one leading dimension")
    return lds.pop()


def rbm_gibbs_multi(jobs, k, row0=0, row_ids=None, sub0=0, seed_step=None, temperature=1.0, sub_base=None):
    """ops.rbm_gibbs for 1..8 RBMs of one shape in ONE launch (mnn_rbm_gibbs_multi).  job = dict(v0 = a u8 [N, D] VIEW (any row / column
    strides, the same for every job: e.g. x[:, m::M] of a composer-layout [N, D * M] block, or a contiguous plane), W f32 [D, Hn], bh / bv
    f32 [N or 1, >= Hn / D] (slices of one block: one leading dimension), seed, p_v f32 [N, D] / v_out u8 [N, D] views or None (the element
    strides of v0), given = None or a u8 [N, D] view of codes with v0's column stride (set on every job or on none; not with seed_step)).
    temperature: a positive float or one per job (not with seed_step); all of them 1 is the untempered launch.
    sub_base: ops.rbm_gibbs's, shared by the jobs (mnn_rbm_gibbs_multi_at).
    Per job the results are bit for bit those of ops.rbm_gibbs (at the job's temperature) on contiguous copies."""
    _req(isinstance(jobs, (list, tuple)) and 1 <= len(jobs) <= RBM_MULTI_MAX_JOBS, f"gibbs_multi: 1..{RBM_MULTI_MAX_JOBS} jobs")
    if isinstance(temperature, (int, float)):
        temperature = (temperature,) * len(jobs)
    _req(isinstance(temperature, (list, tuple)), "gibbs_multi: the temperature is a positive finite number, or one per job")
    temps = tuple(_rbm_temperature(t, "gibbs_multi") for t in temperature)
    _req(len(temps) == len(jobs), "gibbs_multi: one temperature, or one per job")
    tempered = any(t != 1.0 for t in temps)
    _req(not (tempered and seed_step is not None), "gibbs_multi: a temperature with seed_step (the stepped chain is training's, untempered)")
    v0 = jobs[0]["v0"]
    _req(torch.is_tensor(v0) and v0.dim() == 2, "gibbs_multi: v0 u8 [N, D] views")
    N, D = v0.shape
    W0 = jobs[0]["W"]
    _req(torch.is_tensor(W0) and W0.dim() == 2 and W0.shape[0] == D, "gibbs_multi: W f32 [D, Hn]")
    Hn = W0.shape[1]
    rs, es = v0.stride()
    _req(es >= 1 and (N == 1 or rs >= (D - 1) * es + 1), "gibbs_multi: v0 needs a positive column stride and rows that do not overlap")
    has_given = jobs[0].get("given") is not None
    rs_g = jobs[0]["given"].stride(0) if has_given else 0
    same_strides = lambda t: t.stride(1) == es and (N == 1 or t.stride(0) == rs)      # (one row: its stride is never multiplied by a row index)
    _req(not (has_given and seed_step is not None), "gibbs_multi: given with seed_step (the stepped chain is training's, unconditioned)")
    for j in jobs:
        v, W = j["v0"], j["W"]
        _req(torch.is_tensor(v) and v.dtype == torch.uint8 and tuple(v.shape) == (N, D) and same_strides(v) and v.device == v0.device,
             "gibbs_multi: v0 u8 [N, D] views of equal shape and strides")
        _req(torch.is_tensor(W) and W.dtype == torch.float32 and tuple(W.shape) == (D, Hn) and W.is_contiguous(), "gibbs_multi: W f32 [D, Hn], one shape for every job")
        for t, dt, what in ((j.get("p_v"), torch.float32, "p_v f32"), (j.get("v_out"), torch.uint8, "v_out u8")):
            _req(t is None or (t.dtype == dt and tuple(t.shape) == (N, D) and same_strides(t)), f"gibbs_multi: {what} [N, D] with the strides of v0")
        g = j.get("given")
        _req((g is not None) == has_given, "gibbs_multi: given on every job or on none")
        _req(g is None or (g.dtype == torch.uint8 and tuple(g.shape) == (N, D) and g.stride(1) == es and g.stride(0) == rs_g
                           and (N == 1 or rs_g >= (D - 1) * es + 1) and g.device == v0.device),
             "gibbs_multi: given u8 [N, D] views with v0's column stride and one row stride")
    ld_bh = _multi_bias_ld(jobs, "bh", Hn, N, "gibbs_multi")
    ld_bv = _multi_bias_ld(jobs, "bv", D, N, "gibbs_multi")
    if row_ids is not None:
        _req(row_ids.dtype == torch.int32 and row_ids.numel() == N, "gibbs_multi: row_ids int32 [N]")
    if seed_step is not None:
        _req(seed_step.dtype == torch.int32 and seed_step.numel() == 1, "gibbs_multi: seed_step int32 [1]")
    arr = (_lib.RbmGibbsJob * len(jobs))()
    for a, j in zip(arr, jobs):
        a.W, a.bh, a.bv, a.seed, a.v0 = _ptr(j["W"]), _ptr(j["bh"]), _ptr(j["bv"]), int(j["seed"]), _ptr(j["v0"])
        a.p_v, a.v_out, a.given = _ptr(j.get("p_v")), _ptr(j.get("v_out")), _ptr(j.get("given"))
    ws = torch.empty(len(jobs) * _lib.load().mnn_rbm_workspace_bytes(D, Hn), dtype=torch.uint8, device=v0.device)
    tail = (rs if N > 1 else max(rs, (D - 1) * es + 1), es, rs_g if N > 1 else max(rs_g, (D - 1) * es + 1), _ptr(ws))
    if sub_base is not None:
        call("mnn_rbm_gibbs_multi_at", _stream(), len(jobs), arr, N, D, Hn, int(k), ld_bh, ld_bv, int(row0), _ptr(row_ids), int(sub0),
             _ptr(seed_step), *tail, (C.c_float * len(jobs))(*temps) if tempered else None, _sub_base(sub_base, v0, "gibbs_multi"))
        return
    if tempered:
        call("mnn_rbm_gibbs_multi_temps", _stream(), len(jobs), arr, N, D, Hn, int(k), ld_bh, ld_bv, int(row0), _ptr(row_ids), int(sub0),
             _ptr(seed_step), *tail, (C.c_float * len(jobs))(*temps))
        return
    call("mnn_rbm_gibbs_multi", _stream(), len(jobs), arr, N, D, Hn, int(k), ld_bh, ld_bv, int(row0), _ptr(row_ids), int(sub0), _ptr(seed_step), *tail)


def rbm_free_energy_multi(jobs):
    """ops.rbm_free_energy for 1..8 RBMs of one shape in ONE launch (mnn_rbm_free_energy_multi).  job = dict(v u8 [N, D], W f32 [D, Hn],
    bh / bv f32 [N or 1, .] (one leading dimension over the jobs), F f32 [N], p_h = None or f32 [N, Hn])."""
    _req(isinstance(jobs, (list, tuple)) and 1 <= len(jobs) <= RBM_MULTI_MAX_JOBS, f"free_energy_multi: 1..{RBM_MULTI_MAX_JOBS} jobs")
    v0 = jobs[0]["v"]
    _req(torch.is_tensor(v0) and v0.dim() == 2, "free_energy_multi: v u8 [N, D]")
    N, D = v0.shape
    W0 = jobs[0]["W"]
    _req(torch.is_tensor(W0) and W0.dim() == 2 and W0.shape[0] == D, "free_energy_multi: W f32 [D, Hn]")
    Hn = W0.shape[1]
    for j in jobs:
        v, W, F, p_h = j["v"], j["W"], j["F"], j.get("p_h")
        _req(torch.is_tensor(v) and v.dtype == torch.uint8 and tuple(v.shape) == (N, D) and v.is_contiguous() and v.device == v0.device,
             "free_energy_multi: v u8 [N, D], one shape for every job")
        _req(torch.is_tensor(W) and W.dtype == torch.float32 and tuple(W.shape) == (D, Hn) and W.is_contiguous(), "free_energy_multi: W f32 [D, Hn], one shape for every job")
        _req(torch.is_tensor(F) and F.dtype == torch.float32 and F.numel() == N and F.is_contiguous(), "free_energy_multi: F f32 [N]")
        _req(p_h is None or (p_h.dtype == torch.float32 and p_h.is_contiguous() and tuple(p_h.shape) == (N, Hn)), "free_energy_multi: p_h f32 [N, Hn]")
    ld_bh = _multi_bias_ld(jobs, "bh", Hn, N, "free_energy_multi")
    ld_bv = _multi_bias_ld(jobs, "bv", D, N, "free_energy_multi")
    arr = (_lib.RbmFreeEnergyJob * len(jobs))()
    for a, j in zip(arr, jobs):
        a.v, a.W, a.bh, a.bv, a.F, a.p_h = _ptr(j["v"]), _ptr(j["W"]), _ptr(j["bh"]), _ptr(j["bv"]), _ptr(j["F"]), _ptr(j.get("p_h"))
    call("mnn_rbm_free_energy_multi", _stream(), len(jobs), arr, N, D, Hn, ld_bh, ld_bv)


def rbm_cd_bias_delta(v, p_v, h, p_h, scale, dbv, dbh):
    """dbv += scale * colsum(v - p_v), dbh += scale * colsum(h - p_h) (rbm.py:318-327); v/h u8, p_* f32, outputs f32 (zeroed by the caller)."""
    N, D = v.shape
    Hn = h.shape[1]
    _req(v.dtype == torch.uint8 and h.dtype == torch.uint8 and v.is_contiguous() and h.is_contiguous() and h.shape[0] == N, "cd_bias_delta: v/h u8 [N,.]")
    _req(p_v.dtype == torch.float32 and p_v.shape == (N, D) and p_v.is_contiguous() and p_h.dtype == torch.float32 and p_h.shape == (N, Hn)
         and p_h.is_contiguous(), "cd_bias_delta: p_v / p_h f32 [N,.]")
    _req(dbv.dtype == torch.float32 and dbv.numel() == D and dbv.is_contiguous() and dbh.dtype == torch.float32 and dbh.numel() == Hn
         and dbh.is_contiguous(), "cd_bias_delta: outputs f32 [D] / [Hn]")
    call("mnn_rbm_cd_bias_delta", _stream(), N, D, Hn, _ptr(v), _ptr(p_v), _ptr(h), _ptr(p_h), float(scale), _ptr(dbv), _ptr(dbh))


def sigmoid_grad(dy, y, dz):
    """dz = dy * y * (1 - y) (f32, same shapes; dz may alias dy)."""
    n = y.numel()
    for t in (dy, y, dz):
        _req(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, "sigmoid_grad: contiguous f32 buffers of equal size")
    call("mnn_sigmoid_grad_f32", _stream(), n, _ptr(dy), _ptr(y), _ptr(dz))
    return dz


def rbm_cd_rows(v, v_s, sv, ss, rw, scale, d_out, pos, neg):
    """Rows of the LSTM-RBM cost gradient: d_out[:, :Hn] = w (ss - sv), d_out[:, Hn:Hn+D] = w (v_s - v), padding zeroed; pos = w ss, neg = -w sv
    (w = rw * scale).  v / v_s u8 [N,D], sv / ss f32 [N,Hn], d_out f32 [N, ld >= Hn + D] (rnn_rbm.py:113-126, rbm.py:229)."""
    N, D = v.shape
    Hn = sv.shape[1]
    _req(v.dtype == torch.uint8 and v_s.dtype == torch.uint8 and v.is_contiguous() and v_s.is_contiguous() and v_s.shape == (N, D), "cd_rows: v / v_s u8 [N,D]")
    for t in (sv, ss, pos, neg):
        _req(t.dtype == torch.float32 and t.shape == (N, Hn) and t.is_contiguous(), "cd_rows: sv / ss / pos / neg f32 [N,Hn]")
    _req(rw.dtype == torch.float32 and rw.numel() == N and rw.is_contiguous(), "cd_rows: row weights f32 [N]")
    _req(d_out.dtype == torch.float32 and d_out.dim() == 2 and d_out.shape[0] == N and d_out.is_contiguous() and d_out.shape[1] >= Hn + D, "cd_rows: d_out f32 [N, ld]")
    call("mnn_rbm_cd_rows", _stream(), N, D, Hn, d_out.shape[1], _ptr(v), _ptr(v_s), _ptr(sv), _ptr(ss), _ptr(rw), float(scale), _ptr(d_out), _ptr(pos), _ptr(neg))


def rbm_visible_bias_init(colsum, count, bv):
    """bv[d] = log(1e-6 + p/(1-p)), p = colsum[d]/count (rbm.py:286-297)."""
    D = colsum.numel()
    _req(colsum.dtype == torch.float32 and colsum.is_contiguous() and bv.dtype == torch.float32 and bv.numel() == D and bv.is_contiguous(),
         "visible_bias_init: f32 [D] buffers")
    call("mnn_rbm_visible_bias_init", _stream(), D, _ptr(colsum), float(count), _ptr(bv))


def axpby(a, x, b, y, out):
    """out = a*x + b*y over flat f32 buffers (out may alias x or y; y None with b == 0)."""
    n = x.numel()
    for t in (x, out) + (() if y is None else (y,)):
        _req(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, "axpby: contiguous f32 buffers of equal size")
    _req(y is not None or b == 0, "axpby: y missing")
    call("mnn_axpby_f32", _stream(), n, float(a), _ptr(x), float(b), _ptr(y), _ptr(out))
    return out


# ------------------------------------------------------------------------------------------------
def sumsq(x, out):
    _req(x.dtype == torch.float32 and x.is_contiguous() and out.dtype == torch.float32, "sumsq: f32")
    call("mnn_sumsq", _stream(), _ptr(x), x.numel(), _ptr(out))


def weighted_sum(x, w, out):
    _req(x.dtype == torch.float32 and x.is_contiguous() and (w is None or (w.numel() == x.numel() and w.dtype == torch.float32)), "weighted_sum")
    call("mnn_weighted_sum", _stream(), _ptr(x), _ptr(w), x.numel(), _ptr(out))


def clip_adam_step(theta, grad, m, v, sumsq_buf, clip_norm, lr, beta1, beta2, eps, step, sgd=False, step_dev=None, skipped=None):
    n = theta.numel()
    for t in (theta, grad) + (() if sgd else (m, v)):
        _req(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, "adam: flat f32 buffers of equal size")
    call("mnn_clip_adam_step", _stream(), _ptr(theta), _ptr(grad), _ptr(m), _ptr(v), n, _ptr(sumsq_buf), float(clip_norm), float(lr),
         float(beta1), float(beta2), float(eps), int(step), _ptr(step_dev), int(sgd), _ptr(skipped))


def step_increment(step_dev, sumsq_buf=None, clip_norm=0.0, ls_dyn=None, ls_good=None, grow_after=200):
    """Advance the device step counter -- unless (sumsq_buf, clip_norm) say that clip_adam_step skipped this step (non-finite norm).
    ls_dyn f32 [m, 1/m] + ls_good int32[1]: the dynamic part of the f16 loss scale follows the outcome (halved by a skipped step, doubled
    back up to 1 after `grow_after` applied steps in a row)."""
    _step_ok(step_dev)
    _req((ls_dyn is None) == (ls_good is None), "step_increment: ls_dyn and ls_good come together")
    if ls_dyn is not None:
        _req(ls_dyn.dtype == torch.float32 and ls_dyn.numel() == 2 and ls_dyn.is_contiguous() and ls_good.dtype == torch.int32 and ls_good.numel() == 1,
             "step_increment: ls_dyn f32[2], ls_good int32[1]")
    call("mnn_step_increment", _stream(), _ptr(step_dev), _ptr(sumsq_buf), float(clip_norm), _ptr(ls_dyn), _ptr(ls_good), int(grow_after))


OPT_MULTI_MAX_JOBS = _lib.OPT_MULTI_MAX_JOBS


class OptJobTables:
    """The mnn_opt_job tables of a job list, validated and built ONCE (at most OPT_MULTI_MAX_JOBS jobs per table): what the three grouped
    optimiser ops launch from.  Holds the jobs, so the tensors behind the pointers live as long as the tables."""

    def __init__(self, jobs, sgd=False, who="opt_job_tables"):
        _req(isinstance(jobs, (list, tuple)) and len(jobs) >= 1, f"{who}: a non-empty list of jobs")
        for j in jobs:
            n = j["theta"].numel()
            for t in (j["theta"], j["grad"]) + (() if sgd else (j["m"], j["v"])):
                _req(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and n > 0, f"{who}: flat f32 buffers of equal size per job")
            _req(j.get("step_dev") is not None, f"{who}: step_dev is required")
            _step_ok(j["step_dev"])
            sk, ld, lg = j.get("skipped"), j.get("ls_dyn"), j.get("ls_good")
            _req(sk is None or (sk.dtype == torch.int32 and sk.numel() == 1), f"{who}: skipped int32[1]")
            _req((ld is None) == (lg is None), f"{who}: ls_dyn and ls_good come together")
            _req(ld is None or (ld.dtype == torch.float32 and ld.numel() == 2 and ld.is_contiguous() and lg.dtype == torch.int32 and lg.numel() == 1),
                 f"{who}: ls_dyn f32[2], ls_good int32[1]")
        self.jobs, self.sgd, self.tables = list(jobs), bool(sgd), []
        for c in range(0, len(jobs), OPT_MULTI_MAX_JOBS):
            chunk = jobs[c:c + OPT_MULTI_MAX_JOBS]
            arr = (_lib.OptJob * len(chunk))()
            for a, j in zip(arr, chunk):
                a.theta, a.grad, a.m, a.v, a.n = _ptr(j["theta"]), _ptr(j["grad"]), _ptr(j.get("m")), _ptr(j.get("v")), j["theta"].numel()
                a.step_dev, a.skipped, a.ls_dyn, a.ls_good = _ptr(j["step_dev"]), _ptr(j.get("skipped")), _ptr(j.get("ls_dyn")), _ptr(j.get("ls_good"))
            self.tables.append(arr)


def opt_job_tables(jobs, sgd=False):
    """Prepare a job list for sumsq_multi / clip_adam_step_multi / step_increment_multi, which take the result in place of the list: a step
    that calls all three validates and builds the tables once.  job = dict(theta, grad, m, v: flat f32 of one size (m, v None with sgd);
    step_dev int32 [1]; skipped int32 [1] or None; ls_dyn f32 [2] + ls_good int32 [1] or both None).  sgd: m and v are not asked for (the
    tables then serve clip_adam_step_multi(sgd=True) only)."""
    return OptJobTables(jobs, sgd)


def _opt_tables(jobs, sgd, who):
    if isinstance(jobs, OptJobTables):
        _req(sgd or not jobs.sgd, f"{who}: these tables were prepared for sgd (no m, v)")
        return jobs.tables
    return OptJobTables(jobs, sgd, who).tables


def sumsq_multi(jobs, out):
    """out[0] += sum over the jobs of sum(grad^2): ops.sumsq of every job's gradient in one launch per 16 jobs (mnn_sumsq_multi).
    jobs: a list of job dicts, or opt_job_tables(jobs)."""
    _req(out.dtype == torch.float32 and out.numel() >= 1, "sumsq_multi: out f32")
    for arr in _opt_tables(jobs, True, "sumsq_multi"):
        call("mnn_sumsq_multi", _stream(), len(arr), arr, _ptr(out))


def clip_adam_step_multi(jobs, sumsq_buf, clip_norm, lr, beta1, beta2, eps, sgd=False):
    """ops.clip_adam_step (its step_dev form) of every job behind the one norm word sumsq_buf, in one launch per 16 jobs
    (mnn_clip_adam_step_multi): bit for bit the per-job calls.  jobs: a list of job dicts, or opt_job_tables(jobs)."""
    for arr in _opt_tables(jobs, sgd, "clip_adam_step_multi"):
        call("mnn_clip_adam_step_multi", _stream(), len(arr), arr, _ptr(sumsq_buf), float(clip_norm), float(lr), float(beta1), float(beta2),
             float(eps), int(sgd))


def step_increment_multi(jobs, sumsq_buf=None, clip_norm=0.0, grow_after=200):
    """ops.step_increment of every job's step_dev (and ls_dyn / ls_good where the job has them) in one launch per 16 jobs.
    jobs: a list of job dicts, or opt_job_tables(jobs)."""
    for arr in _opt_tables(jobs, True, "step_increment_multi"):
        call("mnn_step_increment_multi", _stream(), len(arr), arr, _ptr(sumsq_buf), float(clip_norm), int(grow_after))


def segments_copy(segs):
    """dst[:n] = src[:n] for a list of (src, dst, n) over flat f32 tensors, one launch per 16 segments (mnn_segments_copy)."""
    _req(isinstance(segs, (list, tuple)) and len(segs) >= 1, "segments_copy: a non-empty list of (src, dst, n)")
    for src, dst, n in segs:
        for t in (src, dst):
            _req(t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n > 0, "segments_copy: contiguous f32 buffers of at least n > 0 words")
    for c in range(0, len(segs), OPT_MULTI_MAX_JOBS):
        chunk = segs[c:c + OPT_MULTI_MAX_JOBS]
        arr = (_lib.CopySeg * len(chunk))()
        for a, (src, dst, n) in zip(arr, chunk):
            a.src, a.dst, a.n = _ptr(src), _ptr(dst), int(n)
        call("mnn_segments_copy", _stream(), len(arr), arr)


def bias_grad(dY, db, accumulate=False):
    _rowmajor(dY, "bias_grad dY")
    _req(dY.dtype == torch.float32 and db.dtype == torch.float32 and db.numel() == dY.shape[1] and db.is_contiguous(), "bias_grad: shapes")
    call("mnn_bias_grad", _stream(), _ptr(dY), dY.shape[0], dY.shape[1], dY.stride(0), _ptr(db), int(accumulate))


def grad_rows_fanout(dY, cols_t, out_c, out_t, db):
    """One pass over dY f32 [rows, cols_c]: out_c = bf16 copy, out_t[:cols_t, :rows] = bf16 transpose, db[:cols_t] += column sums."""
    _rowmajor(dY, "fanout dY"); _rowmajor(out_c, "fanout out_c"); _rowmajor(out_t, "fanout out_t")
    rows, cols_c = dY.shape
    _req(dY.dtype == torch.float32 and out_c.dtype in H16 and out_t.dtype == out_c.dtype and db.dtype == torch.float32,
         "fanout: dY/db f32, outputs bf16 / f16")
    _req(out_c.shape == dY.shape and out_t.shape[0] == cols_t and out_t.shape[1] >= rows and 0 < cols_t <= cols_c and db.numel() == cols_t
         and db.is_contiguous(), "fanout: shapes")
    call("mnn_grad_rows_fanout", _stream(), _ptr(dY), rows, cols_c, cols_t, dY.stride(0), _ptr(out_c), out_c.stride(0), _ptr(out_t),
         out_t.stride(0), _ptr(db), dtype_code(out_c))


def fill(x, value):
    _req(x.dtype == torch.float32 and x.is_contiguous(), "fill: f32 contiguous")
    call("mnn_fill_f32", _stream(), _ptr(x), x.numel(), float(value))


# ------------------------------------------------------------------------------------------------
def musical_bar_stats(x, poly_threshold, pattern_class, notes, used_pitches, used_classes, poly_steps, pat_on, pat_tol, beat_chroma):
    """x u8 [B,bars,steps,P,M]; int32 outputs [B*bars, M], beat_chroma int32 [B*bars,4,12,M] (metrics/musical.py)."""
    _req(x.dtype == torch.uint8 and x.dim() == 5 and x.is_contiguous(), "musical_bar_stats: x u8 [B,bars,steps,P,M]")
    B, bars, steps, P, M = x.shape
    for t in (notes, used_pitches, used_classes, poly_steps, pat_on, pat_tol):
        _req(t.dtype == torch.int32 and t.numel() == B * bars * M and t.is_contiguous(), "musical_bar_stats: int32 [B*bars, M] outputs")
    _req(beat_chroma.dtype == torch.int32 and beat_chroma.numel() == B * bars * 48 * M and beat_chroma.is_contiguous(), "musical_bar_stats: beat_chroma")
    _req(pattern_class is None or (pattern_class.dtype == torch.uint8 and pattern_class.numel() == steps), "musical_bar_stats: pattern_class u8 [steps]")
    call("mnn_musical_bar_stats", _stream(), _ptr(x), B * bars, steps, P, M, int(poly_threshold), _ptr(pattern_class), _ptr(notes), _ptr(used_pitches),
         _ptr(used_classes), _ptr(poly_steps), _ptr(pat_on), _ptr(pat_tol), _ptr(beat_chroma))


def musical_note_stats(x, threshold, onsets, qualified):
    """x u8 [B,T,P,M]; onsets / qualified int32 [M], accumulated (zero them first)."""
    _req(x.dtype == torch.uint8 and x.dim() == 4 and x.is_contiguous(), "musical_note_stats: x u8 [B,T,P,M]")
    B, T, P, M = x.shape
    for t in (onsets, qualified):
        _req(t.dtype == torch.int32 and t.numel() == M, "musical_note_stats: int32 [M] outputs")
    call("mnn_musical_note_stats", _stream(), _ptr(x), B, T, P, M, int(threshold), _ptr(onsets), _ptr(qualified))


def eval_counts(targets, predictions, counts):
    """counts int64 [4] += (tp, fp, fn, equal) over all cells of targets / predictions (u8, same shape)."""
    _req(targets.dtype == torch.uint8 and predictions.dtype == torch.uint8 and targets.is_contiguous() and predictions.is_contiguous()
         and targets.numel() == predictions.numel(), "eval_counts: targets / predictions u8, same size")
    _req(counts.dtype == torch.int64 and counts.numel() == 4, "eval_counts: counts int64 [4]")
    call("mnn_eval_counts", _stream(), _ptr(targets), _ptr(predictions), targets.numel(), _ptr(counts))


def log_loss_rows(targets, probs, out):
    """out[row] = sum_d tf.losses.log_loss(targets, probs) (epsilon 1e-7); targets u8 [N,D], probs f32 [N,D] (row stride >= D)."""
    N, D = targets.shape
    _req(targets.dtype == torch.uint8 and targets.is_contiguous(), "log_loss_rows: targets u8 [N,D]")
    _req(probs.dtype == torch.float32 and probs.shape == (N, D) and probs.stride(1) == 1, "log_loss_rows: probs f32 [N,D]")
    _req(out.dtype == torch.float32 and out.numel() == N and out.is_contiguous(), "log_loss_rows: out f32 [N]")
    call("mnn_log_loss_rows", _stream(), _ptr(targets), _ptr(probs), N, D, probs.stride(0), _ptr(out))


# ------------------------------------------------------------------------------------------------
# deterministic f32 single steps of the sampling scan (csrc/det_step.hip)
def _prompt_lengths_dev(lengths, B, device, what):
    """A launch's ragged-prompt lengths: int32 [B], contiguous, on `device` (common.prompt_lengths checks the values, on the host)."""
    _req(torch.is_tensor(lengths) and lengths.dtype == torch.int32 and tuple(lengths.shape) == (B,) and lengths.is_contiguous() and lengths.device == device,
         f"{what}: lengths int32 [B], contiguous, on the device of the call")
    return _ptr(lengths)


def lstm_step_det(jobs, lengths=None, t=0):
    """One LSTMBlockCell step per job, ALL jobs in one launch.  job = dict(x=[B, >= n_x] u8 | f32 (or None), n_x, x2=f32 [B, n_x2] or None,
    h_prev / c_prev f32 [B, u] or None (zero state), W f32 [(n_x + n_x2 + u), 4u] (TF layout), bias f32 [4u], c_out / h_out f32 [B, u]).
    lengths (int32 [B] on the device), t (mnn_lstm_step_det_ragged): step t of ragged prompts -- a row with t >= lengths[row] is frozen,
    its c_out / h_out copies of c_prev / h_prev (zeros without them), every other row the step without the argument, bit for bit."""
    _req(1 <= len(jobs) <= 8, "lstm_step_det: 1..8 jobs")
    arr = (_lib.DetLstmJob * len(jobs))()
    B = jobs[0]["c_out"].shape[0]
    for a, j in zip(arr, jobs):
        u = j["c_out"].shape[1]
        x, x2 = j.get("x"), j.get("x2")
        n_x = int(j.get("n_x", x.shape[1] if x is not None else 0))
        n_x2 = x2.shape[1] if x2 is not None else 0
        W, b = j["W"], j["bias"]
        _req(W.dtype == torch.float32 and W.is_contiguous() and tuple(W.shape) == (n_x + n_x2 + u, 4 * u), f"lstm_step_det: W {tuple(W.shape)} != ({n_x + n_x2 + u}, {4 * u})")
        _req(b.dtype == torch.float32 and b.is_contiguous() and b.numel() == 4 * u, "lstm_step_det: bias f32 [4u]")
        for k in ("c_out", "h_out", "h_prev", "c_prev"):
            st = j.get(k)
            _req(st is None or (st.dtype == torch.float32 and st.is_contiguous() and tuple(st.shape) == (B, u)), f"lstm_step_det: {k} must be contiguous f32 [B, u]")
        if x is not None:         # any 2-D view: element (row, k) at row * stride(0) + k * stride(1) (one track of a [B, P, M] step has stride(1) = M)
            _req(x.dim() == 2 and x.stride(1) >= 1 and x.shape[0] == B and x.shape[1] >= n_x and x.dtype in (torch.uint8, torch.float32),
                 "lstm_step_det: x is a u8 / f32 [B, >= n_x] view")
        if x2 is not None:
            _rowmajor(x2, "lstm_step_det x2")
            _req(x2.shape[0] == B and x2.dtype == torch.float32, "lstm_step_det: x2 is f32 [B, n_x2]")
        a.x, a.x_dtype, a.n_x, a.ld_x = (_ptr(x) if x is not None else None), (dtype_code(x) if x is not None else F32), n_x, (x.stride(0) if x is not None else 0)
        a.es_x = x.stride(1) if x is not None else 1
        a.x2, a.n_x2, a.ld_x2 = (_ptr(x2) if x2 is not None else None), n_x2, (x2.stride(0) if x2 is not None else 0)
        a.h_prev, a.c_prev = _ptr(j.get("h_prev")), _ptr(j.get("c_prev"))
        a.W, a.bias, a.c_out, a.h_out, a.units = _ptr(W), _ptr(b), _ptr(j["c_out"]), _ptr(j["h_out"]), u
        Wp = j.get("Wp")                                     # det_lstm_pack(W, u): the same numbers in the kernel's load order (optional)
        _req(Wp is None or (Wp.dtype == torch.float32 and Wp.is_contiguous() and Wp.numel() * 4 == det_lstm_pack_bytes(n_x + n_x2 + u, u) and Wp.data_ptr() % 16 == 0),
             "lstm_step_det: Wp is det_lstm_pack(W, units)")
        a.Wp = _ptr(Wp)
    if lengths is None:
        return call("mnn_lstm_step_det", _stream(), B, len(jobs), arr)
    _req(isinstance(t, int) and not isinstance(t, bool) and t >= 0, "lstm_step_det: t is a step number")
    call("mnn_lstm_step_det_ragged", _stream(), B, len(jobs), arr, _prompt_lengths_dev(lengths, B, jobs[0]["c_out"].device, "lstm_step_det"), t)


def det_lstm_pack_bytes(K, units):
    return int(_lib.load().mnn_det_lstm_pack_bytes(int(K), int(units)))


def det_lstm_pack(W, units, out=None):
    """W f32 [K, 4 units] (TF layout) repacked for lstm_step_det's job["Wp"]; to be redone whenever W changes."""
    _req(W.dtype == torch.float32 and W.is_contiguous() and W.dim() == 2 and W.shape[1] == 4 * units and W.shape[0] > units, "det_lstm_pack: W f32 [K, 4 units]")
    n = det_lstm_pack_bytes(W.shape[0], units) // 4
    if out is None:
        out = torch.empty(n, device=W.device, dtype=torch.float32)
    _req(out.dtype == torch.float32 and out.numel() == n and out.is_contiguous() and out.data_ptr() % 16 == 0, "det_lstm_pack: out")
    call("mnn_det_lstm_pack", _stream(), _ptr(W), W.shape[0], int(units), _ptr(out))
    return out


def dense_det(jobs):
    """out = x . W + bias per job (ascending-k fmaf chain), all jobs in one launch.  job = dict(x f32 [B, K], W f32 [K, N] (row pitch >= N),
    bias f32 [N] or None, out f32 [B, >= N] view)."""
    _req(1 <= len(jobs) <= 8, "dense_det: 1..8 jobs")
    arr = (_lib.DetDenseJob * len(jobs))()
    B = jobs[0]["x"].shape[0]
    for a, j in zip(arr, jobs):
        x, W, b, out = j["x"], j["W"], j.get("bias"), j["out"]
        _rowmajor(x, "dense_det x"); _rowmajor(W, "dense_det W"); _rowmajor(out, "dense_det out")
        K, N = W.shape
        _req(x.dtype == W.dtype == out.dtype == torch.float32 and x.shape == (B, K) and out.shape[0] == B and out.shape[1] == N, "dense_det: f32 x [B,K], W [K,N], out [B,N]")
        _req(b is None or (b.dtype == torch.float32 and b.is_contiguous() and b.numel() == N), "dense_det: bias f32 [N]")
        a.x, a.ld_x, a.K, a.W, a.ld_w, a.N, a.bias, a.out, a.ld_out = _ptr(x), x.stride(0), K, _ptr(W), W.stride(0), N, _ptr(b), _ptr(out), out.stride(0)
        Wp = j.get("Wp")                                     # det_dense_pack(W): the same numbers in the kernel's load order (optional)
        _req(Wp is None or (Wp.dtype == torch.float32 and Wp.is_contiguous() and Wp.numel() * 4 == int(_lib.load().mnn_det_dense_pack_bytes(K, N)) and Wp.data_ptr() % 16 == 0),
             "dense_det: Wp is det_dense_pack(W)")
        a.Wp = _ptr(Wp)
    call("mnn_dense_det", _stream(), B, len(jobs), arr)


def det_dense_pack(W, out=None):
    """W f32 [K, N] (row pitch >= N) repacked for dense_det's job["Wp"]; to be redone whenever W changes."""
    _rowmajor(W, "det_dense_pack W")
    _req(W.dtype == torch.float32 and W.dim() == 2, "det_dense_pack: W f32 [K, N]")
    K, N = W.shape
    n = int(_lib.load().mnn_det_dense_pack_bytes(K, N)) // 4
    if out is None:
        out = torch.empty(n, device=W.device, dtype=torch.float32)
    _req(out.dtype == torch.float32 and out.numel() == n and out.is_contiguous() and out.data_ptr() % 16 == 0, "det_dense_pack: out")
    call("mnn_det_dense_pack", _stream(), _ptr(W), K, N, W.stride(0), _ptr(out))
    return out


def _scan_tables(what, layers, n_in, n_out, dense_W, dense_bias, w_enc, w_dec, tracks, D, Hn):
    """The host checks the scan entry points share, and the layer table (mnn_scan_lstm_layer array) they pass."""
    arr = (_lib.ScanLstmLayer * len(layers))()
    k_in = n_in
    for a, (W, b) in zip(arr, layers):
        u = b.numel() // 4
        _req(W.dtype == torch.float32 and W.is_contiguous() and tuple(W.shape) == (k_in + u, 4 * u) and b.dtype == torch.float32 and b.is_contiguous(),
             f"{what}: layer weights f32 [(n_in + u), 4u] / [4u]")
        a.W, a.bias, a.units = _ptr(W), _ptr(b), u
        k_in = u
    _req(dense_W.dtype == torch.float32 and dense_W.is_contiguous() and tuple(dense_W.shape) == (k_in, n_out), f"{what}: Dense kernel f32 [units_last, n_out]")
    _req(dense_bias is None or (dense_bias.dtype == torch.float32 and dense_bias.is_contiguous() and dense_bias.numel() == n_out), f"{what}: Dense bias")
    for w in (w_enc, w_dec):
        _req(w.dtype == torch.float32 and w.is_contiguous() and w.numel() == tracks * D * Hn, f"{what}: NADE weights f32 [tracks, D, Hn]")
    return arr


def _scan_state(what, state, arr, B, device):
    """(c pointers, h pointers) of a per-layer [(c, h) f32 [B, u]] state, or (None, None)."""
    if state is None:
        return None, None
    _req(len(state) == len(arr), f"{what}: one (c, h) per layer")
    for (c, h), a in zip(state, arr):
        for t in (c, h):
            _req(t.dtype == torch.float32 and tuple(t.shape) == (B, a.units) and t.is_contiguous() and t.device == device,
                 f"{what} entries f32 [B, u], contiguous")
    return (C.c_void_p * len(arr))(*[c.data_ptr() for c, _ in state]), (C.c_void_p * len(arr))(*[h.data_ptr() for _, h in state])


def _scan_call(what, ref, intro, Ti, num_steps, layers, dense_W, dense_bias, tracks, D, Hn, w_enc, w_dec, seed, row0, given):
    """What generate_scan and generate_scan_chunk share: the table and `given` checks, the workspace (256-byte aligned) and the samples
    u8 [B, num_steps, tracks * D] on ref's device -> (layer table, launch).  launch(symbol, temps, *state) makes the call -- the 16 leading
    arguments, the temperature slot (`temps`: one argument, or the pair (temps, caps) of the _caps entry points), seed .. given, then the entry
    point's own state arguments -- and returns the samples."""
    B, n_in, n_out = ref.shape[0], tracks * D, tracks * (Hn + D)
    arr = _scan_tables(what, layers, n_in, n_out, dense_W, dense_bias, w_enc, w_dec, tracks, D, Hn)
    if given is not None:
        _req(given.dtype == torch.uint8 and tuple(given.shape) == (B, num_steps, n_in) and given.is_contiguous() and given.device == ref.device,
             f"{what}: given u8 [B, num_steps, tracks * D], contiguous")
    need = int(_lib.load().mnn_generate_scan_workspace_bytes(B, n_in, len(layers), arr, n_out))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=ref.device)
    off = (-ws.data_ptr()) % 256
    samples = torch.empty((B, num_steps, n_in), dtype=torch.uint8, device=ref.device)

    def launch(symbol, temps, *state):
        call(symbol, _stream(), B, Ti, num_steps, _ptr(intro), n_in, len(layers), arr, _ptr(dense_W), _ptr(dense_bias), n_out, tracks, D, Hn,
             _ptr(w_enc), _ptr(w_dec), *(temps if isinstance(temps, tuple) else (temps,)), int(seed), int(row0), _ptr(samples), C.c_void_p(ws.data_ptr() + off), need, _ptr(given), *state)
        return samples                      # (the workspace returns to the allocator in stream order: later users are behind the scan)
    return arr, launch


def generate_scan(intro, num_steps, layers, dense_W, dense_bias, tracks, D, Hn, w_enc, w_dec, temperature, seed, row0, given=None, state0=None,
                  by_visible=False, max_notes=None, redraws=0, redraw_stats=None, particles=0, ess=None, pick=None, lengths=None):
    """mnn_generate_scan: the whole sampling scan of an LSTM-(Multi)NADE generator in one call.  intro u8 [B, Ti, tracks * D]; layers = [(W, bias)]
    f32 master weights; returns samples u8 [B, num_steps, tracks * D].  given (optional): codes u8 [B, num_steps, tracks * D] in the layout of
    the samples (see nade_sample).  temperature: a float, None, or a sequence (per track, or by visible index: nade_sample).  state0 (optional, mnn_generate_scan_state): [(c0, h0) f32 [B, u]] per layer, the state the intro pass starts from.
    lengths (optional, mnn_generate_scan_ragged): int32 [B] on the device, row b's prompt being intro[b, :lengths[b]]; without it every
    call below is the entry point it was."""
    _req(intro.dtype == torch.uint8 and intro.dim() == 3 and intro.is_contiguous() and intro.shape[2] == tracks * D, "generate_scan: intro u8 [B, Ti, tracks * D]")
    arr, launch = _scan_call("generate_scan", intro, intro, intro.shape[1], int(num_steps), layers, dense_W, dense_bias, tracks, D, Hn, w_enc, w_dec,
                             seed, row0, given)
    tt = _temps(temperature, tracks, by_visible, "generate_scan")
    cp, hp = _scan_state("generate_scan: state0", state0, arr, intro.shape[0], intro.device)
    cc = _caps(max_notes, tracks, by_visible, "generate_scan")
    rd = _redraw(redraws, redraw_stats, cc, temperature, intro, "generate_scan")
    if lengths is not None:         # ragged prompts: the one entry point that takes them, with everything else a call can carry
        lp = _prompt_lengths_dev(lengths, intro.shape[0], intro.device, "generate_scan")
        sr = None
        if particles and particles > 1 and given is not None:
            _req(cc is None and temperature is not None, "generate_scan: particles go with a temperature and without max_notes")
            sr, ws = _sir("generate_scan", particles, ess, pick, (int(num_steps), tracks, intro.shape[0]), tracks, intro.shape[0], D, intro)
        return launch("mnn_generate_scan_ragged", (C.byref(_temps_table(temperature, tracks, by_visible, "generate_scan")), None if cc is None else C.byref(cc)),
                      cp, hp, None if rd is None else C.byref(rd), None if sr is None else C.byref(sr), lp)
    if particles and particles > 1 and given is not None:      # importance resampling (nade_sample_sir): ess / pick [num_steps, tracks, B] are written
        _req(cc is None and temperature is not None, "generate_scan: particles go with a temperature and without max_notes")
        sr, ws = _sir("generate_scan", particles, ess, pick, (int(num_steps), tracks, intro.shape[0]), tracks, intro.shape[0], D, intro)
        return launch("mnn_generate_scan_sir", (C.byref(_temps_table(temperature, tracks, by_visible, "generate_scan")), None), cp, hp, None, C.byref(sr))
    if rd is not None:              # the cap by rejection (nade_sample): the caps entry point with the redraws behind its state
        return launch("mnn_generate_scan_redraw", (C.byref(_temps_table(temperature, tracks, by_visible, "generate_scan")), C.byref(cc)), cp, hp,
                      C.byref(rd))
    if cc is not None:              # polyphony caps (nade_sample): the entry point that takes both tables
        return launch("mnn_generate_scan_caps", (C.byref(_temps_table(temperature, tracks, by_visible, "generate_scan")), C.byref(cc)), cp, hp)
    if tt is not None:              # a temperature table: the one entry point that takes it, with or without an initial state
        return launch("mnn_generate_scan_temps", C.byref(tt), cp, hp)
    t = float(-1.0 if temperature is None else temperature)
    return launch("mnn_generate_scan", t) if state0 is None else launch("mnn_generate_scan_state", t, cp, hp)


def generate_scan_chunk(intro, num_steps, layers, dense_W, dense_bias, tracks, D, Hn, w_enc, w_dec, temperature, seed, row0, state_in, state_out,
                        given=None, step0=0, step_base=None, by_visible=False, max_notes=None, redraws=0, redraw_stats=None, particles=0, ess=None,
                        pick=None, lengths=None):
    """mnn_generate_scan_chunk: one chunk of a generation session of an LSTM-(Multi)NADE generator.  intro u8 [B, Ti, tracks * D] or None (the
    chunk continues from state_in); num_steps >= 0 (0 with an intro: the intro pass alone -> None); state_in: [(c, h) f32 [B, u]] per layer or
    None (the zero state); state_out: likewise, written with the state behind the last step (may be the arrays of state_in).  Step st draws
    with the sub-counter step0 + *step_base + st (step_base: one int32 on the device, or None).  Returns samples u8 [B, num_steps, tracks * D];
    given (optional): the chunk's codes in that layout.  lengths (optional, with an intro; mnn_generate_scan_chunk_ragged): the prompt
    lengths, int32 [B] on the device.  Everything else is generate_scan."""
    ref = intro if intro is not None else state_in[0][0]
    num_steps, Ti = int(num_steps), 0 if intro is None else intro.shape[1]
    _req(intro is None or (intro.dtype == torch.uint8 and intro.dim() == 3 and intro.is_contiguous() and intro.shape[2] == tracks * D and Ti > 0),
         "generate_scan_chunk: intro u8 [B, Ti, tracks * D]")
    _req(num_steps >= 0 and Ti + num_steps > 0 and (Ti > 0 or state_in is not None), "generate_scan_chunk: an intro, or steps from an input state")
    arr, launch = _scan_call("generate_scan_chunk", ref, intro, Ti, num_steps, layers, dense_W, dense_bias, tracks, D, Hn, w_enc, w_dec, seed, row0, given)
    ci, hi = _scan_state("generate_scan_chunk: state_in", state_in, arr, ref.shape[0], ref.device)
    co, ho = _scan_state("generate_scan_chunk: state_out", state_out, arr, ref.shape[0], ref.device)
    _req(0 <= int(step0) and int(step0) + num_steps <= 1 << 32, "generate_scan_chunk: step0 + num_steps passes 2^32")
    tt = _temps_table(temperature, tracks, by_visible, "generate_scan_chunk")
    cc = _caps(max_notes, tracks, by_visible, "generate_scan_chunk")
    rd = _redraw(redraws, redraw_stats, cc, temperature, ref, "generate_scan_chunk")
    if lengths is not None:         # ragged prompts: generate_scan's
        _req(Ti > 0, "generate_scan_chunk: lengths go with an intro")
        lp = _prompt_lengths_dev(lengths, ref.shape[0], ref.device, "generate_scan_chunk")
        sr = None
        if particles and particles > 1 and given is not None and num_steps > 0:
            _req(cc is None and temperature is not None, "generate_scan_chunk: particles go with a temperature and without max_notes")
            sr, ws = _sir("generate_scan_chunk", particles, ess, pick, (num_steps, tracks, ref.shape[0]), tracks, ref.shape[0], D, ref)
        samples = launch("mnn_generate_scan_chunk_ragged", (C.byref(tt), None if cc is None else C.byref(cc)), ci, hi, co, ho, int(step0),
                         _sub_base(step_base, ref, "generate_scan_chunk"), None if rd is None else C.byref(rd), None if sr is None else C.byref(sr), lp)
        return samples if num_steps > 0 else None
    if particles and particles > 1 and given is not None and num_steps > 0:      # importance resampling: generate_scan's
        _req(cc is None and temperature is not None, "generate_scan_chunk: particles go with a temperature and without max_notes")
        sr, ws = _sir("generate_scan_chunk", particles, ess, pick, (num_steps, tracks, ref.shape[0]), tracks, ref.shape[0], D, ref)
        return launch("mnn_generate_scan_chunk_sir", (C.byref(tt), None), ci, hi, co, ho, int(step0), _sub_base(step_base, ref, "generate_scan_chunk"),
                      None, C.byref(sr))
    if rd is not None:
        samples = launch("mnn_generate_scan_chunk_redraw", (C.byref(tt), C.byref(cc)), ci, hi, co, ho, int(step0),
                         _sub_base(step_base, ref, "generate_scan_chunk"), C.byref(rd))
        return samples if num_steps > 0 else None
    if cc is not None:
        samples = launch("mnn_generate_scan_chunk_caps", (C.byref(tt), C.byref(cc)), ci, hi, co, ho, int(step0),
                         _sub_base(step_base, ref, "generate_scan_chunk"))
        return samples if num_steps > 0 else None
    samples = launch("mnn_generate_scan_chunk", C.byref(tt), ci, hi, co, ho, int(step0), _sub_base(step_base, ref, "generate_scan_chunk"))
    return samples if num_steps > 0 else None
