// The Gibbs chain of the RBMs, whole: the chain bodies, the argument block of their kernels, the three kernel templates and the ONE host
// dispatch that every entry point -- single (rbm.hip) or grouped (rbm_multi.hip), free or clamped, tempered or not -- goes through.  Also the
// free-energy body.
//
// Every body is one templated device function over a GibbsView -- the per-job argument block: a kernel builds the view of ITS job (the one
// job of mnn_rbm_gibbs, or job blockIdx.y of mnn_rbm_gibbs_multi) and calls the body with its first row.  STRIDED = false is the layout the
// single launches always had (v0 / p_v / v_out contiguous [N, D]); STRIDED = true addresses cell (n, d) of v0 / p_v / v_out at
// n * rs + d * es and of the codes at n * ld_given + d * es (es = M: track m of a composer-layout row [D, M], read and written in place).
// The arithmetic does not depend on the addressing, so a grouped job is bit for bit its single launch.
//
// A translation unit instantiates the kernels of the argument blocks its entry points fill, and no others: rbm.hip the single-job blocks,
// rbm_multi.hip the job tables -- (LDS 4 + matrix cores 1 + streaming 1) x GIVEN x TEMPERED = 24 kernels each.
#pragma once
#include "common.h"

#define RBM_R 8

__device__ __forceinline__ uint32_t rbm_rowid(const uint32_t* __restrict__ row_ids, uint32_t row0, int n) {
    return row_ids != nullptr ? row_ids[n] : row0 + (uint32_t)n;
}

// out-unit phase: for each output unit `o` (strided over threads) and each of the block's rows
//   z[r] = sum_{k asc} in[r][k] * Wk[k*ldw + o]  + bias[row r][o]
// in_s: LDS [RBM_R][Kpad] f32 (Kpad multiple of 4, zero padded).  Calls fn(r, o, z).
// The bias rows bias[(n0 + r) * ld_bias + o] (ld_bias = 0: one shared row) are REQUESTED in front of the K loop and added behind it; the
// weights come 16 k at a time, unconditionally (k clamped: the inputs are zero past K, so the clamped weight contributes fma(0, w, acc) = acc
// exactly -- same ascending fma chain, bit for bit).  Round 3: with `k < K ? load : 0` per weight and the bias loaded inside the per-row
// callback every load was waited for on its own (s_waitcnt vmcnt(0) per element: 4 + 8 memory round trips per 4 k).
template <typename F>
__device__ __forceinline__ void rbm_phase(const float* __restrict__ in_s, int Kpad, int K, const float* __restrict__ Wk, int ldw, int n_out,
                                          const float* __restrict__ bias, int ld_bias, int n0, int N, F&& fn) {
    for (int o = threadIdx.x; o < n_out; o += blockDim.x) {
        float acc[RBM_R], bb[RBM_R];
#pragma unroll
        for (int r = 0; r < RBM_R; ++r) { acc[r] = 0.f; bb[r] = bias[(size_t)min(n0 + r, N - 1) * ld_bias + o]; }
        for (int k0 = 0; k0 < K; k0 += 16) {
            float w[16];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) w[kk] = Wk[(size_t)min(k0 + kk, K - 1) * ldw + o];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (k0 + 4 * q < K) {                       // block-uniform; Kpad covers the quad
#pragma unroll
                    for (int r = 0; r < RBM_R; ++r) {
                        const float4 x = *reinterpret_cast<const float4*>(in_s + r * Kpad + k0 + 4 * q);
                        acc[r] = fmaf(x.x, w[4 * q + 0], acc[r]);
                        acc[r] = fmaf(x.y, w[4 * q + 1], acc[r]);
                        acc[r] = fmaf(x.z, w[4 * q + 2], acc[r]);
                        acc[r] = fmaf(x.w, w[4 * q + 3], acc[r]);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RBM_R; ++r) fn(r, o, acc[r] + bb[r]);
    }
}

template <typename TV>
__device__ __forceinline__ void rbm_load_rows(const TV* __restrict__ src, int N, int n0, int K, int Kpad, float* __restrict__ dst_s) {
    for (int e = threadIdx.x; e < RBM_R * Kpad; e += blockDim.x) {
        const int r = e / Kpad, k = e % Kpad, n = n0 + r;
        dst_s[e] = (n < N && k < K) ? (float)src[(size_t)n * K + k] : 0.f;
    }
}

// codes of the clamped chain (u8 per visible): 0 / 1 hold the visible at that value, RBM_GIVEN_FREE leaves it to the chain
#define RBM_GIVEN_FREE 255

// per-job argument block of the chain bodies
struct GibbsView {
    int N, D, Hn, k;
    const uint8_t* v0; const float* W; const float* Wt; const float* bh; int ld_bh; const float* bv; int ld_bv;
    uint64_t seed; uint32_t row0; const uint32_t* row_ids; uint32_t sub0; float* p_v; uint8_t* v_out;
    const uint8_t* given; long ld_given;      // GIVEN only
    long rs; int es;                          // STRIDED only
    float temp;                               // TEMPERED only: the chain samples exp(-E / temp)
};
// TEMPERED (a template flag of the three chain bodies, false = the code they always were): every conditional of the chain, hidden and visible,
// is det_sigmoid(z / temp) with z the pre-activation including its bias -- the Gibbs chain of the RBM with energy E / temp.  A division, as in the
// NADE scan: by a power of two it is exact, so that chain is bit for bit the untempered one on parameters scaled by 1 / temp.  Uniforms, counters
// and clamps are untouched; p_v is the tempered probability the last visible phase drew from.
template <bool TEMPERED> __device__ __forceinline__ float gv_sigmoid(const GibbsView& a, float z) {
    return det_sigmoid(TEMPERED ? z / a.temp : z);
}
template <bool STRIDED> __device__ __forceinline__ size_t gv_cell(const GibbsView& a, int n, int d) {
    return STRIDED ? (size_t)n * a.rs + (size_t)d * a.es : (size_t)n * a.D + d;
}
template <bool STRIDED> __device__ __forceinline__ size_t gv_code(const GibbsView& a, int n, int d) {
    return STRIDED ? (size_t)n * a.ld_given + (size_t)d * a.es : (size_t)n * a.ld_given + d;
}

template <int R, int RG, typename F>      // RG rows per thread; thread t -> (row group t / n_out, output t % n_out)
__device__ __forceinline__ void rbm_phase_lds(const float* __restrict__ in_s, int Kpad, int K, const float* __restrict__ Ws, int w_k_stride,
                                              int w_o_stride, int n_out, F&& fn) {
    const int g = threadIdx.x / n_out, o = threadIdx.x - g * n_out;
    if (g >= R / RG) return;
    const float* __restrict__ wp = Ws + (size_t)o * w_o_stride;
    const float* __restrict__ xp = in_s + (size_t)g * RG * Kpad;
    float acc[RG];
#pragma unroll
    for (int r = 0; r < RG; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 4) {
        float w[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) w[kk] = wp[(size_t)min(k0 + kk, K - 1) * w_k_stride];     // beyond K the input is the zero padding
#pragma unroll
        for (int r = 0; r < RG; ++r) {
            const float4 x = *reinterpret_cast<const float4*>(xp + r * Kpad + k0);
            acc[r] = fmaf(x.x, w[0], acc[r]);
            acc[r] = fmaf(x.y, w[1], acc[r]);
            acc[r] = fmaf(x.z, w[2], acc[r]);
            acc[r] = fmaf(x.w, w[3], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < RG; ++r) fn(g * RG + r, r, o, acc[r]);
}

typedef float gm_f32x16 __attribute__((ext_vector_type(16)));
#define GM_ROWS 64

// pitch (bytes) of a byte-state row of `n` cells: covers n rounded up to even (the k pairs of the MFMA), a whole number of words, and an ODD
// number of words (rows land in distinct banks)
static __host__ __device__ __forceinline__ int gm_pitch(int n) { int w = (n + 1 + 3) / 4; return 4 * (w | 1); }

// one output tile (32 units x 32 rows) of a phase: K ascending in pairs; A = W (unit, k) from LDS, B = the rows' byte states
// (Reading the operands of eight k-pairs ahead of their MFMAs -- what the single-wave det-step kernels need -- was measured SLOWER here, 2.78 ->
// 3.19 ms per jamming step: with two waves per SIMD the other wave's MFMA fills the LDS wait, and the batches cost 60 more registers.)
template <bool VIS>
__device__ __forceinline__ void gm_chain(const float* __restrict__ Ws, int ldw, const uint8_t* __restrict__ st, int pitch, int K, int unit,
                                         int lane, gm_f32x16& acc) {
    const int r = lane & 31, hh = lane >> 5;
    const uint8_t* sp = st + r * pitch + hh;
    // hidden phase: A[i = hidden j][k = d] = W[d][j] (walks down a column); visible phase: A[i = visible d][k = j] = W[d][j] (walks a row)
    const float* ap = VIS ? Ws + (size_t)unit * ldw + hh : Ws + (size_t)hh * ldw + unit;
    const int astep = VIS ? 2 : 2 * ldw;
    for (int s = 0; s < K / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[(size_t)s * astep], (float)sp[2 * s], acc, 0, 0, 0);
}

// GIVEN helper of the matrix-core chain: whether any of the four codes packed into a word (gv_code_quad) is free
__device__ __forceinline__ bool gm_any_free(uint32_t q) {
    return (q & 0xffu) == 0xffu || (q & 0xff00u) == 0xff00u || (q & 0xff0000u) == 0xff0000u || (q & 0xff000000u) == 0xff000000u;
}
// the codes of cells d0 .. d0 + 3 of one row packed into a word (cells past D repeat D - 1: never used)
template <bool STRIDED>
__device__ __forceinline__ uint32_t gv_code_quad(const GibbsView& a, int row, int d0) {
    uint32_t q = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) q |= (uint32_t)a.given[gv_code<STRIDED>(a, row, min(d0 + e, a.D - 1))] << (8 * e);
    return q;
}

// ----------------------------------------------------------------------------------------------
// STREAMING form: one 256-thread workgroup owns RBM_R rows for the whole chain: their visible and hidden states live in LDS (as f32 0/1), W
// is streamed from L2 (coalesced over the output unit; a transposed copy Wt serves the visible phase), each thread accumulates RBM_R rows of
// one output unit.
// smem: f32 [RBM_R][Dp] | f32 [RBM_R][Hp] | GIVEN: u8 [RBM_R][Dp]
// ----------------------------------------------------------------------------------------------
template <bool GIVEN, bool STRIDED, bool TEMPERED = false>
__device__ __forceinline__ void rbm_gibbs_stream_body(const GibbsView& a, const int n0, float* __restrict__ smem) {
    const int N = a.N, D = a.D, Hn = a.Hn, k = a.k;
    const uint64_t seed = a.seed;
    const int Dp = (D + 3) & ~3, Hp = (Hn + 3) & ~3;
    float* vs = smem;                 // [RBM_R][Dp]
    float* hs = smem + RBM_R * Dp;    // [RBM_R][Hp]
    uint8_t* cs = reinterpret_cast<uint8_t*>(hs + RBM_R * Hp);      // GIVEN: the rows' codes [RBM_R][Dp]
    if (STRIDED) {
        for (int e = threadIdx.x; e < RBM_R * Dp; e += blockDim.x) {
            const int r = e / Dp, d = e % Dp, n = n0 + r;
            vs[e] = (n < N && d < D) ? (float)a.v0[gv_cell<true>(a, n, d)] : 0.f;
        }
    } else {
        rbm_load_rows<uint8_t>(a.v0, N, n0, D, Dp, vs);
    }
    if (GIVEN)                        // the same cells per thread as the load above: no barrier in between
        for (int e = threadIdx.x; e < RBM_R * Dp; e += blockDim.x) {
            const int r = e / Dp, d = e % Dp, n = n0 + r;
            const uint8_t c = (n < N && d < D) ? a.given[gv_code<STRIDED>(a, n, d)] : (uint8_t)RBM_GIVEN_FREE;
            cs[e] = c;
            if (c != RBM_GIVEN_FREE) vs[e] = (float)c;
        }
    for (int e = threadIdx.x; e < RBM_R * Hp; e += blockDim.x) hs[e] = 0.f;
    __syncthreads();
    if (k == 0) {                     // tf.while_loop with zero iterations returns (v, v)
        for (int e = threadIdx.x; e < RBM_R * D; e += blockDim.x) {
            const int r = e / D, d = e % D, n = n0 + r;
            if (n < N) {
                if (a.p_v) a.p_v[gv_cell<STRIDED>(a, n, d)] = vs[r * Dp + d];
                if (a.v_out) a.v_out[gv_cell<STRIDED>(a, n, d)] = (uint8_t)vs[r * Dp + d];
            }
        }
        return;
    }
    for (int it = 0; it < k; ++it) {
        rbm_phase(vs, Dp, D, a.W, Hn, Hn, a.bh, a.ld_bh, n0, N, [&](int r, int j, float z) {
            const int n = n0 + r;
            if (n >= N) return;
            const float p = gv_sigmoid<TEMPERED>(a, z);
            const float u = philox_uniform1(seed, MNN_STREAM_RBM_H, rbm_rowid(a.row_ids, a.row0, n), a.sub0 + (uint32_t)it, (uint32_t)j);
            hs[r * Hp + j] = u < p ? 1.f : 0.f;
        });
        __syncthreads();
        const bool last = it == k - 1;
        rbm_phase(hs, Hp, Hn, a.Wt, D, D, a.bv, a.ld_bv, n0, N, [&](int r, int d, float z) {
            const int n = n0 + r;
            if (n >= N) return;
            const float p = gv_sigmoid<TEMPERED>(a, z);
            float s;
            if (GIVEN && cs[r * Dp + d] != RBM_GIVEN_FREE) {
                s = (float)cs[r * Dp + d];
            } else {
                const float u = philox_uniform1(seed, MNN_STREAM_RBM_V, rbm_rowid(a.row_ids, a.row0, n), a.sub0 + (uint32_t)it, (uint32_t)d);
                s = u < p ? 1.f : 0.f;
            }
            vs[r * Dp + d] = s;
            if (last) {
                if (a.p_v) a.p_v[gv_cell<STRIDED>(a, n, d)] = p;
                if (a.v_out) a.v_out[gv_cell<STRIDED>(a, n, d)] = (uint8_t)s;
            }
        });
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------------
// The same chain with W RESIDENT IN LDS (D (Hn + 1) floats fit: D = 88, Hn = 256 is 90 KB).  The streaming form above fetches every
// W row from L2 inside the k loop, twice per Gibbs iteration, and waits for it: 33 us per iteration whatever the row count.  Here W is
// read once per workgroup; the row stride Hn + 1 makes both walks conflict-free (hidden phase: consecutive threads, consecutive
// columns; visible phase: thread d walks row d, bank (d + k) mod 32), so no transposed copy either.  R = 2 rows per workgroup (many
// short workgroups; used below 2048 rows, see rbm_gibbs_forms); a phase with fewer outputs than threads splits the rows over the
// spare threads (visible phase at D = 88: two row groups).  Biases stay in registers over the chain.  Arithmetic and order are
// the streaming form's: ascending-index fma chain from 0, + bias, det_sigmoid, Philox draw -- bit-identical draws.
// smem: f32 [R][Dp] | [R][Hp] | [D][Hn + 1]
// ----------------------------------------------------------------------------------------------
template <int R, int RGH, int RGV, bool GIVEN, bool STRIDED, bool TEMPERED = false>        // rows per thread in the hidden / visible phase (R / RG row groups of n_out threads each)
__device__ __forceinline__ void rbm_gibbs_lds_body(const GibbsView& a, const int n0, float* __restrict__ smem) {
    const int N = a.N, D = a.D, Hn = a.Hn, k = a.k;
    const uint64_t seed = a.seed;
    const uint32_t sub0 = a.sub0;
    const float* __restrict__ W = a.W;
    const int Dp = (D + 3) & ~3, Hp = (Hn + 3) & ~3, ldw = Hn + 1;
    float* vs = smem;                 // [R][Dp]
    float* hs = vs + R * Dp;          // [R][Hp]
    float* Ws = hs + R * Hp;          // [D][ldw]
    for (int d = threadIdx.x >> 6; d < D; d += 4)            // one wave per row of W: coalesced, no index division
        for (int j = threadIdx.x & 63; j < Hn; j += 64) Ws[d * ldw + j] = W[(size_t)d * Hn + j];
    for (int e = threadIdx.x; e < R * Dp; e += blockDim.x) {
        const int r = e / Dp, kx = e % Dp, n = n0 + r;
        vs[e] = (n < N && kx < D) ? (float)a.v0[gv_cell<STRIDED>(a, n, kx)] : 0.f;
        if (GIVEN && n < N && kx < D) {
            const uint8_t c = a.given[gv_code<STRIDED>(a, n, kx)];
            if (c != RBM_GIVEN_FREE) vs[e] = (float)c;
        }
    }
    for (int e = threadIdx.x; e < R * Hp; e += blockDim.x) hs[e] = 0.f;
    // this thread's biases, row ids (and GIVEN: codes of its visible cells): constant over the chain
    float bhr[RGH], bvr[RGV];
    uint32_t idh[RGH], idv[RGV], cvr[RGV];
    {
        const int g = threadIdx.x / Hn, o = threadIdx.x - g * Hn;
#pragma unroll
        for (int r = 0; r < RGH; ++r) {
            const int n = min(n0 + g * RGH + r, N - 1);
            bhr[r] = a.bh[(size_t)n * a.ld_bh + min(o, Hn - 1)];
            idh[r] = rbm_rowid(a.row_ids, a.row0, n);
        }
    }
    {
        const int g = threadIdx.x / D, o = threadIdx.x - g * D;
#pragma unroll
        for (int r = 0; r < RGV; ++r) {
            const int n = min(n0 + min(g * RGV + r, R - 1), N - 1);
            bvr[r] = a.bv[(size_t)n * a.ld_bv + min(o, D - 1)];
            idv[r] = rbm_rowid(a.row_ids, a.row0, n);
            if (GIVEN) cvr[r] = a.given[gv_code<STRIDED>(a, n, min(o, D - 1))];
        }
    }
    __syncthreads();
    if (k == 0) {                     // tf.while_loop with zero iterations returns (v, v)
        for (int e = threadIdx.x; e < R * D; e += blockDim.x) {
            const int r = e / D, d = e % D, n = n0 + r;
            if (n < N) {
                if (a.p_v) a.p_v[gv_cell<STRIDED>(a, n, d)] = vs[r * Dp + d];
                if (a.v_out) a.v_out[gv_cell<STRIDED>(a, n, d)] = (uint8_t)vs[r * Dp + d];
            }
        }
        return;
    }
    for (int it = 0; it < k; ++it) {
        rbm_phase_lds<R, RGH>(vs, Dp, D, Ws, ldw, 1, Hn, [&](int r, int rl, int j, float acc) {
            if (n0 + r >= N) return;
            const float p = gv_sigmoid<TEMPERED>(a, acc + bhr[rl]);
            const float u = philox_uniform1(seed, MNN_STREAM_RBM_H, idh[rl], sub0 + (uint32_t)it, (uint32_t)j);
            hs[r * Hp + j] = u < p ? 1.f : 0.f;
        });
        __syncthreads();
        const bool last = it == k - 1;
        rbm_phase_lds<R, RGV>(hs, Hp, Hn, Ws, 1, ldw, D, [&](int r, int rl, int d, float acc) {
            const int n = n0 + r;
            if (n >= N) return;
            const float p = gv_sigmoid<TEMPERED>(a, acc + bvr[rl]);
            float sv;
            if (GIVEN && cvr[rl] != RBM_GIVEN_FREE) {        // clamped: no Philox evaluation
                sv = (float)cvr[rl];
            } else {
                const float u = philox_uniform1(seed, MNN_STREAM_RBM_V, idv[rl], sub0 + (uint32_t)it, (uint32_t)d);
                sv = u < p ? 1.f : 0.f;
            }
            vs[r * Dp + d] = sv;
            if (last) {
                if (a.p_v) a.p_v[gv_cell<STRIDED>(a, n, d)] = p;
                if (a.v_out) a.v_out[gv_cell<STRIDED>(a, n, d)] = (uint8_t)sv;
            }
        });
        __syncthreads();
    }
}

static inline size_t rbm_lds_resident_bytes(int R, int D, int Hn) {
    return ((size_t)R * (((D + 3) & ~3) + ((Hn + 3) & ~3)) + (size_t)D * (Hn + 1)) * sizeof(float);
}

// ----------------------------------------------------------------------------------------------
// The chain on the MATRIX CORES, bit for bit the same draws (training batches, N >= 2048 rows).  v_mfma_f32_32x32x2_f32 computes
// D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) with one IEEE rounding per product-add (cdna_hip_programming.md, "FP32-input MFMA"): a run of
// such instructions over ascending k IS the ascending-index fmaf chain of the vector forms above, so the logits -- and with them every
// Bernoulli draw -- are identical, at the matrix pipe's rate instead of one fma per lane and term (the vector form reaches 22 TFLOP/s of the
// 157 f32 peak: its inner loop is LDS reads and address arithmetic).  Layout: a workgroup (8 waves) owns GM_ROWS = 64 rows for the whole chain;
// W sits in LDS once (f32 [D][Hn + 1]); the binary v / h states sit in LDS as BYTES (row pitch = an odd number of words: the B-operand reads
// of the 32 rows of a tile hit 32 banks).  The product is formed TRANSPOSED, C[out unit][row] = sum_k W(k, unit) state[row][k] (A = the weights,
// B = the states): a lane then holds four CONSECUTIVE output units of one row per accumulator quad = exactly the four uniforms of one
// Philox block (element >> 2 is the block counter), so every Philox evaluation is used in full -- the vector forms draw one element per
// evaluation.  Hidden phase: 2 row tiles x (Hn / 32) unit tiles, two unit tiles per wave share the state operand; visible phase:
// 2 x ceil(D / 32) jobs on the first waves (one K = Hn chain per output: it cannot be split without changing the summation order).
// smem: f32 [De][Hn + 1] | u8 [64][pv] | u8 [64][ph]
// GIVEN: the codes clamp the byte states at load and after each visible quad; a lane's codes of its first-pass visible job stay in registers
// (four packed words next to bvr: no LDS, so the given form fits wherever the free one does); a quad whose four cells are all clamped skips its
// Philox block
// ----------------------------------------------------------------------------------------------
template <bool GIVEN, bool STRIDED, bool TEMPERED = false>
__device__ __forceinline__ void rbm_gibbs_mfma_body(const GibbsView& A, const int n0, float* __restrict__ smem) {
    const uint64_t seed = A.seed;
    const int N = A.N, D = A.D, Hn = A.Hn, ldw = Hn + 1;
    const int De = (D + 1) & ~1, He = (Hn + 1) & ~1;          // K of the two phases (even; the states are zero past D / Hn)
    const int pv = gm_pitch(D), ph = gm_pitch(Hn);
    float* Ws = smem;                                         // [De][ldw] (row D, if any, repeats row D - 1: its inputs are zero)
    uint8_t* vs = reinterpret_cast<uint8_t*>(Ws + (size_t)De * ldw);      // [64][pv]
    uint8_t* hs = vs + GM_ROWS * pv;                                        // [64][ph]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int d = w; d < De; d += 8)                          // one wave per row of W: coalesced
        for (int j = lane; j < ldw; j += 64) Ws[d * ldw + j] = j < Hn ? A.W[(size_t)min(d, D - 1) * Hn + j] : 0.f;
    {   // v0 rows: thread t -> row t >> 3, eight lanes walk its bytes, sixteen loads in flight (unconditional, clamped)
        const int rr = threadIdx.x >> 3, sub = threadIdx.x & 7, n = n0 + rr;
        const int es = STRIDED ? A.es : 1;
        const uint8_t* __restrict__ src = A.v0 + gv_cell<STRIDED>(A, min(n, N - 1), 0);
        const uint8_t* __restrict__ gsrc = GIVEN ? A.given + gv_code<STRIDED>(A, min(n, N - 1), 0) : nullptr;
        for (int kb = sub; kb < pv; kb += 128) {
            uint8_t v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = STRIDED ? src[(size_t)min(kb + 8 * q, D - 1) * es] : src[min(kb + 8 * q, D - 1)];
            if (GIVEN) {
                uint8_t c[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) c[q] = STRIDED ? gsrc[(size_t)min(kb + 8 * q, D - 1) * es] : gsrc[min(kb + 8 * q, D - 1)];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = c[q] != RBM_GIVEN_FREE ? c[q] : v[q];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (kb + 8 * q < pv) vs[rr * pv + kb + 8 * q] = (n < N && kb + 8 * q < D) ? v[q] : (uint8_t)0;
        }
    }
    for (int e = threadIdx.x; e < GM_ROWS * ph; e += 512) hs[e] = 0;
    const int r = lane & 31, hh = lane >> 5;
    // jobs: hidden -- row tile w >> 2, unit tiles 2 (w & 3) + 8 q ... (two per pass, all Hn / 32 covered in ceil(Hn / 256) passes);
    //       visible -- job id w (+ 8 per pass) = row tile * ndt + unit tile
    const int nht = (Hn + 31) / 32, ndt = (D + 31) / 32;
    const int rt_h = w >> 2;
    const int row_h = n0 + 32 * rt_h + r;                     // the batch row of this lane's accumulator column (hidden jobs)
    const uint32_t id_h = rbm_rowid(A.row_ids, A.row0, min(row_h, N - 1));
    // the biases of this wave's first-pass jobs stay in registers over the chain (they do not change between Gibbs iterations; loaded inside
    // the epilogue, every accumulator quad waited for its own L2 round trip in every iteration)
    float bhr[2][16], bvr[16];
    uint32_t cvr[4];                                          // GIVEN: the codes of the first-pass visible job, one quad per word
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = min(32 * (2 * (w & 3) + q) + (e & 3) + 8 * (e >> 2) + 4 * hh, Hn - 1);
            bhr[q][e] = A.bh[(size_t)min(row_h, N - 1) * A.ld_bh + j];
        }
    {
        const int job = min(w, 2 * ndt - 1), rt = job / ndt, dt = job - rt * ndt;
        const int row = min(n0 + 32 * rt + r, N - 1);
#pragma unroll
        for (int e = 0; e < 16; ++e) bvr[e] = A.bv[(size_t)row * A.ld_bv + min(32 * dt + (e & 3) + 8 * (e >> 2) + 4 * hh, D - 1)];
        if (GIVEN)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) cvr[g4] = gv_code_quad<STRIDED>(A, row, 32 * dt + 8 * g4 + 4 * hh);
    }
    __syncthreads();
    if (A.k == 0) {
        for (int e = threadIdx.x; e < GM_ROWS * D; e += 512) {
            const int rr = e / D, d = e - rr * D, n = n0 + rr;
            if (n < N) {
                if (A.p_v) A.p_v[gv_cell<STRIDED>(A, n, d)] = (float)vs[rr * pv + d];
                if (A.v_out) A.v_out[gv_cell<STRIDED>(A, n, d)] = vs[rr * pv + d];
            }
        }
        return;
    }
    for (int it = 0; it < A.k; ++it) {
        // ---- hidden phase ----
        for (int jt0 = 2 * (w & 3); jt0 < nht; jt0 += 8) {
            gm_f32x16 acc[2];
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
            const uint8_t* sp = vs + (32 * rt_h + r) * pv + hh;
            const int u0 = min(32 * jt0 + r, Hn - 1), u1 = min(32 * (jt0 + 1) + r, Hn - 1);
            const float* a0 = Ws + (size_t)hh * ldw + u0;
            const float* a1 = Ws + (size_t)hh * ldw + u1;
            const bool two = jt0 + 1 < nht;
            for (int s = 0; s < De / 2; ++s) {                // the two unit tiles share the state operand
                const float b = (float)sp[2 * s];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[(size_t)s * 2 * ldw], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[(size_t)s * 2 * ldw], b, acc[1], 0, 0, 0);      // (a lone last tile repeats column Hn - 1: discarded)
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q == 1 && !two) break;
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int j0 = 32 * (jt0 + q) + 8 * g4 + 4 * hh;          // four consecutive hidden units: one Philox block
                    if (j0 >= Hn) continue;
                    float u[4];
                    philox_uniform4(seed, MNN_STREAM_RBM_H, id_h, A.sub0 + (uint32_t)it, (uint32_t)(j0 >> 2), u);
                    uint32_t pk = 0u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = min(j0 + e, Hn - 1);
                        const float bb = jt0 < 8 ? bhr[q][4 * g4 + e] : A.bh[(size_t)min(row_h, N - 1) * A.ld_bh + j];
                        const float p = gv_sigmoid<TEMPERED>(A, acc[q][4 * g4 + e] + bb);
                        pk |= (u[e] < p && j0 + e < Hn ? 1u : 0u) << (8 * e);
                    }
                    *reinterpret_cast<uint32_t*>(hs + (32 * rt_h + r) * ph + j0) = pk;     // j0 % 4 == 0, ph % 4 == 0
                }
            }
        }
        __syncthreads();
        // ---- visible phase ----
        const bool last = it == A.k - 1;
        for (int job = w; job < 2 * ndt; job += 8) {
            const int rt = job / ndt, dt = job - rt * ndt;
            gm_f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            gm_chain<true>(Ws, ldw, hs + 32 * rt * ph, ph, He, min(32 * dt + r, D - 1), lane, acc);
            const int row = n0 + 32 * rt + r;
            const uint32_t idv = rbm_rowid(A.row_ids, A.row0, min(row, N - 1));
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * dt + 8 * g4 + 4 * hh;
                if (d0 >= D) continue;
                float u[4];
                uint32_t cq = 0xffffffffu;
                if (GIVEN) cq = job < 8 ? cvr[g4] : gv_code_quad<STRIDED>(A, min(row, N - 1), d0);
                if (!GIVEN || gm_any_free(cq)) philox_uniform4(seed, MNN_STREAM_RBM_V, idv, A.sub0 + (uint32_t)it, (uint32_t)(d0 >> 2), u);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int d = d0 + e;
                    if (d >= D) continue;
                    const float p = gv_sigmoid<TEMPERED>(A, acc[4 * g4 + e] + (job < 8 ? bvr[4 * g4 + e] : A.bv[(size_t)min(row, N - 1) * A.ld_bv + d]));
                    const uint8_t c = (uint8_t)(cq >> (8 * e));
                    const uint8_t sv = GIVEN && c != RBM_GIVEN_FREE ? c : (u[e] < p ? 1 : 0);
                    vs[(32 * rt + r) * pv + d] = sv;
                    if (last && row < N) {
                        if (A.p_v) A.p_v[gv_cell<STRIDED>(A, row, d)] = p;
                        if (A.v_out) A.v_out[gv_cell<STRIDED>(A, row, d)] = sv;
                    }
                }
            }
        }
        __syncthreads();
    }
}

static inline size_t gibbs_mfma_lds_bytes(int D, int Hn) {
    return (size_t)((D + 1) & ~1) * (Hn + 1) * sizeof(float) + (size_t)GM_ROWS * (gm_pitch(D) + gm_pitch(Hn));
}
static inline size_t rbm_lds_bytes(int D, int Hn) { return (size_t)RBM_R * (((D + 3) & ~3) + ((Hn + 3) & ~3)) * sizeof(float); }

// ----------------------------------------------------------------------------------------------
// The argument blocks of the chain kernels, passed by value.  Two shapes: the one job of mnn_rbm_gibbs / _stepped / _temp, contiguous [N, D]
// (STRIDED = false: the bodies keep their n * D + d addressing, the view does not read blockIdx.y), and a table of up to RBM_MULTI_MAX_JOBS
// jobs, job = blockIdx.y, STRIDED.  `given` (null: the free chain), `temp`, `seed_step` and `sub_base` (null: none) are plain fields; whether a kernel
// reads the first two is its GIVEN / TEMPERED.  For the dispatch both give view() on the device and, on the host, jobs(), weights(j),
// set_wt(j, .) (the streaming form's transposed copy), has_given() and complete(j).
// ----------------------------------------------------------------------------------------------
#define RBM_MULTI_MAX_JOBS 8

// the single-job block
template <bool TEMPERED_>
struct GibbsArgs {
    static constexpr bool STRIDED = false, TEMPERED = TEMPERED_;
    int N, D, Hn, k;
    const uint8_t* v0; const float* W; const float* Wt; const float* bh; int ld_bh; const float* bv; int ld_bv;
    uint64_t seed; uint32_t row0; const uint32_t* row_ids; uint32_t sub0; float* p_v; uint8_t* v_out;
    const uint8_t* given; int ld_given; float temp; const int* seed_step;
    const uint32_t* sub_base; uint32_t sub_scale;       // null, or the generated steps before this launch (a session's step cell): sub0 += *sub_base * sub_scale
    __device__ __forceinline__ GibbsView view() const {
        uint64_t sd = seed;
        if (seed_step != nullptr) sd += (uint64_t)(int64_t)*seed_step;      // step counter on the device: a captured launch draws anew every replay
        uint32_t sb = sub0;
        if (sub_base != nullptr) sb += *sub_base * sub_scale;               // likewise the sub-counter base: a captured chunk of a session continues the piece
        return GibbsView{N, D, Hn, k, v0, W, Wt, bh, ld_bh, bv, ld_bv, sd, row0, row_ids, sb, p_v, v_out, given, ld_given, 0, 1, temp};
    }
    int jobs() const { return 1; }
    const float* weights(int) const { return W; }
    void set_wt(int, const float* wt) { Wt = wt; }
    bool has_given() const { return given != nullptr; }
    bool complete(int) const { return v0 && W && bh && bv; }
};

// the job-table block
struct GibbsJob {
    const float* W; const float* Wt; const float* bh; const float* bv; uint64_t seed;
    const uint8_t* v0; float* p_v; uint8_t* v_out; const uint8_t* given;
};
template <bool TEMPERED_>
struct GibbsTableArgs {
    static constexpr bool STRIDED = true, TEMPERED = TEMPERED_;
    GibbsJob job[RBM_MULTI_MAX_JOBS];
    int N, D, Hn, k, ld_bh, ld_bv;
    uint32_t row0; const uint32_t* row_ids; uint32_t sub0; const int* seed_step;
    long rs, rs_given; int es, njobs;
    float temp[RBM_MULTI_MAX_JOBS];          // read by the TEMPERED kernels only
    const uint32_t* sub_base; uint32_t sub_scale;       // as GibbsArgs'
    __device__ __forceinline__ GibbsView view() const {
        const GibbsJob& j = job[blockIdx.y];
        uint64_t seed = j.seed;
        if (seed_step != nullptr) seed += (uint64_t)(int64_t)*seed_step;
        uint32_t sb = sub0;
        if (sub_base != nullptr) sb += *sub_base * sub_scale;
        return GibbsView{N, D, Hn, k, j.v0, j.W, j.Wt, j.bh, ld_bh, j.bv, ld_bv, seed, row0, row_ids, sb, j.p_v, j.v_out, j.given, rs_given, rs, es,
                         temp[blockIdx.y]};
    }
    int jobs() const { return njobs; }
    const float* weights(int j) const { return job[j].W; }
    void set_wt(int j, const float* wt) { job[j].Wt = wt; }
    bool has_given() const { return job[0].given != nullptr; }
    bool complete(int j) const { return job[j].v0 && job[j].W && job[j].bh && job[j].bv && (job[j].given != nullptr) == has_given(); }
};

// The three forms.  Grid: x = row block, y = job.
template <typename Args, bool GIVEN>
__global__ void __launch_bounds__(256) rbm_gibbs_stream_kernel(Args A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_stream_body<GIVEN, Args::STRIDED, Args::TEMPERED>(A.view(), blockIdx.x * RBM_R, smem);
}
template <typename Args, bool GIVEN, int R, int RGH, int RGV>
__global__ void __launch_bounds__(256) rbm_gibbs_lds_kernel(Args A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_lds_body<R, RGH, RGV, GIVEN, Args::STRIDED, Args::TEMPERED>(A.view(), blockIdx.x * R, smem);
}
template <typename Args, bool GIVEN>
__global__ void __launch_bounds__(512) rbm_gibbs_mfma_kernel(Args A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_mfma_body<GIVEN, Args::STRIDED, Args::TEMPERED>(A.view(), blockIdx.x * GM_ROWS, smem);
}

extern "C" int mnn_transpose(mnn_stream_t s, const void* in, int in_dtype, int R, int C, int ld_in, void* out, int out_dtype, int ld_out);

// Launch KERNEL over (ceil(N / rows), jobs) workgroups.  Dynamic LDS above 64 KB has to be asked for once per instantiation and device; false
// (nothing launched) when that is refused.
template <auto KERNEL, typename Args>
static bool gibbs_launch(hipStream_t st, const Args& A, int rows, int threads, size_t lds) {
    static MnnPerDeviceOnce raised;
    if (mnn_once_per_device(raised, [] { return mnn_raise_dynamic_lds(reinterpret_cast<const void*>(KERNEL), 160 * 1024); }) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    hipLaunchKernelGGL(KERNEL, dim3(cdiv(A.N, rows), A.jobs()), dim3(threads), lds, st, A);
    return true;
}

// The choice of the form: the same one for a shape whether the launch is single or grouped, clamped or tempered (the clamped forms need no
// LDS beyond the free ones' except the streaming kernel's codes, which no threshold looks at).
template <bool GIVEN, typename Args>
static int rbm_gibbs_forms(const char* who, mnn_stream_t s, Args& A, void* workspace) {
    const int N = A.N, D = A.D, Hn = A.Hn;
    const size_t codes_lds = GIVEN ? (size_t)RBM_R * ((D + 3) & ~3) : 0;
    MNN_REQUIRE(rbm_lds_bytes(D, Hn) + codes_lds <= 160 * 1024, "%s: D+Hn too large for LDS", who);
    hipStream_t st = (hipStream_t)s;
    if (N < 2048 && Hn <= 256 && D <= 256 && rbm_lds_resident_bytes(2, D, Hn) <= 158 * 1024 && !mnn_switch_set(MNN_SW_RBM_STREAM_W)) {
        // sampling-sized batches: W resident in LDS, two rows per workgroup (one workgroup per CU: at training sizes -- 32 768 rows --
        // the streaming kernel's eight rows per workgroup and several workgroups per CU win, 1.5 vs 2.5 ms; round 3: also with the workgroup
        // walking over its row groups so that W is loaded once, 4.9 ms -- two rows per pass are two dependent fma chains per thread at one
        // wave per SIMD: latency-bound); rows per thread by how many row groups of n_out threads fit 256
        const int gh = 256 / Hn, gv = 256 / D;          // row groups available in the hidden / visible phase
        const size_t lds = rbm_lds_resident_bytes(2, D, Hn);
#define GIBBS_LDS(RGH, RGV) gibbs_launch<&rbm_gibbs_lds_kernel<Args, GIVEN, 2, RGH, RGV>>(st, A, 2, 256, lds)
        const bool done = gv >= 2 ? (gh >= 2 ? GIBBS_LDS(1, 1) : GIBBS_LDS(2, 1)) : (gh >= 2 ? GIBBS_LDS(1, 2) : GIBBS_LDS(2, 2));
#undef GIBBS_LDS
        if (done) {
            MNN_LAUNCH_CHECK();
            return MNN_OK;
        }
    }
    if (gibbs_mfma_lds_bytes(D, Hn) <= 158 * 1024 && !mnn_switch_set(MNN_SW_RBM_NO_MFMA)) {
        // training batches: the chain on the f32 matrix cores, 64 rows per workgroup (same draws: see rbm_gibbs_mfma_body)
        MNN_REQUIRE((gibbs_launch<&rbm_gibbs_mfma_kernel<Args, GIVEN>>(st, A, GM_ROWS, 512, gibbs_mfma_lds_bytes(D, Hn))), "%s: cannot raise the dynamic LDS limit", who);
        MNN_LAUNCH_CHECK();
        return MNN_OK;
    }
    // neither fits: the streaming chain, W and a transposed copy per job from L2
    for (int j = 0; j < A.jobs(); ++j) {
        float* wt = (float*)workspace + (size_t)j * D * Hn;
        int rc = mnn_transpose(s, A.weights(j), MNN_F32, D, Hn, Hn, wt, MNN_F32, D);
        if (rc != MNN_OK) return rc;
        A.set_wt(j, wt);
    }
    MNN_REQUIRE((gibbs_launch<&rbm_gibbs_stream_kernel<Args, GIVEN>>(st, A, RBM_R, 256, rbm_lds_bytes(D, Hn) + codes_lds)), "%s: cannot raise the dynamic LDS limit", who);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

// What every entry point requires of a filled block, then the launch.  `who`: the entry point, for the messages.
template <typename Args>
static int rbm_gibbs_dispatch(const char* who, mnn_stream_t s, Args& A, void* workspace) {
    MNN_REQUIRE(A.N > 0 && A.D > 0 && A.Hn > 0 && A.k >= 0, "%s: bad sizes N=%d D=%d Hn=%d k=%d", who, A.N, A.D, A.Hn, A.k);
    MNN_REQUIRE((A.ld_bh == 0 || A.ld_bh >= A.Hn) && (A.ld_bv == 0 || A.ld_bv >= A.D), "%s: bad bias leading dimension", who);
    MNN_REQUIRE(workspace, "%s: null workspace", who);
    for (int j = 0; j < A.jobs(); ++j)
        MNN_REQUIRE(A.complete(j), "%s: job %d: null pointer, or `given` set on some jobs only", who, j);
    return A.has_given() ? rbm_gibbs_forms<true>(who, s, A, workspace) : rbm_gibbs_forms<false>(who, s, A, workspace);
}

// ----------------------------------------------------------------------------------------------
// free energy, per row (rbm.py:256-258; R4):  F[n] = -sum_j softplus((vW)_j + bh[n,j]) - v.bv[n]
// smem: f32 [RBM_R][Dp]; fsum: __shared__ f32 [4][RBM_R] -- the four waves' partial sums, added in wave order: F has the same bits in every
// launch (and in a grouped launch) whichever wave finishes first
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplus_f(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }

__device__ __forceinline__ void rbm_free_energy_body(int N, int D, int Hn, const uint8_t* __restrict__ v, const float* __restrict__ W,
                                                     const float* __restrict__ bh, int ld_bh, const float* __restrict__ bv, int ld_bv,
                                                     float* __restrict__ F, float* __restrict__ p_h, const int n0, float* __restrict__ smem,
                                                     float* __restrict__ fsum) {
    const int Dp = (D + 3) & ~3;
    rbm_load_rows<uint8_t>(v, N, n0, D, Dp, smem);
    __syncthreads();
    float part[RBM_R];
#pragma unroll
    for (int r = 0; r < RBM_R; ++r) part[r] = 0.f;
    rbm_phase(smem, Dp, D, W, Hn, Hn, bh, ld_bh, n0, N, [&](int r, int j, float z) {
        const int n = n0 + r;
        if (n < N) {
            part[r] -= softplus_f(z);
            // d F / d z = -sigmoid(z): the backward pass's hidden activations, from the pre-activation this pass has anyway (the same
            // det_sigmoid as mnn_rbm_hidden, so the gradient keeps its bits; saves that pass re-reading v and W and re-forming z)
            if (p_h != nullptr) p_h[(size_t)n * Hn + j] = det_sigmoid(z);
        }
    });
    for (int d = threadIdx.x; d < D; d += blockDim.x)
#pragma unroll
        for (int r = 0; r < RBM_R; ++r) {
            const int n = n0 + r;
            if (n < N) part[r] -= smem[r * Dp + d] * bv[(size_t)n * ld_bv + d];
        }
#pragma unroll
    for (int r = 0; r < RBM_R; ++r) {
        float x = part[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if ((threadIdx.x & 63) == 0) fsum[(threadIdx.x >> 6) * RBM_R + r] = x;
    }
    __syncthreads();
    if (threadIdx.x < RBM_R && n0 + threadIdx.x < N)
        F[n0 + threadIdx.x] = ((fsum[threadIdx.x] + fsum[RBM_R + threadIdx.x]) + fsum[2 * RBM_R + threadIdx.x]) + fsum[3 * RBM_R + threadIdx.x];
}
