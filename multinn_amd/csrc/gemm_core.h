// MFMA GEMM core for gfx950, shared by the GEMM kernels (gemm.hip) and the launch-per-timestep LSTM step kernels (lstm_seq.hip).
//
// T = bf16 / f16 -> v_mfma_f32_32x32x16_{bf16,f16} ; T = f32 -> v_mfma_f32_32x32x2_f32 (exact f32 fma chain).
// Tiles are staged global -> registers -> LDS (double buffered); an LDS row holds one 64-byte
// K-chunk (32 bf16 / 16 f32) padded to 80 bytes so that the 16 rows a ds_read_b128 lane group
// touches fall on 16 distinct 16-byte slots (conflict-free, MI355X_MICROARCH "LDS").
#pragma once
#include "common.h"
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// (LDS tile rows: GemmCore::ROW = bytes of K per stage + 16 B pad)
#define CHUNK_B 64   // bytes of K per row per stage

template <typename T> struct Elem;
template <> struct Elem<bf16_t> { static constexpr int PER16 = 8; static constexpr int PER_CHUNK = 32; };
template <> struct Elem<f16_t>  { static constexpr int PER16 = 8; static constexpr int PER_CHUNK = 32; };
template <> struct Elem<float>  { static constexpr int PER16 = 4; static constexpr int PER_CHUNK = 32; };      // f32 stages 128 B of K per row (below)

// KH = 2 (f32 only): the workgroup has a second set of WM x WN waves that takes the other half of every K chunk (the step kernels of the f32
// recurrence: one wave per 32 x 128 tile put 512 waves on 1024 SIMDs -- half of the f32 matrix-core rate at best); reduce_kh() adds the halves.
template <typename T, int BM, int BN, int WM, int WN, int KH = 1>
struct GemmCore {
    static constexpr int NT = WM * WN * KH * 64;
    static constexpr int TM = BM / WM / 32;
    static constexpr int TN = BN / WN / 32;
    // bytes of K per tile row and stage: 64 for the 16-bit types (32 k), 128 for f32 (32 k: with 16 k a wave had 4 .. 32 MFMAs between two
    // workgroup barriers and the step kernels of the f32 recurrence were barrier-bound); ROW = its LDS pitch (+ 16 B pad), P = 16-byte pieces
    static constexpr int RB = sizeof(T) == 4 ? 128 : 64, ROW = RB + 16, P = RB / 16;
    static constexpr int A_CHUNKS = (BM * P + NT - 1) / NT;   // 16-byte pieces per thread per stage
    static constexpr int B_CHUNKS = (BN * P + NT - 1) / NT;
    static constexpr int LDS_BYTES = 2 * (BM + BN) * ROW;
    static_assert(BM % (WM * 32) == 0 && BN % (WN * 32) == 0, "tile/wave mismatch");
    static_assert(KH == 1 || (KH == 2 && sizeof(T) == 4), "the in-workgroup K split is built for f32 operands");
    static_assert(KH == 1 || WM * WN * 16 * 64 * 4 <= LDS_BYTES, "reduce_kh stages one tile per wave in the stage buffers");

    uint4 ra[A_CHUNKS], rb[B_CHUNKS];

    __device__ __forceinline__ void gload(const T* __restrict__ A, int lda, int M, int m0, const T* __restrict__ B, int ldb,
                                          int N, int n0, int K, int k0, int tid) {
#pragma unroll
        for (int s = 0; s < A_CHUNKS; ++s) {
            const int idx = tid + s * NT, row = min(idx / P, BM - 1), c = idx % P;     // (BM * P < NT: the surplus threads repeat the last row)
            const int gr = m0 + row, gk = k0 + c * Elem<T>::PER16;
            ra[s] = (gr < M && gk < K) ? *reinterpret_cast<const uint4*>(A + (size_t)gr * lda + gk) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < B_CHUNKS; ++s) {
            const int idx = tid + s * NT, row = min(idx / P, BN - 1), c = idx % P;
            const int gr = n0 + row, gk = k0 + c * Elem<T>::PER16;
            rb[s] = (gr < N && gk < K) ? *reinterpret_cast<const uint4*>(B + (size_t)gr * ldb + gk) : make_uint4(0, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void lstore(char* sA, char* sB, int tid) {
#pragma unroll
        for (int s = 0; s < A_CHUNKS; ++s) {
            const int idx = tid + s * NT, row = min(idx / P, BM - 1), c = idx % P;     // (surplus threads store the same bytes again)
            *reinterpret_cast<uint4*>(sA + row * ROW + c * 16) = ra[s];
        }
#pragma unroll
        for (int s = 0; s < B_CHUNKS; ++s) {
            const int idx = tid + s * NT, row = min(idx / P, BN - 1), c = idx % P;
            *reinterpret_cast<uint4*>(sB + row * ROW + c * 16) = rb[s];
        }
    }
    // one 64-byte K-chunk of MFMAs for this wave
    __device__ __forceinline__ void compute(const char* sA, const char* sB, int wm, int wn, int lane, f32x16_t (&acc)[TM][TN], int kh = 0) {
        const int r = lane & 31, h = lane >> 5;
        const char* pa = sA + (wm * (BM / WM) + r) * ROW;
        const char* pb = sB + (wn * (BN / WN) + r) * ROW;
        if constexpr (sizeof(T) == 2) {
            using F = typename FlavorOf<T>::type;
            using V8 = typename F::x8;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                V8 a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const V8*>(pa + i * 32 * ROW + ks * 32 + h * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const V8*>(pb + j * 32 * ROW + ks * 32 + h * 16);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = F::mfma32(a[i], b[j], acc[i][j]);
            }
        } else {
            // K order inside the 32-k chunk is permuted (lane half h owns k = 16 h .. 16 h + 15) so each lane reads contiguous bytes; A and B use
            // the same permutation, so the product is unchanged.  KH == 2: this wave multiplies half of that, k = 16 h + 8 kh .. + 7.
            constexpr int NV = 4 / KH;                   // 16-byte pieces per lane, tile row and chunk
            f32x4_t a[TM][NV], b[TN][NV];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int v = 0; v < NV; ++v) a[i][v] = *reinterpret_cast<const f32x4_t*>(pa + i * 32 * ROW + h * 64 + kh * (NV * 16) + v * 16);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int v = 0; v < NV; ++v) b[j][v] = *reinterpret_cast<const f32x4_t*>(pb + j * 32 * ROW + h * 64 + kh * (NV * 16) + v * 16);
#pragma unroll
            for (int ks = 0; ks < 4 * NV; ++ks)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][ks >> 2][ks & 3], b[j][ks >> 2][ks & 3], acc[i][j], 0, 0, 0);
        }
    }

    // full K loop [kc0, kc1) in chunk units; acc must be initialised by the caller
    __device__ __forceinline__ void run(const T* __restrict__ A, int lda, int M, int m0, const T* __restrict__ B, int ldb, int N,
                                        int n0, int K, int kc0, int kc1, char* smem, f32x16_t (&acc)[TM][TN]) {
        const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int kh = wave / (WM * WN), wq = wave % (WM * WN);
        const int wm = wq / WN, wn = wq % WN;
        char* sA[2] = {smem, smem + (BM + BN) * ROW};
        char* sB[2] = {smem + BM * ROW, smem + (BM + BN) * ROW + BM * ROW};
        if (kc0 >= kc1) return;
        gload(A, lda, M, m0, B, ldb, N, n0, K, kc0 * Elem<T>::PER_CHUNK, tid);
        lstore(sA[0], sB[0], tid);
        __syncthreads();
        int cur = 0;
        for (int kc = kc0; kc < kc1; ++kc) {
            const bool more = kc + 1 < kc1;
            if (more) gload(A, lda, M, m0, B, ldb, N, n0, K, (kc + 1) * Elem<T>::PER_CHUNK, tid);
            compute(sA[cur], sB[cur], wm, wn, lane, acc, kh);
            if (more) lstore(sA[cur ^ 1], sB[cur ^ 1], tid);
            __syncthreads();
            cur ^= 1;
        }
    }
    // KH == 2, after run() (its last barrier has freed the stage buffers): the second wave set's partial tiles are added into the first set's,
    // tile by tile through `smem`.  Returns true for the waves that now hold the sums (the epilogue is theirs; wave % (WM WN) is their tile slot).
    __device__ __forceinline__ bool reduce_kh(char* smem, f32x16_t (&acc)[TM][TN]) {
        if constexpr (KH == 1) return true;
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int kh = wave / (WM * WN), wq = wave % (WM * WN);
        float* red = reinterpret_cast<float*>(smem) + wq * 16 * 64;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (i + j > 0) __syncthreads();
                if (kh == 1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[r * 64 + lane] = acc[i][j][r];
                }
                __syncthreads();
                if (kh == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] += red[r * 64 + lane];
                }
            }
        return kh == 0;
    }
};

// C/D fragment coordinates of a 32x32 MFMA tile: reg r of lane l -> (row, col)
__device__ __forceinline__ int frag_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// LDS-DMA (global_load_lds) operand pointers
typedef __attribute__((address_space(1))) const void* gas_ptr_t;
typedef __attribute__((address_space(3))) void* lds_ptr_t;
