// The GEMM kernels for gfx950, their epilogues and launcher (the tile core: gemm_core.h).
//
//   C[M,N] (op)= A[M,K] . B[N,K]^T        both operands K-contiguous
#include "gemm_core.h"
typedef unsigned gm_u4 __attribute__((ext_vector_type(4)));

// 16-bit C outputs: the mnn_dtype code of C (MNN_F32 = plain f32) travels as `c16`; a 16-bit value is converted by its own flavour
__device__ __forceinline__ h16_t cvt_c16(float v, int c16) { return c16 == MNN_F16 ? f32_to_f16(v) : f32_to_bf16(v); }

// ----------------------------------------------------------------------------------------------
// plain GEMM
// ----------------------------------------------------------------------------------------------
template <typename T, int BM, int BN, int WM, int WN, int KH = 1>
__global__ void __launch_bounds__(WM * WN * KH * 64)
gemm_tn_kernel(const T* __restrict__ A, int lda, const T* __restrict__ B, int ldb, void* __restrict__ Cv, int ldc, int c_bf16,
               const float* __restrict__ bias, int M, int N, int K, int flags, int split_k, int ntm, int ntn) {
    using Core = GemmCore<T, BM, BN, WM, WN, KH>;
    extern __shared__ __attribute__((aligned(16))) char gemm_tn_smem[];      // Core::LDS_BYTES (f32: 72 KB, past the static limit)
    char* smem = gemm_tn_smem;
    // XCD-aware tile order: blocks b and b+8 share an XCD (speed only); give each XCD one m-panel
    // for all n-tiles so the A panel stays in that XCD's L2.
    const int bid = blockIdx.x;
    const int grp = bid / (8 * ntn), within = bid % (8 * ntn);
    const int mt = grp * 8 + (within & 7), nt = within >> 3;
    if (mt >= ntm) return;
    const int m0 = mt * BM, n0 = nt * BN;
    const int nchunks = (K + Elem<T>::PER_CHUNK - 1) / Elem<T>::PER_CHUNK;
    const int z = blockIdx.y;
    const int per = (nchunks + split_k - 1) / split_k;
    const int kc0 = z * per, kc1 = min(nchunks, kc0 + per);
    f32x16_t acc[Core::TM][Core::TN];
#pragma unroll
    for (int i = 0; i < Core::TM; ++i)
#pragma unroll
        for (int j = 0; j < Core::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    Core core;
    core.run(A, lda, M, m0, B, ldb, N, n0, K, kc0, kc1, smem, acc);
    if (kc0 >= kc1 && z > 0) return;                     // (uniform over the workgroup)
    if (!core.reduce_kh(smem, acc)) return;              // KH == 2: the second wave set's halves are added in; the first set owns the epilogue

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;
    float* Cf = reinterpret_cast<float*>(Cv);
    bf16_t* Cb = reinterpret_cast<bf16_t*>(Cv);
#pragma unroll
    for (int i = 0; i < Core::TM; ++i)
#pragma unroll
        for (int j = 0; j < Core::TN; ++j) {
            const int col = n0 + wn * (BN / WN) + j * 32 + (lane & 31);
            if (col >= N) continue;
            const float bv = (bias != nullptr && z == 0) ? bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * (BM / WM) + i * 32 + frag_row(r, lane);
                if (row >= M) continue;
                const float val = acc[i][j][r] + bv;
                const size_t o = (size_t)row * ldc + col;
                if (c_bf16) {
                    Cb[o] = cvt_c16(val, c_bf16);
                } else if (flags & MNN_GEMM_ATOMIC) {
                    atomicAdd(Cf + o, val);
                } else if (flags & MNN_GEMM_ACCUMULATE) {
                    Cf[o] += val;
                } else {
                    Cf[o] = val;
                }
            }
        }
}


// ----------------------------------------------------------------------------------------------
// bf16 GEMM, direct-to-LDS staging (global_load_lds_dwordx4): 128x128 tile, BK = 64, 4 waves (2x2),
// two LDS buffers, one barrier per K-tile.  An LDS-DMA wave-instruction writes 64 lanes x 16 B = 1 KiB
// LINEARLY (8 tile rows of 128 B), so the tile image cannot be padded; bank conflicts of the
// ds_read_b128 fragment reads are removed by an XOR swizzle applied on the per-lane SOURCE address and
// again on the read (cdna_hip_programming.md rule 21).  BK = 64 (128-byte tile rows) by default, BK = 128 for the
// tall-K weight-gradient GEMMs.  Requires K % 64 == 0 (operands are zero-padded by the callers).
// ----------------------------------------------------------------------------------------------

// CPR = 16-byte chunks per tile row (8 for BK = 64, 16 for BK = 128); swizzle: chunk c of row r lives at
// c ^ ((r >> 1) & 7) for 128-byte rows and c ^ (r & 15) for 256-byte rows (16 rows of a ds_read_b128 group -> 16 slots).

// Epilogue of the LDS-DMA kernels: one wave's NI x NJ accumulator tiles -> C.  The store mode is resolved ONCE (template), the row
// part of every address is wave-uniform (scalar arithmetic), the per-lane part is one offset computed once.  The per-element form
// (64-bit row * ldc per lane, four run-time mode branches per element) cost ~40 instructions per stored value: at K = 448 the
// 256 x 256 tile spent 21 of its 35 us issuing its 128 stores per thread (profiles/tools/gemm_trace.hip) -- 150 -> 89 us for xproj1.
enum { EPI_STORE = 0, EPI_ATOMIC = 1, EPI_ACCUM = 2, EPI_BF16 = 3, EPI_F16 = 4 };
template <int MODE>
__device__ __forceinline__ void epi_put(float* __restrict__ rowf, bf16_t* __restrict__ rowb, unsigned lane_off, float val) {
    // rowf / rowb are wave-uniform pointers (SGPR base), lane_off the one per-lane offset: the store needs no vector address arithmetic
    if (MODE == EPI_BF16) rowb[lane_off] = f32_to_bf16(val);
    else if (MODE == EPI_F16) rowb[lane_off] = f32_to_f16(val);
    else if (MODE == EPI_ATOMIC) atomicAdd(rowf + lane_off, val);
    else if (MODE == EPI_ACCUM) rowf[lane_off] += val;
    else rowf[lane_off] = val;
}
template <int MODE, int NI, int NJ>
__device__ __forceinline__ void epi_store_tiles(void* __restrict__ Cv, int ldc, int M, int N, int row0, int col0, const f32x16_t (&acc)[NI][NJ],
                                                const float* __restrict__ bias, int lane) {
    const int r = lane & 31, h4 = 4 * (lane >> 5);
    float* Cf = reinterpret_cast<float*>(Cv);
    bf16_t* Cb = reinterpret_cast<bf16_t*>(Cv);
    const unsigned lane_off = (unsigned)h4 * (unsigned)ldc + (unsigned)r;
    if (row0 + NI * 32 <= M && col0 + NJ * 32 <= N) {          // interior (uniform): no predicates at all
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float bv = bias != nullptr ? bias[col0 + j * 32 + r] : 0.f;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const size_t ro = (size_t)(row0 + i * 32 + (e & 3) + 8 * (e >> 2)) * ldc + col0 + j * 32;      // uniform
                    epi_put<MODE>(Cf + ro, Cb + ro, lane_off, acc[i][j][e] + bv);
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = col0 + j * 32;                          // uniform
        if (cb >= N) continue;
        const bool colok = cb + r < N;
        const float bv = (bias != nullptr && colok) ? bias[cb + r] : 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rb = row0 + i * 32 + (e & 3) + 8 * (e >> 2);      // uniform: this register's row for lanes 0..31 (lanes 32..63: +4)
                if (rb >= M) continue;
                if (colok && rb + h4 < M) {
                    const size_t ro = (size_t)rb * ldc + cb;
                    epi_put<MODE>(Cf + ro, Cb + ro, lane_off, acc[i][j][e] + bv);
                }
            }
        }
    }
}
// Wide form for plain / bf16 stores of an interior wave tile: every 32 x 32 accumulator tile is turned round through a wave-private LDS
// tile ([32][36] f32: the stage buffers are idle after the K loop) so that a lane holds consecutive COLUMNS, and leaves as 16-byte stores
// covering whole 128-byte rows (f32: 4 stores of 8 rows x 128 B per tile; bf16: 2 stores of 16 rows x 64 B) instead of sixteen 4- / 2-byte
// stores per lane.  A CU issues stores at a fixed instruction rate whatever their width (the element-wise epilogue of a 256 x 256 f32 tile:
// 128 store instructions per lane, ~11 us at K = 448 next to ~12 us of K loop), so the bytes per instruction are what counts.
#define EPI_SC_FLOATS 1152        // per-wave scratch: 32 rows x 36 floats
#ifndef EPI_WIDE
#define EPI_WIDE 1
#endif
template <int MODE, int NI, int NJ>
__device__ __forceinline__ void epi_store_wide(void* __restrict__ Cv, int ldc, int row0, int col0, const f32x16_t (&acc)[NI][NJ],
                                               const float* __restrict__ bias, int lane, float* __restrict__ sc) {
    const int r = lane & 31, hh = lane >> 5;
    float* Cf = reinterpret_cast<float*>(Cv);
    bf16_t* Cb = reinterpret_cast<bf16_t*>(Cv);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float bv = bias != nullptr ? bias[col0 + j * 32 + r] : 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[((e & 3) + 8 * (e >> 2) + 4 * hh) * 36 + r] = acc[i][j][e] + bv;
            asm volatile("" ::: "memory");
            if (MODE == EPI_BF16 || MODE == EPI_F16) {
                using CF = typename std::conditional<MODE == EPI_F16, Fp16F, Bf16F>::type;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int row = 16 * p + (lane >> 2), c8 = 8 * (lane & 3);
                    const float4 v0 = *reinterpret_cast<const float4*>(sc + row * 36 + c8);
                    const float4 v1 = *reinterpret_cast<const float4*>(sc + row * 36 + c8 + 4);
                    uint4 pk;
                    pk.x = pack2<CF>(v0.x, v0.y);
                    pk.y = pack2<CF>(v0.z, v0.w);
                    pk.z = pack2<CF>(v1.x, v1.y);
                    pk.w = pack2<CF>(v1.z, v1.w);
                    // NON-TEMPORAL (also below): the activation GEMMs' C is written once and read by a later kernel; with the default policy it pushes the
                    // operand panels the tiles of a row share through the L2 out (Dense forward 240 -> 212 us, xproj1 on this kernel 745 -> 605 us)
                    __builtin_nontemporal_store(__builtin_bit_cast(gm_u4, pk), reinterpret_cast<gm_u4*>(Cb + (size_t)(row0 + i * 32 + row) * ldc + col0 + j * 32 + c8));
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int row = 8 * p + (lane >> 3), c4 = 4 * (lane & 7);
                    __builtin_nontemporal_store(*reinterpret_cast<const gm_u4*>(sc + row * 36 + c4), reinterpret_cast<gm_u4*>(Cf + (size_t)(row0 + i * 32 + row) * ldc + col0 + j * 32 + c4));
                }
            }
            asm volatile("" ::: "memory");
        }
    }
}
template <int NI, int NJ>
__device__ __forceinline__ void epi_dispatch(void* __restrict__ Cv, int ldc, int c_bf16, int flags, int M, int N, int row0, int col0,
                                             const f32x16_t (&acc)[NI][NJ], const float* __restrict__ bias, int lane, float* __restrict__ sc = nullptr) {
    if (sc != nullptr && !(flags & (MNN_GEMM_ATOMIC | MNN_GEMM_ACCUMULATE)) && row0 + NI * 32 <= M && col0 + NJ * 32 <= N &&
        ((size_t)Cv & 15) == 0 && (ldc & (c_bf16 ? 7 : 3)) == 0) {               // all wave-uniform
        if (c_bf16 == MNN_F16) epi_store_wide<EPI_F16, NI, NJ>(Cv, ldc, row0, col0, acc, bias, lane, sc);
        else if (c_bf16) epi_store_wide<EPI_BF16, NI, NJ>(Cv, ldc, row0, col0, acc, bias, lane, sc);
        else epi_store_wide<EPI_STORE, NI, NJ>(Cv, ldc, row0, col0, acc, bias, lane, sc);
        return;
    }
    if (c_bf16 == MNN_F16) epi_store_tiles<EPI_F16, NI, NJ>(Cv, ldc, M, N, row0, col0, acc, bias, lane);
    else if (c_bf16) epi_store_tiles<EPI_BF16, NI, NJ>(Cv, ldc, M, N, row0, col0, acc, bias, lane);
    else if (flags & MNN_GEMM_ATOMIC) epi_store_tiles<EPI_ATOMIC, NI, NJ>(Cv, ldc, M, N, row0, col0, acc, bias, lane);
    else if (flags & MNN_GEMM_ACCUMULATE) epi_store_tiles<EPI_ACCUM, NI, NJ>(Cv, ldc, M, N, row0, col0, acc, bias, lane);
    else epi_store_tiles<EPI_STORE, NI, NJ>(Cv, ldc, M, N, row0, col0, acc, bias, lane);
}

template <int CPR>
__device__ __forceinline__ int swz(int row) { return CPR == 8 ? ((row >> 1) & 7) : (CPR == 4 ? ((row >> 2) & 3) : (row & 15)); }

// This thread's LDS-DMA slots of one operand tile (ROWS rows x CPR 16-byte chunks, NW waves): the global address of every slot at
// k = 0 is computed ONCE per workgroup (row clamp, swizzle, 64-bit row * ld); staging a K tile is then one 64-bit add per slot.
// Recomputing them per K tile cost ~0.5 us of address arithmetic per tile in front of the 8 DMA instructions (profiles/tools/gemm_trace.hip).
// KB = the operand is stored K-BLOCKED: element (row, k) at ((k >> 5) * ld + row) * 32 + (k & 31), ld = its total row count -- 32 consecutive k of
// one row are 64 contiguous bytes, and the 32 k of all rows of a block are one contiguous slab.  A producer that owns a (32-k block, row
// range) -- the backward recurrence: 32 batch rows of one timestep x its 128 gate columns -- writes its piece of dz^T as whole contiguous
// kilobytes instead of one 32-byte run per row (rows 512 KB apart).  The LDS image and everything behind it are the same as for the plain
// K-contiguous operand (BK = 64 = two blocks: chunks 0..3 from block 2 kt, chunks 4..7 from block 2 kt + 1).
template <int ROWS, int NW, int CPR, bool KB = false>
struct GldsSlots {
    static constexpr int NS = ROWS * CPR / (64 * NW);
    const bf16_t* base;                                    // wave-uniform
    unsigned off[NS];                                       // element offset of the slot at k = 0 (operands stay below 2^31 elements)
    unsigned kmul;                                          // KB: elements per unit of k0 (= ld); plain: 1
    __device__ __forceinline__ void init(const bf16_t* __restrict__ G, int ld, int rows_total, int r0, int wave, int lane) {
        static_assert(!KB || CPR == 8, "the K-blocked layout is defined for 64-deep K tiles");
        base = G;
        kmul = KB ? (unsigned)ld : 1u;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int p = (s * NW + wave) * 64 + lane;      // linear 16-byte slot of the tile image
            const int row = p / CPR, pc = p % CPR;
            const int c = pc ^ swz<CPR>(row);               // logical K chunk held by this slot
            const int gr = min(r0 + row, rows_total - 1);   // rows past the edge replicate the last row (never stored)
            if (KB) off[s] = ((unsigned)(c >> 2) * (unsigned)ld + (unsigned)gr) * 32u + (unsigned)((c & 3) * 8);
            else off[s] = (unsigned)gr * (unsigned)ld + (unsigned)(c * 8);
        }
    }
    __device__ __forceinline__ void stage(int k0, char* tile, int wave) const {
        const bf16_t* b = base + (size_t)k0 * kmul;         // wave-uniform (K-blocked: 64 k = two blocks = 64 ld elements)
#pragma unroll
        for (int s = 0; s < NS; ++s)
            __builtin_amdgcn_global_load_lds((gas_ptr_t)(b + off[s]), (lds_ptr_t)(tile + (s * NW + wave) * 1024), 16, 0, 0);
    }
};

// Split-K work mapping.  The hardware deals consecutive workgroup ids round-robin over the 8 XCDs (xcd = id % 8).  All tiles that read the same
// K slice should run on ONE XCD, so that the slice's A and B panels are fetched into that L2 once and the other tiles hit.  `z = id % split_k`
// achieves that when split_k is a multiple of 8 (or the real tiles sit at multiples of 8 in the slot order: a single row group).  For other
// slice counts XCD x owns the CONTIGUOUS range [x T / 8, (x + 1) T / 8) of the slice-major order (item = z * slots + tile); the grid's x
// extent is a multiple of 8 workgroups, so T % 8 == 0.  Measured, [1024 x 768] weight gradient, K = 262144, split 20: 708 -> 399 us (split
// 16: 456 either way).  Not used for multiples of 8: [256 x 704] at split 64 takes 159 us with id % split_k and 349 us contiguous.
#define GEMM_SPLITK_CONTIG 0x100         // internal flag bit (set by the launcher): the mapping below; clear: z = id % split_k
__device__ __forceinline__ void splitk_item(int split_k, int flags, int& z, int& bid) {
    const int lin = blockIdx.x + blockIdx.y * gridDim.x;
    if (!(flags & GEMM_SPLITK_CONTIG)) { z = lin % split_k; bid = lin / split_k; return; }
    const int slots = gridDim.x, per_xcd = (slots * split_k) >> 3;
    const int item = (lin & 7) * per_xcd + (lin >> 3);
    z = item / slots;
    bid = item - z * slots;
}

template <int BK, typename F>
__global__ void __launch_bounds__(256)
gemm_tn_glds_kernel(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ B, int ldb, void* __restrict__ Cv, int ldc, int c_bf16,
                    const float* __restrict__ bias, int M, int N, int K, int flags, int split_k, int ntm, int ntn) {
    constexpr int CPR = BK / 8, ROWB = BK * 2, TILE = 128 * ROWB;
    __shared__ __attribute__((aligned(16))) char smem[2][2][TILE];
    int z, bid;
    splitk_item(split_k, flags, z, bid);               // the tiles that share an XCD read the same K slice of A and B: the re-reads hit that XCD's L2
    const int grp = bid / (8 * ntn), within = bid % (8 * ntn);
    const int mt = grp * 8 + (within & 7), nt = within >> 3;
    if (mt >= ntm) return;
    const int m0 = mt * 128, n0 = nt * 128;
    const int nkt = K / BK;
    const int per = (nkt + split_k - 1) / split_k;
    const int kt0 = z * per, kt1 = min(nkt, kt0 + per);
    if (kt0 >= kt1) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    GldsSlots<128, 4, CPR> slotA, slotB;
    slotA.init(A, lda, M, m0, wave, lane);
    slotB.init(B, ldb, N, n0, wave, lane);
    slotA.stage(kt0 * BK, smem[0][0], wave);
    slotB.stage(kt0 * BK, smem[0][1], wave);
    __syncthreads();                                        // hipcc drains vmcnt(0) before the barrier
    int cur = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        if (kt + 1 < kt1) {
            slotA.stage((kt + 1) * BK, smem[cur ^ 1][0], wave);
            slotB.stage((kt + 1) * BK, smem[cur ^ 1][1], wave);
        }
        const char* sA = smem[cur][0];
        const char* sB = smem[cur][1];
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            typename F::x8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = wm * 64 + i * 32 + r;
                a[i] = *reinterpret_cast<const typename F::x8*>(sA + row * ROWB + (((ks * 2 + h) ^ swz<CPR>(row)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int row = wn * 64 + j * 32 + r;
                b[j] = *reinterpret_cast<const typename F::x8*>(sB + row * ROWB + (((ks * 2 + h) ^ swz<CPR>(row)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = F::mfma32(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
        cur ^= 1;
    }
    epi_dispatch<2, 2>(Cv, ldc, c_bf16, flags, M, N, m0 + wm * 64, n0 + wn * 64, acc, z == 0 ? bias : nullptr, lane,
                       EPI_WIDE ? reinterpret_cast<float*>(&smem[0][0][0]) + wave * EPI_SC_FLOATS : nullptr);      // the K loop ended with a barrier
}

// ----------------------------------------------------------------------------------------------
// Large-tile variant: 256 x 256 x 64 per workgroup, 8 waves as 2 (M) x 4 (N), wave tile 128 x 64 = 4 x 2 MFMA tiles.
// The 128 x 128 kernel above reads one LDS fragment per MFMA (2 A + 2 B fragments feed 4 MFMAs) and stages 0.5 KiB of
// operands per MFMA through LDS-DMA: 1.5 KiB of LDS traffic per 32-cycle MFMA against a 128 B/clk LDS -- it is LDS-bound
// at two thirds of the MFMA rate before any latency.  Here 4 A + 2 B fragments feed 8 MFMAs and a stage carries 0.25 KiB
// per MFMA: 1.0 KiB per MFMA, and one workgroup per CU holds two 64 KiB stages.
// ----------------------------------------------------------------------------------------------
#ifdef GM_TRACE      // development only (profiles/tools/gemm_trace.hip): phase clocks of workgroup GM_TRACE, accumulated in 10 ns units
__device__ long long gm_trace[16];
#define GM_T(k) do { if (threadIdx.x == 0 && blockIdx.x == GM_TRACE && blockIdx.y == 0) { const long long now_ = wall_clock64(); gm_trace[k] += now_ - gmprev_; gmprev_ = now_; } } while (0)
#define GM_T0() long long gmprev_ = wall_clock64()
#else
#define GM_T(k) do { } while (0)
#define GM_T0() do { } while (0)
#endif
template <typename F, bool AKB = false>
__global__ void __launch_bounds__(512)
gemm_tn_glds256_kernel(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ B, int ldb, void* __restrict__ Cv, int ldc, int c_bf16,
                       const float* __restrict__ bias, int M, int N, int K, int flags, int split_k, int ntm, int ntn,
                       const int* __restrict__ m_rows_dev, const int* __restrict__ k_rows_dev) {
    constexpr int BK = 64, CPR = 8, ROWB = 128, TILE = 256 * ROWB;
    extern __shared__ __attribute__((aligned(16))) char smem256[];        // [stage][A | B][256 rows x 128 B]
    int z, bid;
    splitk_item(split_k, flags, z, bid);
    const int grp = bid / (8 * ntn), within = bid % (8 * ntn);
    const int mt = grp * 8 + (within & 7), nt = within >> 3;
    if (mt >= ntm) return;
    const int m0 = mt * 256, n0 = nt * 256;
    // compacted ragged batches (mnn_gemm_tn_rows): only the first *m_rows_dev rows of A (of C) / the first *k_rows_dev of the K dimension carry
    // data -- row tiles past the count leave (their C rows are never read), the K loop stops at the count (what lies behind it is zero)
    if (m_rows_dev != nullptr && m0 >= *m_rows_dev) return;
    const int nkt = k_rows_dev != nullptr ? min(K / BK, (*k_rows_dev + BK - 1) / BK) : K / BK;
    const int per = (nkt + split_k - 1) / split_k;
    const int kt0 = z * per, kt1 = min(nkt, kt0 + per);
    // An empty slice leaves -- except slice 0 of a product whose hinted K extent is 0 tiles and whose C is not only added to: it still owes C
    // the value every other kernel gives for an all-zero K range (bias, or zeros), so it runs its epilogue on zero accumulators and stages
    // nothing.  (Adding into C without a bias is a no-op: the weight gradients of an empty window leave here as before.)
    if (kt0 >= kt1 && (nkt > 0 || z != 0 || (bias == nullptr && (flags & (MNN_GEMM_ACCUMULATE | MNN_GEMM_ATOMIC))))) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int r = lane & 31, h = lane >> 5;
    f32x16_t acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    GldsSlots<256, 8, CPR, AKB> slotA;
    GldsSlots<256, 8, CPR> slotB;
    slotA.init(A, lda, M, m0, wave, lane);
    slotB.init(B, ldb, N, n0, wave, lane);
    auto stage = [&](int buf, int kt) {
        slotA.stage(kt * BK, smem256 + (buf * 2 + 0) * TILE, wave);
        slotB.stage(kt * BK, smem256 + (buf * 2 + 1) * TILE, wave);
    };
    GM_T0();
    if (kt0 < kt1) stage(0, kt0);                           // (uniform; false only for the zero-extent K hint above)
    __syncthreads();                                        // hipcc drains vmcnt(0) before the barrier
    GM_T(1);
    int cur = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        // (spreading these 8 DMA instructions over the four k-steps was measured: the 0.6 us they hold the wave moves into the k-steps --
        // 256 x 256 x 448 tile: issue 4.3 -> 1.4 us, LDS reads + MFMA 8.9 -> 10.2, barriers 1.8 -> 2.6: the K tile stays at ~2 us, LDS-bound)
#ifndef ABL_NODMA
        if (kt + 1 < kt1) stage(cur ^ 1, kt + 1);
#endif
        GM_T(2);
        const char* sA = smem256 + (cur * 2 + 0) * TILE;
        const char* sB = smem256 + (cur * 2 + 1) * TILE;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            typename F::x8 a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wm * 128 + i * 32 + r;
                a[i] = *reinterpret_cast<const typename F::x8*>(sA + row * ROWB + (((ks * 2 + h) ^ swz<CPR>(row)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int row = wn * 64 + j * 32 + r;
                b[j] = *reinterpret_cast<const typename F::x8*>(sB + row * ROWB + (((ks * 2 + h) ^ swz<CPR>(row)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#ifndef ABL_NOMFMA
                    acc[i][j] = F::mfma32(a[i], b[j], acc[i][j]);
#else
                    asm volatile("" :: "v"(a[i]), "v"(b[j]));
#endif
                }
        }
        GM_T(3);
        __syncthreads();
        GM_T(4);
        cur ^= 1;
    }
    epi_dispatch<4, 2>(Cv, ldc, c_bf16, flags, M, N, m0 + wm * 128, n0 + wn * 64, acc, z == 0 ? bias : nullptr, lane,
                       EPI_WIDE ? reinterpret_cast<float*>(smem256) + wave * EPI_SC_FLOATS : nullptr);             // the K loop ended with a barrier
    GM_T(5);
#ifdef GM_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GM_T(6);
#endif
}

int mnn_gemm_bres_ok(int M, int N, int K);                      // gemm_bres.hip (internal: not part of the C ABI)
// MNN_GEMM_BRES=0: the LDS-staged kernels for these shapes too -- the comparison partner of the weight-resident form in
// tests/test_gpu_kernels.py (one process runs both: switches are read per call)
static bool gemm_bres_enabled() { return mnn_switch_int(MNN_SW_GEMM_BRES, 1) != 0; }
int mnn_gemm_bres_launch(hipStream_t st, int f16, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc, const float* bias);

template <typename T>
static int launch_gemm(hipStream_t st, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                       int c_bf16, const float* bias, int flags, int split_k, const int* m_rows_dev = nullptr, const int* k_rows_dev = nullptr) {
    constexpr int BM = 128, BN = 128;
    const int ntm = cdiv(M, BM), ntn = cdiv(N, BN);
    const int ngrp = cdiv(ntm, 8);
    dim3 grid(ngrp * 8 * ntn, split_k);
    if constexpr (sizeof(T) == 2) {
        // large problems: 256 x 256 tiles (enough of them to occupy the chip, each with enough K tiles to amortise its prologue)
        const int ntm2 = cdiv(M, 256), ntn2 = cdiv(N, 256);
        const bool no256 = mnn_switch_set(MNN_SW_GEMM_NO256);
        // A persistent ring form of this tile (4 LDS slots of 32-deep sub-tiles, counted vmcnt, raw barriers) was measured in round 3 and is NOT
        // shipped (profiles/round3_b_gemm_ablation.md): slower on K = 448 .. 1024 and on the K = 262144 weight gradients, because the operand
        // stream arrives at ~34 GB/s per CU whatever is in flight; its one win (K = 256, the Dense forward) needs an N-edge epilogue at N = 704.
        if (flags & MNN_GEMM_A_KBLOCK32) {                  // A stored K-blocked: the 256 x 256 tile, only the LDS-DMA source addresses differ
            using F = typename FlavorOf<T>::type;
            static MnnPerDeviceOnce raised_kb;
            MNN_HIP(mnn_once_per_device(raised_kb, [] { return mnn_raise_dynamic_lds((const void*)gemm_tn_glds256_kernel<F, true>, 4 * 256 * 128); }));
            dim3 grid2(cdiv(ntm2, 8) * 8 * ntn2, split_k);
            hipLaunchKernelGGL((gemm_tn_glds256_kernel<F, true>), grid2, dim3(512), 4 * 256 * 128, st, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, C,
                               ldc, c_bf16, bias, M, N, K, flags, split_k, ntm2, ntn2, m_rows_dev, k_rows_dev);
            MNN_LAUNCH_CHECK();
            return MNN_OK;
        }
        // the input projections (K = 448 / 512, 16-bit C, M a multiple of 128): the weight-resident persistent form (gemm_bres.hip)
        {
            if (gemm_bres_enabled() && split_k == 1 && !(flags & (MNN_GEMM_ACCUMULATE | MNN_GEMM_ATOMIC | MNN_GEMM_A_KBLOCK32)) && c_bf16 != 0 &&
                c_bf16 == (std::is_same<T, f16_t>::value ? MNN_F16 : MNN_BF16) && mnn_gemm_bres_ok(M, N, K) && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 &&
                ((uintptr_t)C & 15) == 0 && (size_t)128 * 64 * (size_t)lda < ((size_t)1 << 31))
                return mnn_gemm_bres_launch(st, std::is_same<T, f16_t>::value ? 1 : 0, M, N, K, A, lda, B, ldb, C, ldc, bias);
        }
        if (!no256 && K % 64 == 0 && M >= 256 && N >= 192 && (long)ntm2 * ntn2 * split_k >= 192 && K / 64 / split_k >= 4) {     // measured per shape: profiles/round1_f_gemm_shapes.md; round 3: 4 K tiles suffice (Dense forward K = 256: 362 -> 247 us)
            using F = typename FlavorOf<T>::type;
            static MnnPerDeviceOnce raised256;                  // per device and per flavour (this function is instantiated once per T)
            MNN_HIP(mnn_once_per_device(raised256, [] { return mnn_raise_dynamic_lds((const void*)gemm_tn_glds256_kernel<F>, 4 * 256 * 128); }));
            dim3 grid2(cdiv(ntm2, 8) * 8 * ntn2, split_k);
            hipLaunchKernelGGL(gemm_tn_glds256_kernel<F>, grid2, dim3(512), 4 * 256 * 128, st, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, C, ldc, c_bf16,
                               bias, M, N, K, flags, split_k, ntm2, ntn2, m_rows_dev, k_rows_dev);
            MNN_LAUNCH_CHECK();
            return MNN_OK;
        }
        // (BK = 128 for the tall-K weight-gradient GEMMs was measured slower: C2 1.28 -> 1.54 ms, 1 block/CU at 128 KiB LDS)
        if (K % 64 == 0) {
            hipLaunchKernelGGL((gemm_tn_glds_kernel<64, typename FlavorOf<T>::type>), grid, dim3(256), 0, st, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, C, ldc, c_bf16, bias, M,
                               N, K, flags, split_k, ntm, ntn);
            MNN_LAUNCH_CHECK();
            return MNN_OK;
        }
    }
    if constexpr (sizeof(T) == 4) {
        // f32 operands: eight waves per 128 x 128 tile, two per 64 x 64 quadrant, each taking half of every staged K chunk (MNN_GEMM_F32_KH=0: four)
        const bool kh2 = mnn_switch_int(MNN_SW_GEMM_F32_KH, 1) != 0;
        static MnnPerDeviceOnce raised;
        MNN_HIP(mnn_once_per_device(raised, [] {
            const hipError_t e = mnn_raise_dynamic_lds((const void*)gemm_tn_kernel<T, BM, BN, 2, 2, 2>, GemmCore<T, BM, BN, 2, 2, 2>::LDS_BYTES);
            return e != hipSuccess ? e : mnn_raise_dynamic_lds((const void*)gemm_tn_kernel<T, BM, BN, 2, 2>, GemmCore<T, BM, BN, 2, 2>::LDS_BYTES);
        }));
        if (kh2) {
            constexpr size_t lds2 = GemmCore<T, BM, BN, 2, 2, 2>::LDS_BYTES;
            hipLaunchKernelGGL((gemm_tn_kernel<T, BM, BN, 2, 2, 2>), grid, dim3(512), lds2, st, (const T*)A, lda, (const T*)B, ldb, C, ldc,
                               c_bf16, bias, M, N, K, flags, split_k, ntm, ntn);
            MNN_LAUNCH_CHECK();
            return MNN_OK;
        }
    }
    constexpr size_t lds1 = GemmCore<T, BM, BN, 2, 2>::LDS_BYTES;
    hipLaunchKernelGGL((gemm_tn_kernel<T, BM, BN, 2, 2>), grid, dim3(256), lds1, st, (const T*)A, lda, (const T*)B, ldb, C, ldc,
                       c_bf16, bias, M, N, K, flags, split_k, ntm, ntn);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

extern "C" int mnn_gemm_tn(mnn_stream_t s, int dtype, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                           int ldc, int c_dtype, const float* bias, int flags, int split_k) {
    return mnn_gemm_tn_rows(s, dtype, M, N, K, A, lda, B, ldb, C, ldc, c_dtype, bias, flags, split_k, nullptr, nullptr);
}

extern "C" int mnn_gemm_tn_rows(mnn_stream_t s, int dtype, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                                int ldc, int c_dtype, const float* bias, int flags, int split_k, const int* m_rows_dev, const int* k_rows_dev) {
    hipStream_t st = (hipStream_t)s;
    MNN_REQUIRE(dtype == MNN_BF16 || dtype == MNN_F16 || dtype == MNN_F32, "mnn_gemm_tn: dtype must be bf16, f16 or f32 (got %d)", dtype);
    MNN_REQUIRE(c_dtype == MNN_F32 || c_dtype == MNN_BF16 || c_dtype == MNN_F16, "mnn_gemm_tn: c_dtype must be f32, bf16 or f16");
    MNN_REQUIRE(M > 0 && N > 0 && K > 0, "mnn_gemm_tn: empty problem M=%d N=%d K=%d", M, N, K);
    const int al = dtype == MNN_F32 ? 4 : 8;
    MNN_REQUIRE(K % al == 0 && lda % al == 0 && ldb % al == 0, "mnn_gemm_tn: K/lda/ldb must be multiples of %d (K=%d lda=%d ldb=%d)",
                al, K, lda, ldb);
    if (flags & MNN_GEMM_A_KBLOCK32) {
        MNN_REQUIRE(dtype != MNN_F32 && K % 64 == 0 && lda >= M && ldb >= K && ldc >= N &&
                    (size_t)K * (size_t)lda < ((size_t)1 << 32),
                    "mnn_gemm_tn: a K-blocked A needs 16-bit operands, K %% 64 == 0, lda (its row count) >= M, K * lda < 2^32 (M=%d K=%d lda=%d)", M, K, lda);
    } else {
        MNN_REQUIRE(lda >= K, "mnn_gemm_tn: leading dimension too small");
    }
    MNN_REQUIRE(ldb >= K && ldc >= N, "mnn_gemm_tn: leading dimension too small");
    MNN_REQUIRE(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, "mnn_gemm_tn: operands must be 16-byte aligned");
    if (split_k < 1) split_k = 1;
    if (split_k > 1) {
        MNN_REQUIRE(c_dtype == MNN_F32, "mnn_gemm_tn: split-K needs an f32 C");
        if (!(flags & MNN_GEMM_ACCUMULATE)) {
            MNN_HIP(mnn_zero_async(C, (size_t)N * 4, (size_t)ldc * 4, M, st));
        }
        flags |= MNN_GEMM_ATOMIC | MNN_GEMM_ACCUMULATE;
        const int map = mnn_switch_int(MNN_SW_GEMM_SPLITK_MAP, -1);      // 0 | 1 forces a mapping (development); default: by slice count
        if (map == 1 || (map < 0 && split_k % 8 != 0)) flags |= GEMM_SPLITK_CONTIG;       // see splitk_item
    }
    MNN_REQUIRE(!(c_dtype != MNN_F32 && (flags & (MNN_GEMM_ACCUMULATE | MNN_GEMM_ATOMIC))), "mnn_gemm_tn: a 16-bit C cannot accumulate");
    const int c16 = c_dtype == MNN_F32 ? 0 : c_dtype;      // 0: f32 C; else the mnn_dtype code of the 16-bit C
    if (dtype == MNN_BF16) return launch_gemm<bf16_t>(st, M, N, K, A, lda, B, ldb, C, ldc, c16, bias, flags, split_k, m_rows_dev, k_rows_dev);
    if (dtype == MNN_F16) return launch_gemm<f16_t>(st, M, N, K, A, lda, B, ldb, C, ldc, c16, bias, flags, split_k, m_rows_dev, k_rows_dev);
    return launch_gemm<float>(st, M, N, K, A, lda, B, ldb, C, ldc, c16, bias, flags, split_k);      // (the f32 kernels do not look at the row counts: a hint only)
}
