// Annealed importance sampling (AIS) of an RBM's log partition function, one estimate per bias row (Neal 2001, "Annealed importance
// sampling"; Salakhutdinov & Murray 2008, "On the quantitative analysis of deep belief networks").  DESIGN.md §4 "AIS estimator".
//
// For one row: biases bh [Hn], bv [D], shared W [D, Hn], a ladder 0 = b_0 <= b_1 <= ... <= b_{L-1} = 1, and S independent chains.
//   F_b(v) = -bv.v - sum_j softplus(bh_j + b s_j),  s = v W.   b = 0 is exact: log Z_0 = sum_d softplus(bv_d) + sum_j softplus(bh_j).
//   chain c: v ~ Bernoulli(sigmoid(bv))                                      (stream 7, sub c L)
//            for k = 1 .. L-1:  log w_c += F_{b_{k-1}}(v) - F_{b_k}(v)       (the bv terms cancel)
//                               if k < L-1: h ~ sigmoid(bh + b_k s)          (stream 6, sub c L + k)
//                                           v ~ sigmoid(bv + b_k h W^T)      (stream 7, sub c L + k)
//   log Z^ = log Z_0 + logsumexp_c(log w_c) - log S.
// The s = v W of a step serves both its weight increment and its hidden half-step: two contractions per step.
//
// Arithmetic (fixed: the chains are checked bit for bit against a float32 restatement): every pre-activation is an ascending fmaf chain from
// 0 over the input index, then fmaf(b, s, bias), det_sigmoid, and the draw u < p.  At b = 1 this is s + bias -- a transition at b = 1 is
// the Gibbs iteration of mnn_rbm_gibbs bit for bit.
// The weight increment of unit j, softplus(x1) - softplus(x1 - dl) with x1 = bh_j + b_k s_j and dl = (b_k - b_{k-1}) s_j, is formed from the
// hidden phase's own sigmoid p = sigmoid(x1) so that it does not cancel:  -log1p(p expm1(-dl)) for x1 <= 0, dl - log1p(sigmoid(-x1)
// expm1(dl)) for x1 > 0 (both log1p arguments stay above -1/2); |dl| > 1 (short ladders only: no cancellation to fear) takes the plain
// difference of the two softplus values.  Each lane
// adds its float increments into a double accumulator over the whole ladder; a chain's lanes are combined in a fixed order at the end, so a
// chain's log w depends on nothing but its own counters (not on S, N or the row's position in the launch).
//
// Reverse AIS (RAISE: Burda, Grosse & Salakhutdinov 2015; mnn_rbm_raise, DESIGN.md §4 "Reverse AIS") runs the same ladder backwards from a
// data vector: the REVERSE instantiation of the two chain bodies below.
//   chain c: x = the row's data vector
//            for k = L-1 .. 0:  s = x W;  if k < L-1: log w_c += F_{b_{k+1}}(x) - F_{b_k}(x)
//                               if k > 0: h ~ sigmoid(bh + b_k s)            (stream 8, sub c L + k)
//                                         x ~ sigmoid(bv + b_k h W^T)        (stream 9, sub c L + k)
//   log Z^_rev = log Z_0 - (logsumexp_c(log w_c) - log S).
// It is the forward step with the rungs taken downwards: the draw's sigmoid sits at the LOWER b of the increment's pair, so with z = bh_j +
// b_k s_j the term is softplus(z) - softplus(z - dl) with dl = (b_k - b_{k+1}) s_j: ais_increment as it stands, and dl = 0 on the first pass
// (an increment of exactly 0).  L hidden and L - 1 visible contractions against the forward run's L - 1 and L - 2.
//
// Clamped AIS (mnn_rbm_ais_given / mnn_rbm_raise_given, DESIGN.md §4 "Clamped AIS"): `given` u8 [N, ld_given] holds one code per visible, the
// convention of mnn_rbm_gibbs -- 0 / 1 clamp the visible to that value, 255 leaves it free.  With G the clamped cells and F the free ones the
// target is Z_c = sum over {v : v_G = c_G} and h of exp(bv.v + bh.h + v W h), so that F_1(v) + log Z_c = -log p(v_F | v_G).  The ladder is
// the one above with the clamped cells held at their codes on every rung: the GIVEN instantiation of the two chain bodies.
//   base:       log Z_0 = sum_{d in F} softplus(bv_d) + sum_{d in G} bv_d c_d + sum_j softplus(bh_j); a clamped cell of the base draw is its
//               code and its uniform is not consumed (the counters are per cell: every free cell draws what it draws unclamped)
//   increment:  unchanged, s = v W over all visibles
//   transition: the hidden phase is unchanged; in the visible phase a clamped cell keeps its code (the clamped Gibbs chain)
//   reverse:    every chain starts from the data vector with each clamped cell replaced by its code
// given = NULL is the unconditioned estimator: the GIVEN = false instantiations, which hold no trace of the clamp.  All codes 255 runs the
// GIVEN kernels of the same form and gives the same bits.
#include "common.h"

// Philox streams of the hidden / visible draws: the reverse chains are reported beside the forward ones from one seed and share no uniform
template <bool REVERSE> struct AisStreams { static constexpr uint32_t H = REVERSE ? 8u : 6u, V = REVERSE ? 9u : 7u; };

__device__ __forceinline__ uint32_t ais_rowid(const uint32_t* __restrict__ row_ids, uint32_t row0, int n) {
    return row_ids != nullptr ? row_ids[n] : row0 + (uint32_t)n;
}

__device__ __forceinline__ double ais_softplus64(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// softplus(z) - softplus(z - dl), with ex = det_exp(-z) and p = 1 / (1 + ex) = det_sigmoid(z) of the hidden phase
__device__ __forceinline__ float ais_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float ais_increment(float z, float ex, float p, float dl) {
    if (fabsf(dl) > 1.f) return ais_softplus(z) - ais_softplus(z - dl);
    const bool neg = z <= 0.f;                                   // one expm1f and one log1pf per unit
    return (neg ? 0.f : dl) - log1pf((neg ? p : ex * p) * expm1f(neg ? -dl : dl));
}

struct AisArgs {
    int N, D, Hn, S, L;
    const float* betas; const float* W; const float* bh; int ld_bh; const float* bv; int ld_bv;
    uint64_t seed; uint32_t row0; const uint32_t* row_ids;
    double* lw;                 // [N, S] per-chain log weights (workspace)
    uint8_t* v_out;             // optional [N, S, D] final states
    const uint8_t* v_data;      // reverse only: [N, D] the rows' data vectors, where every chain of a row starts
    const uint8_t* given; int ld_given;      // GIVEN only: [N, ld_given] the rows' codes
};

// codes of the clamped chain (u8 per visible): 0 / 1 hold the visible at that value, AIS_GIVEN_FREE leaves it to the chain
#define AIS_GIVEN_FREE 255
// whether any of four codes packed into a word is free
__device__ __forceinline__ bool ais_any_free(uint32_t q) {
    return (q & 0xffu) == AIS_GIVEN_FREE || ((q >> 8) & 0xffu) == AIS_GIVEN_FREE || ((q >> 16) & 0xffu) == AIS_GIVEN_FREE || (q >> 24) == AIS_GIVEN_FREE;
}

// ----------------------------------------------------------------------------------------------
// Matrix-core form: a workgroup (8 waves) runs 64 chains of one row through the whole ladder.  The layout is rbm_gibbs_mfma_kernel's (rbm.hip):
// W f32 [De][Hn + 1] resident in LDS, the binary states as bytes [64][odd word pitch], products formed transposed, C[unit][chain] =
// sum_k W(k, unit) state[chain][k] on v_mfma_f32_32x32x2_f32 (one IEEE rounding per product-add: the ascending fmaf chain).  A lane's
// accumulator quad holds four consecutive units of one chain = the four uniforms of one Philox block.
// GIVEN: the 64 chains of a workgroup share their row's D codes, parked once in LDS behind the state bytes (the form is chosen with 2 KB of
// the LDS limit to spare and takes no D near 2048).  A clamped cell is written at the start and never again; a Philox block whose four cells
// are all clamped is skipped.
// ----------------------------------------------------------------------------------------------
typedef float ais_f32x16 __attribute__((ext_vector_type(16)));
#define AIS_CHAINS 64

static __host__ __device__ __forceinline__ int ais_pitch(int n) { int w = (n + 1 + 3) / 4; return 4 * (w | 1); }

template <bool REVERSE, bool GIVEN> __device__ __forceinline__ void ais_mfma_chains(const AisArgs& A) {
    constexpr uint32_t STREAM_H = AisStreams<REVERSE>::H, STREAM_V = AisStreams<REVERSE>::V;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = A.N, D = A.D, Hn = A.Hn, S = A.S, L = A.L, ldw = Hn + 1;
    const int De = (D + 1) & ~1, He = (Hn + 1) & ~1;
    const int pv = ais_pitch(D), ph = ais_pitch(Hn);
    float* Ws = smem;                                                            // [De][ldw]
    double* red = reinterpret_cast<double*>(Ws + (size_t)De * ldw);            // [8 waves][32]  (8-byte aligned: De is even)
    uint8_t* vs = reinterpret_cast<uint8_t*>(red + 8 * 32);                     // [64][pv]
    uint8_t* hs = vs + AIS_CHAINS * pv;                                          // [64][ph]
    uint8_t* gs = hs + AIS_CHAINS * ph;                                          // GIVEN: [(D + 3) & ~3] the row's codes
    const int nblk = (S + AIS_CHAINS - 1) / AIS_CHAINS;
    const int n = blockIdx.x / nblk, c0 = (blockIdx.x - n * nblk) * AIS_CHAINS;
    (void)N;
    const uint32_t id = ais_rowid(A.row_ids, A.row0, n);
    const float* __restrict__ bh = A.bh + (size_t)n * A.ld_bh;
    const float* __restrict__ bv = A.bv + (size_t)n * A.ld_bv;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int d = w; d < De; d += 8)
        for (int j = lane; j < ldw; j += 64) Ws[d * ldw + j] = j < Hn ? A.W[(size_t)min(d, D - 1) * Hn + j] : 0.f;
    for (int e = threadIdx.x; e < AIS_CHAINS * (pv + ph) / 4; e += 512) reinterpret_cast<uint32_t*>(vs)[e] = 0u;
    if constexpr (GIVEN)                                                         // (the tail of the last quad reads as clamped: nothing to draw there)
        for (int d = threadIdx.x; d < ((D + 3) & ~3); d += 512) gs[d] = d < D ? A.given[(size_t)n * A.ld_given + d] : (uint8_t)0;
    __syncthreads();
    if constexpr (REVERSE) {
        // every chain starts at the row's data vector (GIVEN: a clamped cell at its code): wave -> chains, lane -> visibles
        const uint8_t* __restrict__ x0 = A.v_data + (size_t)n * D;
        for (int lc = w; lc < AIS_CHAINS; lc += 8)
            for (int d = lane; d < D; d += 64) {
                uint8_t x = x0[d];
                if constexpr (GIVEN)
                    if (gs[d] != AIS_GIVEN_FREE) x = gs[d];
                vs[lc * pv + d] = x ? 1 : 0;
            }
    } else {
        // base draw: v ~ Bernoulli(det_sigmoid(bv)), stream 7, sub c L; thread -> (chain, quad of four visibles)
        const int nq = (D + 3) / 4;
        for (int e = threadIdx.x; e < AIS_CHAINS * nq; e += 512) {
            const int lc = e / nq, q = e - lc * nq;
            if constexpr (GIVEN) {
                // a clamped cell is its code; the block of four clamped cells is not drawn
                bool any_free = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = 4 * q + i;
                    if (d >= D) continue;
                    if (gs[d] == AIS_GIVEN_FREE) any_free = true;
                    else vs[lc * pv + d] = gs[d] ? 1 : 0;
                }
                if (!any_free) continue;
            }
            float u[4];
            philox_uniform4(A.seed, STREAM_V, id, (uint32_t)(c0 + lc) * (uint32_t)L, (uint32_t)q, u);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = 4 * q + i;
                if (d >= D) continue;
                if constexpr (GIVEN)
                    if (gs[d] != AIS_GIVEN_FREE) continue;
                vs[lc * pv + d] = u[i] < det_sigmoid(bv[d]) ? 1 : 0;
            }
        }
    }
    const int r = lane & 31, hh = lane >> 5;
    const int nht = (Hn + 31) / 32, ndt = (D + 31) / 32;
    const int rt_h = w >> 2;
    const uint32_t c_h = (uint32_t)(c0 + 32 * rt_h + r);                         // this lane's chain in the hidden phase
    float bhr[2][16], bvr[16];                                                    // the biases of the first-pass jobs (constant over the ladder)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) bhr[q][e] = bh[min(32 * (2 * (w & 3) + q) + (e & 3) + 8 * (e >> 2) + 4 * hh, Hn - 1)];
    {
        const int job = min(w, 2 * ndt - 1), dt = job - (job / ndt) * ndt;
#pragma unroll
        for (int e = 0; e < 16; ++e) bvr[e] = bv[min(32 * dt + (e & 3) + 8 * (e >> 2) + 4 * hh, D - 1)];
    }
    double lw = 0.0;
    __syncthreads();
    // the rungs: k = 1 .. L-1 upwards, or k = L-1 .. 0 downwards.  dbk is b_k minus the other b of the rung's increment pair: the rung below,
    // or downwards the rung above (the top rung itself on the first pass: dbk = 0, no increment).  The last rung of either has no draw.
    for (int k = REVERSE ? L - 1 : 1; REVERSE ? k >= 0 : k < L; k += REVERSE ? -1 : 1) {
        const float bk = A.betas[k], dbk = bk - A.betas[REVERSE ? min(k + 1, L - 1) : k - 1];
        const bool trans = REVERSE ? k > 0 : k < L - 1;
        const uint32_t sub_h = c_h * (uint32_t)L + (uint32_t)k;
        // ---- hidden phase: s = v W, the weight increment, and (trans) h ~ sigmoid(bh + b_k s) ----
        for (int jt0 = 2 * (w & 3); jt0 < nht; jt0 += 8) {
            ais_f32x16 acc[2];
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
            const uint8_t* sp = vs + (32 * rt_h + r) * pv + hh;
            const float* a0 = Ws + (size_t)hh * ldw + min(32 * jt0 + r, Hn - 1);
            const float* a1 = Ws + (size_t)hh * ldw + min(32 * (jt0 + 1) + r, Hn - 1);
            for (int s = 0; s < De / 2; ++s) {
                const float b = (float)sp[2 * s];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[(size_t)s * 2 * ldw], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[(size_t)s * 2 * ldw], b, acc[1], 0, 0, 0);
            }
            // the epilogue of one unit tile (written out twice below: as one unrolled loop over both tiles it exceeds the unroller's size limit)
            auto tile = [&](const ais_f32x16& a, const float* bq, int jt) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int j0 = 32 * jt + 8 * g4 + 4 * hh;
                    if (j0 >= Hn) continue;
                    float u[4] = {0.f, 0.f, 0.f, 0.f};
                    if (trans) philox_uniform4(A.seed, STREAM_H, id, sub_h, (uint32_t)(j0 >> 2), u);
                    uint32_t pk = 0u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (j0 + e >= Hn) continue;
                        const float bb = jt < 8 ? bq[4 * g4 + e] : bh[j0 + e];
                        const float s = a[4 * g4 + e];
                        const float z = fmaf(bk, s, bb);
                        const float ex = det_exp(-z);
                        const float p = 1.0f / (1.0f + ex);                          // = det_sigmoid(z)
                        lw += (double)ais_increment(z, ex, p, dbk * s);
                        pk |= (u[e] < p ? 1u : 0u) << (8 * e);
                    }
                    if (trans) *reinterpret_cast<uint32_t*>(hs + (32 * rt_h + r) * ph + j0) = pk;
                }
            };
            tile(acc[0], bhr[0], jt0);
            tile(acc[1], bhr[1], jt0 + 1);
        }
        if (!trans) break;
        __syncthreads();
        // ---- visible phase: v ~ sigmoid(bv + b_k h W^T) ----
        for (int job = w; job < 2 * ndt; job += 8) {
            const int rt = job / ndt, dt = job - rt * ndt;
            ais_f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            const uint8_t* sp = hs + (32 * rt + r) * ph + hh;
            const float* ap = Ws + (size_t)min(32 * dt + r, D - 1) * ldw + hh;
            for (int s = 0; s < He / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], (float)sp[2 * s], acc, 0, 0, 0);
            const uint32_t sub_v = (uint32_t)(c0 + 32 * rt + r) * (uint32_t)L + (uint32_t)k;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * dt + 8 * g4 + 4 * hh;
                if (d0 >= D) continue;
                uint32_t cq = 0u;                                                    // GIVEN: the quad's four codes, one per byte
                if constexpr (GIVEN) {
                    cq = *reinterpret_cast<const uint32_t*>(gs + d0);
                    if (!ais_any_free(cq)) continue;
                }
                float u[4];
                philox_uniform4(A.seed, STREAM_V, id, sub_v, (uint32_t)(d0 >> 2), u);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int d = d0 + e;
                    if (d >= D) continue;
                    if constexpr (GIVEN)
                        if (((cq >> (8 * e)) & 0xffu) != AIS_GIVEN_FREE) continue;   // a clamped cell keeps its code
                    const float p = det_sigmoid(fmaf(bk, acc[4 * g4 + e], job < 8 ? bvr[4 * g4 + e] : bv[d]));
                    vs[(32 * rt + r) * pv + d] = u[e] < p ? 1 : 0;
                }
            }
        }
        __syncthreads();
    }
    // a chain's partial sums: lanes r and r + 32 of the four waves of its row tile, in a fixed order
    lw += __shfl_xor(lw, 32);
    if (hh == 0) red[w * 32 + r] = lw;
    __syncthreads();
    if (threadIdx.x < AIS_CHAINS) {
        const int lc = threadIdx.x, rt = lc >> 5, rr = lc & 31;
        const double t = ((red[(4 * rt + 0) * 32 + rr] + red[(4 * rt + 1) * 32 + rr]) + red[(4 * rt + 2) * 32 + rr]) + red[(4 * rt + 3) * 32 + rr];
        if (c0 + lc < S) A.lw[(size_t)n * S + c0 + lc] = t;
    }
    if (A.v_out != nullptr)
        for (int e = threadIdx.x; e < AIS_CHAINS * D; e += 512) {
            const int lc = e / D, d = e - lc * D;
            if (c0 + lc < S) A.v_out[((size_t)n * S + c0 + lc) * D + d] = vs[lc * pv + d];
        }
}

__global__ void __launch_bounds__(512) rbm_ais_mfma_kernel(AisArgs A) { ais_mfma_chains<false, false>(A); }
__global__ void __launch_bounds__(512) rbm_raise_mfma_kernel(AisArgs A) { ais_mfma_chains<true, false>(A); }
__global__ void __launch_bounds__(512) rbm_given_ais_mfma_kernel(AisArgs A) { ais_mfma_chains<false, true>(A); }
__global__ void __launch_bounds__(512) rbm_given_raise_mfma_kernel(AisArgs A) { ais_mfma_chains<true, true>(A); }

static size_t ais_mfma_lds_bytes(int D, int Hn) {
    return (size_t)((D + 1) & ~1) * (Hn + 1) * sizeof(float) + 8 * 32 * sizeof(double) + (size_t)AIS_CHAINS * (ais_pitch(D) + ais_pitch(Hn));
}
static size_t ais_codes_lds_bytes(int D) { return (size_t)((D + 3) & ~3); }          // GIVEN: the row's codes, either form

// ----------------------------------------------------------------------------------------------
// Streaming form (every shape mnn_rbm_gibbs takes, e.g. joint mode's D = 440): 256 threads run AIS_R chains of one row, states in LDS as f32
// 0 / 1, W streamed from L2 (coalesced over the output unit; the transposed copy in the workspace serves the visible phase).  Same
// arithmetic, same counters: the same chains as the matrix-core form.  GIVEN: the row's codes in LDS behind the states; a clamped cell is
// written at the start and its visible contraction is skipped.
// ----------------------------------------------------------------------------------------------
#define AIS_R 8

template <bool REVERSE, bool GIVEN> __device__ __forceinline__ void ais_stream_chains(const AisArgs& A, const float* __restrict__ Wt) {
    constexpr uint32_t STREAM_H = AisStreams<REVERSE>::H, STREAM_V = AisStreams<REVERSE>::V;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[4][AIS_R];
    const int D = A.D, Hn = A.Hn, S = A.S, L = A.L;
    const int Dp = (D + 3) & ~3, Hp = (Hn + 3) & ~3;
    float* vs = smem;                     // [AIS_R][Dp]
    float* hs = smem + AIS_R * Dp;        // [AIS_R][Hp]
    uint8_t* gs = reinterpret_cast<uint8_t*>(hs + AIS_R * Hp);      // GIVEN: [(D + 3) & ~3] the row's codes
    const int nblk = (S + AIS_R - 1) / AIS_R;
    const int n = blockIdx.x / nblk, c0 = (blockIdx.x - n * nblk) * AIS_R;
    const uint32_t id = ais_rowid(A.row_ids, A.row0, n);
    const float* __restrict__ bh = A.bh + (size_t)n * A.ld_bh;
    const float* __restrict__ bv = A.bv + (size_t)n * A.ld_bv;
    if constexpr (GIVEN) {
        for (int d = threadIdx.x; d < D; d += blockDim.x) gs[d] = A.given[(size_t)n * A.ld_given + d];
        __syncthreads();
    }
    if constexpr (REVERSE) {
        // every chain starts at the row's data vector (GIVEN: a clamped cell at its code)
        const uint8_t* __restrict__ x0 = A.v_data + (size_t)n * D;
        for (int d = threadIdx.x; d < D; d += blockDim.x) {
            uint8_t c = x0[d];
            if constexpr (GIVEN)
                if (gs[d] != AIS_GIVEN_FREE) c = gs[d];
            const float x = c ? 1.f : 0.f;
#pragma unroll
            for (int r = 0; r < AIS_R; ++r) vs[r * Dp + d] = x;
        }
    } else {
        for (int e = threadIdx.x; e < AIS_R * D; e += blockDim.x) {
            const int r = e / D, d = e - r * D;
            if constexpr (GIVEN)
                if (gs[d] != AIS_GIVEN_FREE) {                       // a clamped cell is its code: no uniform
                    vs[r * Dp + d] = gs[d] ? 1.f : 0.f;
                    continue;
                }
            const float u = philox_uniform1(A.seed, STREAM_V, id, (uint32_t)(c0 + r) * (uint32_t)L, (uint32_t)d);
            vs[r * Dp + d] = u < det_sigmoid(bv[d]) ? 1.f : 0.f;
        }
    }
    double lw[AIS_R];
#pragma unroll
    for (int r = 0; r < AIS_R; ++r) lw[r] = 0.0;
    __syncthreads();
    // the rungs, dbk and trans: as in ais_mfma_chains
    for (int k = REVERSE ? L - 1 : 1; REVERSE ? k >= 0 : k < L; k += REVERSE ? -1 : 1) {
        const float bk = A.betas[k], dbk = bk - A.betas[REVERSE ? min(k + 1, L - 1) : k - 1];
        const bool trans = REVERSE ? k > 0 : k < L - 1;
        for (int j = threadIdx.x; j < Hn; j += blockDim.x) {
            float acc[AIS_R];
#pragma unroll
            for (int r = 0; r < AIS_R; ++r) acc[r] = 0.f;
            for (int d = 0; d < D; ++d) {
                const float wv = A.W[(size_t)d * Hn + j];
#pragma unroll
                for (int r = 0; r < AIS_R; ++r) acc[r] = fmaf(vs[r * Dp + d], wv, acc[r]);
            }
            const float bb = bh[j];
#pragma unroll
            for (int r = 0; r < AIS_R; ++r) {
                const float z = fmaf(bk, acc[r], bb);
                const float ex = det_exp(-z);
                const float p = 1.0f / (1.0f + ex);
                lw[r] += (double)ais_increment(z, ex, p, dbk * acc[r]);
                if (trans) {
                    const float u = philox_uniform1(A.seed, STREAM_H, id, (uint32_t)(c0 + r) * (uint32_t)L + (uint32_t)k, (uint32_t)j);
                    hs[r * Hp + j] = u < p ? 1.f : 0.f;
                }
            }
        }
        if (!trans) break;
        __syncthreads();
        for (int d = threadIdx.x; d < D; d += blockDim.x) {
            if constexpr (GIVEN)
                if (gs[d] != AIS_GIVEN_FREE) continue;                   // a clamped cell keeps its code
            float acc[AIS_R];
#pragma unroll
            for (int r = 0; r < AIS_R; ++r) acc[r] = 0.f;
            for (int j = 0; j < Hn; ++j) {
                const float wv = Wt[(size_t)j * D + d];
#pragma unroll
                for (int r = 0; r < AIS_R; ++r) acc[r] = fmaf(hs[r * Hp + j], wv, acc[r]);
            }
            const float bb = bv[d];
#pragma unroll
            for (int r = 0; r < AIS_R; ++r) {
                const float p = det_sigmoid(fmaf(bk, acc[r], bb));
                const float u = philox_uniform1(A.seed, STREAM_V, id, (uint32_t)(c0 + r) * (uint32_t)L + (uint32_t)k, (uint32_t)d);
                vs[r * Dp + d] = u < p ? 1.f : 0.f;
            }
        }
        __syncthreads();
    }
    // per chain: a fixed-order butterfly over the wave, then the four waves in order
#pragma unroll
    for (int r = 0; r < AIS_R; ++r) {
        double x = lw[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][r] = x;
    }
    __syncthreads();
    if (threadIdx.x < AIS_R && c0 + (int)threadIdx.x < S) {
        const int r = threadIdx.x;
        A.lw[(size_t)n * S + c0 + r] = ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r];
    }
    if (A.v_out != nullptr)
        for (int e = threadIdx.x; e < AIS_R * D; e += blockDim.x) {
            const int r = e / D, d = e - r * D;
            if (c0 + r < S) A.v_out[((size_t)n * S + c0 + r) * D + d] = (uint8_t)vs[r * Dp + d];
        }
}

__global__ void __launch_bounds__(256) rbm_ais_stream_kernel(AisArgs A, const float* __restrict__ Wt) { ais_stream_chains<false, false>(A, Wt); }
__global__ void __launch_bounds__(256) rbm_raise_stream_kernel(AisArgs A, const float* __restrict__ Wt) { ais_stream_chains<true, false>(A, Wt); }
__global__ void __launch_bounds__(256) rbm_given_ais_stream_kernel(AisArgs A, const float* __restrict__ Wt) { ais_stream_chains<false, true>(A, Wt); }
__global__ void __launch_bounds__(256) rbm_given_raise_stream_kernel(AisArgs A, const float* __restrict__ Wt) { ais_stream_chains<true, true>(A, Wt); }

#define AIS_STREAM_STATIC_LDS (4 * AIS_R * sizeof(double))          // the kernel's red[4][AIS_R]
static size_t ais_stream_lds_bytes(int D, int Hn) { return (size_t)AIS_R * (((D + 3) & ~3) + ((Hn + 3) & ~3)) * sizeof(float); }

// ----------------------------------------------------------------------------------------------
// Per-row reduction (one workgroup per row, fixed-order tree sums in double):  log Z^ = log Z_0 + m + log(sum_c exp(lw_c - m)) - log S,
// m = max_c lw_c;  stats = (ESS = (sum w)^2 / sum w^2,  stderr of log Z^ by the delta method on the mean of w = sqrt((S / ESS - 1) / (S - 1))).
// Reverse: the chains' mean weight estimates Z_0 / Z, so log Z^_rev = log Z_0 - (m + log(sum) - log S); ESS and stderr by the same formulas.
// given (null: every visible free): a clamped visible's term of log Z_0 is bv_d c_d in place of softplus(bv_d), in the same place of the sum.
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ double ais_block_sum(double x, double* buf) {
    buf[threadIdx.x] = x;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) buf[threadIdx.x] += buf[threadIdx.x + o];
        __syncthreads();
    }
    const double t = buf[0];
    __syncthreads();
    return t;
}

__global__ void __launch_bounds__(256) rbm_ais_reduce_kernel(int D, int Hn, int S, const float* __restrict__ bh, int ld_bh, const float* __restrict__ bv,
                                                             int ld_bv, const double* __restrict__ lw, float* __restrict__ log_z,
                                                             float* __restrict__ log_w, float* __restrict__ stats, int reverse,
                                                             const uint8_t* __restrict__ given, int ld_given) {
    __shared__ double buf[256];
    const int n = blockIdx.x;
    const double* x = lw + (size_t)n * S;
    double m = -INFINITY;
    for (int c = threadIdx.x; c < S; c += 256) m = fmax(m, x[c]);
    buf[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) buf[threadIdx.x] = fmax(buf[threadIdx.x], buf[threadIdx.x + o]);
        __syncthreads();
    }
    m = buf[0];
    __syncthreads();
    double a = 0.0, b = 0.0, z0 = 0.0;
    for (int c = threadIdx.x; c < S; c += 256) {
        const double e = exp(x[c] - m);
        a += e;
        b += e * e;
        if (log_w != nullptr) log_w[(size_t)n * S + c] = (float)x[c];
    }
    for (int d = threadIdx.x; d < D; d += 256) {
        const double b = (double)bv[(size_t)n * ld_bv + d];
        const uint8_t g = given != nullptr ? given[(size_t)n * ld_given + d] : (uint8_t)AIS_GIVEN_FREE;
        z0 += g == AIS_GIVEN_FREE ? ais_softplus64(b) : (g ? b : 0.0);
    }
    for (int j = threadIdx.x; j < Hn; j += 256) z0 += ais_softplus64((double)bh[(size_t)n * ld_bh + j]);
    a = ais_block_sum(a, buf);
    b = ais_block_sum(b, buf);
    z0 = ais_block_sum(z0, buf);
    if (threadIdx.x == 0) {
        log_z[n] = reverse ? (float)(z0 - (m + log(a) - log((double)S))) : (float)(z0 + m + log(a) - log((double)S));
        if (stats != nullptr) {
            const double ess = a * a / b;
            stats[2 * n] = (float)ess;
            stats[2 * n + 1] = S > 1 ? (float)sqrt(fmax((double)S / ess - 1.0, 0.0) / (double)(S - 1)) : INFINITY;
        }
    }
}

extern "C" int mnn_transpose(mnn_stream_t s, const void* in, int in_dtype, int R, int C, int ld_in, void* out, int out_dtype, int ld_out);

static size_t ais_lw_bytes(int N, int S) { return ((size_t)N * (size_t)S * sizeof(double) + 255) & ~(size_t)255; }

// the form of a shape (not of N or S: a row's chains are the same bits whatever else is in the launch)
static bool ais_use_mfma(int D, int Hn) { return Hn >= 32 && ais_mfma_lds_bytes(D, Hn) <= 158 * 1024 && !mnn_switch_set(MNN_SW_RBM_NO_MFMA); }

extern "C" size_t mnn_rbm_ais_workspace_bytes(int N, int D, int Hn, int n_chains, int n_betas) {
    (void)n_betas;
    if (N <= 0 || D <= 0 || Hn <= 0 || n_chains <= 0) return 0;
    return ais_lw_bytes(N, n_chains) + (size_t)D * Hn * sizeof(float);
}

// both entries: `what` names the entry in messages; reverse runs the chains downwards from v_data
static int ais_launch(const char* what, mnn_stream_t s, int N, int D, int Hn, int n_chains, int n_betas, const float* betas, const float* W,
                      const float* bh, int ld_bh, const float* bv, int ld_bv, const uint8_t* v_data, bool reverse, uint64_t seed, uint32_t row0,
                      const uint32_t* row_ids, float* log_z, float* log_w, uint8_t* v_out, float* stats, void* workspace, const uint8_t* given,
                      int ld_given) {
    MNN_REQUIRE(N > 0 && D > 0 && Hn > 0, "%s: bad sizes N=%d D=%d Hn=%d", what, N, D, Hn);
    MNN_REQUIRE(n_chains >= 1, "%s: n_chains=%d < 1", what, n_chains);
    MNN_REQUIRE(n_betas >= 2, "%s: n_betas=%d < 2 (the ladder runs from 0 to 1)", what, n_betas);
    MNN_REQUIRE((uint64_t)n_chains * (uint64_t)n_betas < (1ull << 32), "%s: n_chains * n_betas = %llu does not fit the 32-bit sub counter", what,
                (unsigned long long)n_chains * (unsigned long long)n_betas);
    MNN_REQUIRE(betas && W && bh && bv && log_z && workspace && (v_data || !reverse), "%s: null pointer", what);
    MNN_REQUIRE((ld_bh == 0 || ld_bh >= Hn) && (ld_bv == 0 || ld_bv >= D), "%s: bad bias leading dimension", what);
    MNN_REQUIRE(given == nullptr || ld_given >= D, "%s: ld_given=%d < D=%d", what, ld_given, D);
    const size_t codes_lds = given != nullptr ? ais_codes_lds_bytes(D) : 0;
    MNN_REQUIRE(ais_stream_lds_bytes(D, Hn) + codes_lds + AIS_STREAM_STATIC_LDS <= 160 * 1024,
                "%s: D+Hn too large for LDS (8 chains' f32 states%s)", what, given != nullptr ? " and the row's D code bytes" : "");
    const bool mfma = ais_use_mfma(D, Hn);
    const long blocks = (long)N * ((n_chains + (mfma ? AIS_CHAINS : AIS_R) - 1) / (mfma ? AIS_CHAINS : AIS_R));
    MNN_REQUIRE(blocks <= 0x7fffffffL, "%s: N * chain blocks = %ld exceeds the grid", what, blocks);
    hipStream_t st = (hipStream_t)s;
    double* lw = reinterpret_cast<double*>(workspace);
    AisArgs a{N, D, Hn, n_chains, n_betas, betas, W, bh, ld_bh, bv, ld_bv, seed, row0, row_ids, lw, v_out, v_data, given, ld_given};
    static MnnPerDeviceOnce raised;
    MNN_HIP(mnn_once_per_device(raised, [] {
        hipError_t e = hipSuccess;
        for (auto* f : {&rbm_ais_mfma_kernel, &rbm_raise_mfma_kernel, &rbm_given_ais_mfma_kernel, &rbm_given_raise_mfma_kernel})
            if (e == hipSuccess) e = mnn_raise_dynamic_lds(reinterpret_cast<const void*>(f), 160 * 1024);
        for (auto* f : {&rbm_ais_stream_kernel, &rbm_raise_stream_kernel, &rbm_given_ais_stream_kernel, &rbm_given_raise_stream_kernel})
            if (e == hipSuccess) e = mnn_raise_dynamic_lds(reinterpret_cast<const void*>(f), 160 * 1024 - (int)AIS_STREAM_STATIC_LDS);
        return e;
    }));
    // the form is the shape's, whatever `given` is: the codes fit the LDS the form's choice leaves free
    if (mfma) {
        auto* f = given != nullptr ? (reverse ? rbm_given_raise_mfma_kernel : rbm_given_ais_mfma_kernel) : (reverse ? rbm_raise_mfma_kernel : rbm_ais_mfma_kernel);
        hipLaunchKernelGGL(f, dim3((unsigned)blocks), dim3(512), ais_mfma_lds_bytes(D, Hn) + codes_lds, st, a);
    } else {
        float* Wt = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + ais_lw_bytes(N, n_chains));
        int rc = mnn_transpose(s, W, MNN_F32, D, Hn, Hn, Wt, MNN_F32, D);
        if (rc != MNN_OK) return rc;
        auto* f = given != nullptr ? (reverse ? rbm_given_raise_stream_kernel : rbm_given_ais_stream_kernel)
                                   : (reverse ? rbm_raise_stream_kernel : rbm_ais_stream_kernel);
        hipLaunchKernelGGL(f, dim3((unsigned)blocks), dim3(256), ais_stream_lds_bytes(D, Hn) + codes_lds, st, a, (const float*)Wt);
    }
    MNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rbm_ais_reduce_kernel, dim3(N), dim3(256), 0, st, D, Hn, n_chains, bh, ld_bh, bv, ld_bv, (const double*)lw, log_z, log_w, stats,
                       reverse ? 1 : 0, given, ld_given);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

extern "C" int mnn_rbm_ais_given(mnn_stream_t s, int N, int D, int Hn, int n_chains, int n_betas, const float* betas, const float* W,
                                 const float* bh, int ld_bh, const float* bv, int ld_bv, uint64_t seed, uint32_t row0, const uint32_t* row_ids,
                                 float* log_z, float* log_w, uint8_t* v_out, float* stats, void* workspace, const uint8_t* given, int ld_given) {
    return ais_launch("mnn_rbm_ais", s, N, D, Hn, n_chains, n_betas, betas, W, bh, ld_bh, bv, ld_bv, nullptr, false, seed, row0, row_ids, log_z, log_w,
                      v_out, stats, workspace, given, ld_given);
}

extern "C" int mnn_rbm_ais(mnn_stream_t s, int N, int D, int Hn, int n_chains, int n_betas, const float* betas, const float* W, const float* bh,
                           int ld_bh, const float* bv, int ld_bv, uint64_t seed, uint32_t row0, const uint32_t* row_ids, float* log_z, float* log_w,
                           uint8_t* v_out, float* stats, void* workspace) {
    return mnn_rbm_ais_given(s, N, D, Hn, n_chains, n_betas, betas, W, bh, ld_bh, bv, ld_bv, seed, row0, row_ids, log_z, log_w, v_out, stats, workspace,
                             nullptr, 0);
}

extern "C" int mnn_rbm_raise_given(mnn_stream_t s, int N, int D, int Hn, int n_chains, int n_betas, const float* betas, const float* W,
                                   const float* bh, int ld_bh, const float* bv, int ld_bv, const uint8_t* v, uint64_t seed, uint32_t row0,
                                   const uint32_t* row_ids, float* log_z, float* log_w, uint8_t* v_out, float* stats, void* workspace,
                                   const uint8_t* given, int ld_given) {
    return ais_launch("mnn_rbm_raise", s, N, D, Hn, n_chains, n_betas, betas, W, bh, ld_bh, bv, ld_bv, v, true, seed, row0, row_ids, log_z, log_w,
                      v_out, stats, workspace, given, ld_given);
}

extern "C" int mnn_rbm_raise(mnn_stream_t s, int N, int D, int Hn, int n_chains, int n_betas, const float* betas, const float* W, const float* bh,
                             int ld_bh, const float* bv, int ld_bv, const uint8_t* v, uint64_t seed, uint32_t row0, const uint32_t* row_ids,
                             float* log_z, float* log_w, uint8_t* v_out, float* stats, void* workspace) {
    return mnn_rbm_raise_given(s, N, D, Hn, n_chains, n_betas, betas, W, bh, ld_bh, bv, ld_bv, v, seed, row0, row_ids, log_z, log_w, v_out, stats,
                               workspace, nullptr, 0);
}
