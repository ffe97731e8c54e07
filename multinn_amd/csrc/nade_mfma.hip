// NADE log-prob on the matrix cores (bf16 operands, f32 accumulation) for Hn = 256: forward scan.
// Reference: /root/reference/multinn/models/common/nade.py:155-229.
//
// The conditional of visible d is  p_d = sigmoid(b_dec[d] + w_dec[d] . h_d),  h_d = sigmoid(a_d),
// a_{d+1} = a_d + v_d w_enc[d]  (nade.py:206-219).  `a` only moves at visibles with v = 1, so a row has
// 1 + nnz(v) distinct hidden STATES and the D dot products are a block-sparse GEMM
//     logits[row, d] = state(row, d) . w_dec[d]
// A workgroup owns 32 rows and walks the visibles in tiles of 32 columns.  Per tile:
//   * base states (one per row, as of the tile's first column) x w_dec tile  -> 32 x 32 logits on MFMA
//   * every flip (v = 1) inside the tile creates a new state: a += w_enc[d] in f32 (the wave that owns the row, four hidden units a lane),
//     h = sigmoid(a) -> bf16 into a flip-state tile; flip states x w_dec tile -> 32-slot x 32 logits on MFMA
//   * each (row, d) picks the logit of the latest state created before d (popcount of the row's v bits), adds
//     b_dec, and finishes p, the NLL term and d nll / d b_dec.
// The dense work (D x Hn MACs per row) runs on v_mfma_f32_16x16x32_bf16; the VALU keeps only the sparse encoder
// adds, one sigmoid per state element and the per-(row, d) pointwise.  w_enc stays f32 (a is exact up to f32
// summation order and is handed to the backward pass as a_final); w_dec is read as a bf16 copy.
#include "common.h"
#include "lstm_handoff.h"     // hf_lds_barrier: the workgroup barrier that waits for LDS traffic only (no vmcnt drain at the tile's barriers)
typedef float nm_f4 __attribute__((ext_vector_type(4)));
// results (conditionals, d nll / d logit, a_final) are written once and read by later kernels: stored non-temporal, they leave the decoder / encoder
// weights every workgroup re-reads in the L2 (2.19 -> 2.17 ms at [262144, 440, 256]; same in the backward's d b_enc store)
#define NM_ST4(dst, a) __builtin_nontemporal_store((nm_f4){a[0], a[1], a[2], a[3]}, reinterpret_cast<nm_f4*>(dst))
#include <algorithm>
#include <type_traits>

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const void* gas_ptr_t;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

#ifdef NM_TRACE      // development only: per-phase clocks of one workgroup (profiles/tools/nade_trace.hip)
__device__ long long nm_trace[16];
#define NM_T(k) do { if (tid == 0 && blockIdx.x == NM_TRACE) { const long long now_ = wall_clock64(); nm_trace[k] += now_ - tprev_; tprev_ = now_; } } while (0)
#else
#define NM_T(k) do { } while (0)
#endif
#define NADE_EPS 1e-6f
#define LN2F 0.6931471805599453f
#define NM_H 256          // hidden width this kernel is specialised for
#define NM_PITCH 264      // bf16 elements per state-tile row (256 + 8 pad: rows 16 B aligned, 4-bank skew)
#define NM_LP 36          // floats per logit-tile row

__device__ __forceinline__ float nm_ln(float x) { return __builtin_amdgcn_logf(x) * LN2F; }

// SPLIT = the SPLIT-OPERAND form (precision "fp16": BASELINE.json's 1e-4 on every conditional, which 8- or 11-bit operands of the decoder dot
// products miss).  Every hidden state h and every decoder weight w is carried as TWO IEEE halves, x = hi + lo with hi = f16(x) and
// lo = f16(x - hi) (22 significant bits), and a logit is the f32 sum of three 16-bit matrix-core products  hi.hi + hi.lo + lo.hi  (the
// dropped lo.lo term is 2^-22 of a product): ~1e-6 of the vector scan's f32 arithmetic at the 16-bit MFMA rate.  (Round 3 first shipped
// this form on v_mfma_f32_16x16x4_f32 -- exact f32 products at 1/16 of the 16-bit rate: its two logit phases cost 0.9 of the launch's
// 2.8 ms at [1024,256,88,5]; measured by ablation, profiles/round3_d_nade_fwd_ablation.md.)  A state element is ONE 32-bit LDS word
// (hi in the low half, lo in the high half), unpacked into the two A fragments with v_perm_b32; the pre-activations live in registers
// (indirect register addressing), which keeps two workgroups on a CU.  w_dec comes from mnn_nade_f32_pack as f16 [d][hi | lo][Hn].
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
struct NmPairB { f16x8_t hi, lo; };                       // decoder fragment of one k-step: the weights' high and low halves
template <bool SPLIT> struct NmState;
template <> struct NmState<false> { typedef bf16_t T; static constexpr int PITCH = NM_PITCH; };
template <> struct NmState<true> { typedef unsigned T; static constexpr int PITCH = 260; };  // 260 words: rows 4 banks apart
// state word of x in (0, 1): hi = x truncated to f16's 11 significant bits (a mask: exact), lo = x - hi (exact in f32, at most 13 significant
// bits) rounded toward zero to f16 -- one v_and, one v_sub, one v_cvt_pkrtz; |x - (hi + lo)| < 2^-21 x (f16 subnormals: 2^-24 absolute)
__device__ __forceinline__ unsigned nm_pack_hl(float x) {
    const float hi = __uint_as_float(__float_as_uint(x) & 0xFFFFE000u);
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(hi, x - hi));
}

template <bool SPLIT>
struct NadeFwdSmemT {
    typename NmState<SPLIT>::T sH[32][NmState<SPLIT>::PITCH];            // current state of every row (as of the tile being processed)
    typename NmState<SPLIT>::T sF[32][NmState<SPLIT>::PITCH];            // states created by the flips of the tile (one chunk of 32 slots, row-major)
    float sLb[32][NM_LP];               // logits of the base states  [row][column]
    float sLf[32][NM_LP];               // logits of the flip states  [slot][column]
    unsigned sMask[2][32];              // v bits of the tile, per row (double buffered: tile c, tile c+1)
    unsigned sSb[2][32];                // flips of the owning wave's rows in front of the row (the wave adds the flips of the waves before it)
    unsigned sCnt[2][4];                // flips of the tile in each wave's eight rows
    unsigned char sFl[2][4][256];       // each wave's flips in row-major order: (row - 8w) << 5 | column
};

// 16 rows x K=256 of a state tile as MFMA A fragments (lane: row l & 15, k = 32 s + 8 (l >> 4) + j)
__device__ __forceinline__ void nm_load_a(const bf16_t (*tile)[NM_PITCH], int mi, int lane, bf16x8_t (&a)[8]) {
    const bf16_t* p = &tile[16 * mi + (lane & 15)][8 * (lane >> 4)];
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = *reinterpret_cast<const bf16x8_t*>(p + 32 * s);
}
template <bool SPLIT> __device__ __forceinline__ typename NmState<SPLIT>::T nm_state(float h) {
    if constexpr (SPLIT) return nm_pack_hl(h);
    else return f32_to_bf16(h);
}
// 16 x 16 logits of one state tile against the tile's decoder rows
__device__ __forceinline__ f32x4_t nm_dot(const bf16x8_t (&af)[8], const bf16x8_t (&bfr)[8]) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s], bfr[s], acc, 0, 0, 0);
    return acc;
}
// split-operand form: 16 rows x K = 256 of a packed state tile against the wave's 16 decoder columns.  Lane (row l & 15, k group l >> 4) reads
// its 8 packed words of a k-step with two 16-byte LDS loads (rows 4 banks apart: conflict-free) and splits them into the hi and lo fragments.
__device__ __forceinline__ f32x4_t nm_dot_hl(const unsigned (*tile)[260], int mi, int lane, const NmPairB (&bw)[8]) {
    const unsigned* p = &tile[16 * mi + (lane & 15)][8 * (lane >> 4)];
    f32x4_t accm = {0.f, 0.f, 0.f, 0.f}, accs = {0.f, 0.f, 0.f, 0.f};     // main term | the two small terms: two independent chains
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const uint4 q0 = *reinterpret_cast<const uint4*>(p + 32 * s), q1 = *reinterpret_cast<const uint4*>(p + 32 * s + 4);
        uint4 uh, ul;
        uh.x = __builtin_amdgcn_perm(q0.y, q0.x, 0x05040100u); ul.x = __builtin_amdgcn_perm(q0.y, q0.x, 0x07060302u);
        uh.y = __builtin_amdgcn_perm(q0.w, q0.z, 0x05040100u); ul.y = __builtin_amdgcn_perm(q0.w, q0.z, 0x07060302u);
        uh.z = __builtin_amdgcn_perm(q1.y, q1.x, 0x05040100u); ul.z = __builtin_amdgcn_perm(q1.y, q1.x, 0x07060302u);
        uh.w = __builtin_amdgcn_perm(q1.w, q1.z, 0x05040100u); ul.w = __builtin_amdgcn_perm(q1.w, q1.z, 0x07060302u);
        const f16x8_t ah = __builtin_bit_cast(f16x8_t, uh), al = __builtin_bit_cast(f16x8_t, ul);
        accs = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bw[s].lo, accs, 0, 0, 0);
        accm = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bw[s].hi, accm, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bw[s].hi, accs, 0, 0, 0);
    }
    return accm + accs;
}
// One 32 x 32 logit tile of a state tile: wave (mi, ni) = w & 1, w >> 1 writes its 16 x 16 quadrant.
template <bool SPLIT, typename Tile, typename B>
__device__ __forceinline__ void nm_logit_tile(const Tile& tile, int w, int lane, const B& bfr, float (*out)[NM_LP]) {
    const int ni = w >> 1, mi = w & 1;
    f32x4_t acc;
    if constexpr (SPLIT) {
        acc = nm_dot_hl(tile, mi, lane, bfr);
    } else {
        bf16x8_t af[8];
        nm_load_a(tile, mi, lane, af);
        acc = nm_dot(af, bfr);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) out[16 * mi + 4 * (lane >> 4) + i][16 * ni + (lane & 15)] = acc[i];
}

// Ownership of the sparse side: WAVE w owns rows 8w .. 8w+7 of the workgroup -- their v bytes, their flips, their pre-activations and their
// part of the flip list -- and a LANE owns the four consecutive hidden units 4 lane .. 4 lane + 3.  The 8 x 4 pre-activations live in
// registers, indexed by the (wave-uniform) row of each flip -- the compiler lowers that to s_set_gpr_idx, no scratch.  A flip is executed by
// ONE wave for all 256 hidden units: 4 adds, 4 sigmoids, 4 state words, one 16-byte (bf16 form: 8-byte) LDS store into its slot of sF and one
// into its row of sH; what a flip costs besides (list entry, register index, addresses) is paid once per 256 units.
// Slots are ROW-MAJOR: slot of (row n, its j-th flip) = flips of the rows before n + j, so a wave's flips are consecutive slots, a row's flips
// keep their column order across the 32-slot chunks, and no wave builds a list for the others: each derives its entries from the ballots of
// its own rows and learns the other waves' counts (sCnt) at the tile's first barrier.
#define NM_P 12           // w_enc rows a wave fetches a tile ahead (16 bytes per lane each); a wave's flips beyond them are fetched in place
typedef float nm_f2 __attribute__((ext_vector_type(2)));
typedef float nm_f4u __attribute__((ext_vector_type(4), aligned(4)));          // 16-byte global access at 4-byte alignment (rows of `bias` at any ld_bias)
template <bool SPLIT>
__device__ __forceinline__ void
nade_fwd_mfma_body(int tracks, int N, int D, const uint8_t* __restrict__ v, long v_track_stride, const float* __restrict__ bias, int ld_bias,
                     const float* __restrict__ w_enc, const bf16_t* __restrict__ w_dec_bf, const float* __restrict__ row_weight,
                     float* __restrict__ nll, float* __restrict__ cond_p, float* __restrict__ d_bias, float* __restrict__ a_final,
                     const int* __restrict__ gate, int run_if, const int* __restrict__ n_rows_dev) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    typedef NadeFwdSmemT<SPLIT> NadeFwdSmem;
    typedef typename std::conditional<SPLIT, uint4, ushort4>::type state4_t;      // the four states of a lane: one LDS store
    typedef typename std::conditional<SPLIT, NmPairB, bf16x8_t>::type bfrag_t;
    constexpr int KS = 8;                                    // k-steps of 32 hidden units
    constexpr int P = NM_P;
    static_assert(P % 4 == 0 && P <= 16, "the prefetched rows are handled four at a time; their list entries sit in lanes 0..15");
    NadeFwdSmem& S = *reinterpret_cast<NadeFwdSmem*>(smem_raw);
    if (gate != nullptr && *gate != run_if) return;          // density-gated pair of launches: uniform exit
    constexpr int Hn = NM_H;
    const int m = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ni = w >> 1;                                   // this wave's column half of a 32 x 32 logit tile (w & 1: its row half / K half)
    const int rb = blockIdx.x * 32;
    const uint8_t* __restrict__ vm = v + (size_t)m * v_track_stride;
    const float* __restrict__ we = w_enc + (size_t)m * D * Hn;
    const bf16_t* __restrict__ wd = w_dec_bf + (size_t)m * D * Hn * (SPLIT ? 2 : 1);        // (split form: f16 [d][hi | lo][Hn] behind the 16-bit pointer type)
    const int bd_off = tracks * Hn + m * D;
    const int ntile = (D + 31) / 32;
    // compacted ragged batch (mnn_ragged_index; see nade.hip): a workgroup whose 32 rows are all padding writes the zeros later kernels read and leaves
    if (n_rows_dev != nullptr && rb >= *n_rows_dev) {
        if (d_bias != nullptr)
            for (int e = tid; e < 32 * D; e += 256) {
                const int n = e / D, i = e - n * D;
                if (rb + n < N) d_bias[(size_t)(rb + n) * ld_bias + bd_off + i] = 0.f;
            }
        if (nll != nullptr && tid < 32 && rb + tid < N) nll[(size_t)m * N + rb + tid] = 0.f;
        return;
    }

    auto state4 = [&](const float (&x)[4]) {
        state4_t h;
        h.x = nm_state<SPLIT>(fast_sigmoid(x[0])); h.y = nm_state<SPLIT>(fast_sigmoid(x[1]));
        h.z = nm_state<SPLIT>(fast_sigmoid(x[2])); h.w = nm_state<SPLIT>(fast_sigmoid(x[3]));
        return h;
    };
    // pre-activations of this wave's 8 rows x this lane's 4 hidden units: registers, indexed by the wave-uniform row of a flip.  Held as
    // two arrays of eight 64-BIT words (units 0, 1 | units 2, 3 of a row): an indexed move then carries two units, and the two arrays share one
    // index, so a row is read with one s_set_gpr_idx_on / off pair around two 64-bit moves and written with another (a float[32] took a pair
    // per unit and direction; arrays of eight 32-bit words are compiled into select chains)
    unsigned long long a01[8], a23[8];
    auto pair_of = [](float lo, float hi) { return __builtin_bit_cast(unsigned long long, (nm_f2){lo, hi}); };
    {
        // all 8 encoder-bias loads in flight before the first is used (unconditional, from clamped rows)
        nm_f4 av[8];
#pragma unroll
        for (int r = 0; r < 8; ++r)
            av[r] = *reinterpret_cast<const nm_f4u*>(&bias[(size_t)min(rb + 8 * w + r, N - 1) * ld_bias + m * Hn + 4 * lane]);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = rb + 8 * w + r < N ? av[r][q] : 0.f;
            a01[r] = pair_of(x[0], x[1]); a23[r] = pair_of(x[2], x[3]);
            *reinterpret_cast<state4_t*>(&S.sH[8 * w + r][4 * lane]) = state4(x);
        }
    }
    // v bytes of rows 8w .. 8w+7 of a tile: lane -> (row 8w + 2i + (lane >> 5), column lane & 31)
    auto load_v = [&](int c, unsigned char (&vb)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = min(rb + 8 * w + 2 * i + (lane >> 5), N - 1), dd = min(32 * c + (lane & 31), D - 1);
            vb[i] = vm[(size_t)row * D + dd];
        }
    };
    // The wave's share of a tile's bookkeeping, from the four ballots of its rows: the rows' masks, the flips in front of each row, the wave's
    // flips in row-major order (ballot i covers rows 2i, 2i+1, so entry = 64 i + lane = (row - 8w) << 5 | column and its rank is the count of
    // set bits below it) and the wave's count.  Returns the count.
    auto ballots = [&](int c, const unsigned char (&vb)[4], int b) {
        int cum = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = rb + 8 * w + 2 * i + (lane >> 5), dd = 32 * c + (lane & 31);
            const bool on = row < N && dd < D && vb[i] != 0;
            const unsigned long long bal = __ballot(on);
            const unsigned lo = (unsigned)bal, hi = (unsigned)(bal >> 32);
            if ((lane & 31) == 0) {
                S.sMask[b][8 * w + 2 * i + (lane >> 5)] = lane ? hi : lo;
                S.sSb[b][8 * w + 2 * i + (lane >> 5)] = (unsigned)(cum + (lane ? __popc(lo) : 0));
            }
            if (on) S.sFl[b][w][cum + (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u))] = (unsigned char)(64 * i + lane);
            cum += __popcll(bal);
        }
        if (lane == 0) S.sCnt[b][w] = (unsigned)cum;
        return cum;
    };
    auto load_b = [&](int c, bfrag_t (&b)[KS]) {            // lane: column l & 15 of the wave's column half, k = 32 s + 8 (l >> 4) + j
        const int d = min(32 * c + 16 * ni + (lane & 15), D - 1);
        if constexpr (SPLIT) {                                // [d][hi | lo][Hn] f16
            const f16_t* p = reinterpret_cast<const f16_t*>(wd) + (size_t)d * 2 * Hn + 8 * (lane >> 4);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                b[s].hi = *reinterpret_cast<const f16x8_t*>(p + 32 * s);
                b[s].lo = *reinterpret_cast<const f16x8_t*>(p + Hn + 32 * s);
            }
        } else {
            const bf16_t* p = wd + (size_t)d * Hn + 8 * (lane >> 4);
#pragma unroll
            for (int s = 0; s < KS; ++s) b[s] = *reinterpret_cast<const bf16x8_t*>(p + 32 * s);
        }
    };
    // w_enc[column of the wave's flip j0 + u][this lane's 4 hidden units], u < P, for the flips below jend; four at a time, a group with no flip
    // is not requested (the values of entries past jend inside a group are never used: their list bytes are stale, their columns clamped)
    const __amdgpu_buffer_rsrc_t we_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(we), 0, D * Hn * 4, 0x00020000);
    auto load_we = [&](int c, int b, int j0, int jend, nm_f4 (&wv)[P]) {
        // ONE list read per lane (lane u holds entry j0 + u), the entries then come out of the lanes with v_readlane
        const int entv = (int)S.sFl[b][w][min(j0 + (lane & 15), 255)];
#pragma unroll
        for (int g = 0; g < P; g += 4) {
            if (j0 + g < jend) {
#pragma unroll
                for (int u = g; u < g + 4; ++u) {
                    // buffer load: the row offset rides in the instruction's SCALAR offset operand, the lane offset (16 lane) is one loop-invariant register
                    const int e = __builtin_amdgcn_readlane(entv, u);
                    wv[u] = __builtin_bit_cast(nm_f4, __builtin_amdgcn_raw_buffer_load_b128(we_rs, lane * 16, min(32 * c + (e & 31), D - 1) * (Hn * 4), 0));
                }
            }
        }
    };
    unsigned char vb[4];
    bfrag_t bfr[KS];
    nm_f4 wev[P];
    load_v(0, vb);
    load_b(0, bfr);
    int nxt_cnt = ballots(0, vb, 0);                         // this wave's flips in the tile ahead
    if (ntile > 1) load_v(1, vb);
    load_we(0, 0, 0, nxt_cnt, wev);                          // the wave's own list: ordered by the wave's own LDS queue
    __syncthreads();

    // epilogue ownership: thread -> row n = tid >> 3 (one of its wave's rows), columns 4 (tid & 7) + k
    const int en = tid >> 3, ed0 = 4 * (tid & 7), erow = rb + en;
    const bool evalid = erow < N;
    const int err = evalid ? erow : N - 1;
    const float rw = (row_weight != nullptr && evalid) ? row_weight[erow] : 0.f;
    float lp = 0.f;
#ifdef NM_TRACE
    long long tprev_ = wall_clock64();
#endif
    for (int c = 0; c < ntile; ++c) {
        const int buf = c & 1, nbuf = buf ^ 1;
        // ---- S0: base logits; the next tile's operands start flying ----
        float bdec[4];
        {
            const float* bp = bias + (size_t)err * ld_bias + bd_off + 32 * c + ed0;
            if (32 * c + ed0 + 3 < D && (((size_t)bp) & 15) == 0) {             // one 16-byte request instead of four
                const float4 b4 = *reinterpret_cast<const float4*>(bp);
                bdec[0] = b4.x; bdec[1] = b4.y; bdec[2] = b4.z; bdec[3] = b4.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) bdec[k] = bias[(size_t)err * ld_bias + bd_off + min(32 * c + ed0 + k, D - 1)];
            }
        }
        // (Requesting these and the v bytes in the middle of the tile before instead -- so that the flip pass, whose generated waits drain the
        // memory queue by its last flip, never waits at HBM latency -- was measured: 2.18 -> 2.25 ms, not kept.)
        __builtin_amdgcn_sched_barrier(0);
        nm_logit_tile<SPLIT>(S.sH, w, lane, bfr, S.sLb);
        if (c + 1 < ntile) {
            nxt_cnt = ballots(c + 1, vb, nbuf);              // v bytes requested one tile ago
            if (c + 2 < ntile) load_v(c + 2, vb);
        }
        NM_T(0);
        hf_lds_barrier();                                     // B1: sLb complete, sH consumed, the waves' counts written
        NM_T(1);
        // every wave's count of the tile: the wave's first slot and the tile's total, as scalars
        const int cntv = (int)S.sCnt[buf][lane & 3];
        const int c0 = __builtin_amdgcn_readlane(cntv, 0), c1 = __builtin_amdgcn_readlane(cntv, 1), c2 = __builtin_amdgcn_readlane(cntv, 2),
                  c3 = __builtin_amdgcn_readlane(cntv, 3);
        const int F = c0 + c1 + c2 + c3;
        const int wbase = (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0);
        const int wcnt = w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
        const unsigned mk = S.sMask[buf][en];
        const int sb = wbase + (int)S.sSb[buf][en];          // slot of the row's first flip
        float lsel[4];                                       // the logit of each of this thread's 4 (row, column) pairs
        int slot_of[4];                                      // slot of the state each pair uses: the row's latest flip before the column
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int jj = __popc(mk & ((1u << (ed0 + k)) - 1u));               // flips of this row strictly before the column
            slot_of[k] = jj > 0 ? sb + jj - 1 : -1;
            lsel[k] = S.sLb[en][ed0 + k];
        }
        for (int k0 = 0; k0 < F; k0 += 32) {
            // ---- S1: the wave's flips whose slots lie in this chunk (j = index among the wave's flips of the tile, slot = wbase + j), in
            //      row-major order: a[row] += w_enc[d]; new state -> sF[slot] and the row's current state.  P at a time, the first P of a
            //      tile from the rows fetched a tile ahead.
            const int jhi = min(k0 + 32 - wbase, wcnt);
            for (int jb = max(k0 - wbase, 0); jb < jhi; jb += P) {
                if (jb > 0) load_we(c, buf, jb, jhi, wev);   // beyond the prefetched rows (or a second chunk): fetched in place
                const int cnt = jhi - jb;
                const int flv = (int)S.sFl[buf][w][min(jb + (lane & 15), jhi - 1)];      // the batch's list entries, one per lane (see load_we)
#pragma unroll
                for (int u0 = 0; u0 < P; u0 += 4) {
                    if (u0 < cnt) {
                        // One flip after the other, in list order (a row may appear more than once), each under its own wave-uniform branch:
                        // two 64-bit indexed reads, two packed adds, two 64-bit indexed writes (in place: the branch costs no register copies),
                        // then four sigmoids and state words.  (Four flips interleaved without branches -- entries past the count adding 0 to
                        // the last flip's row -- cost four selects per flip and measured the same: the flip pass is bound by its 8
                        // transcendentals and ~45 other instructions per flip, and the other workgroup's wave fills the latencies.)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            if (u0 + i < cnt) {
                                const int r = __builtin_amdgcn_readlane(flv, u0 + i) >> 5;
                                const nm_f2 p01 = __builtin_bit_cast(nm_f2, a01[r]), p23 = __builtin_bit_cast(nm_f2, a23[r]);
                                const float x[4] = {p01[0] + wev[u0 + i][0], p01[1] + wev[u0 + i][1], p23[0] + wev[u0 + i][2], p23[1] + wev[u0 + i][3]};
                                a01[r] = pair_of(x[0], x[1]); a23[r] = pair_of(x[2], x[3]);
                                __builtin_amdgcn_sched_barrier(0);        // the four indexed moves of the write stay adjacent: one index-mode pair, not three
                                const state4_t hb = state4(x);
                                *reinterpret_cast<state4_t*>(&S.sF[wbase + jb + u0 + i - k0][4 * lane]) = hb;
                                *reinterpret_cast<state4_t*>(&S.sH[8 * w + r][4 * lane]) = hb;
                            }
                        }
                    }
                }
            }
            NM_T(2);
            NM_T(3);
            hf_lds_barrier();                                 // B2: sF complete
            NM_T(4);
            // ---- S2: flip logits; each pair whose state sits in this chunk picks its logit ----
            nm_logit_tile<SPLIT>(S.sF, w, lane, bfr, S.sLf);
            if (k0 + 32 >= F && c + 1 < ntile) load_we(c + 1, nbuf, 0, nxt_cnt, wev);    // behind the tile's last MFMAs: the next tile's encoder rows
            NM_T(5);
            hf_lds_barrier();                                 // B3: sLf ready
            NM_T(6);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int slot = slot_of[k] - k0;
                if (slot_of[k] >= 0 && slot >= 0 && slot < 32) lsel[k] = S.sLf[slot][ed0 + k];
            }
        }
        if (F == 0 && c + 1 < ntile) {                       // no flip in this tile: sLb, the masks and the counts are still read; the next S0 writes them
            hf_lds_barrier();
            load_we(c + 1, nbuf, 0, nxt_cnt, wev);
        }
        // b_dec of this tile (requested at its top) is waited for HERE, in front of the w_dec request: the wait the compiler puts in front of
        // the pointwise must hold on every path that reaches it (also the last tile's, which requests nothing), so it is `vmcnt(3)` -- placed
        // behind the 16 w_dec loads it made the pointwise wait for all of them (2.47 -> 2.18 ms with the batched bias loads above)
#pragma unroll
        for (int k = 0; k < 4; ++k) asm volatile("" :: "v"(bdec[k]));
        if (c + 1 < ntile) load_b(c + 1, bfr);               // the tile's MFMAs are issued: fetch the next tile's w_dec fragments under the pointwise
        NM_T(7);
        // ---- S3: pointwise of this thread's 4 pairs, once per tile; the four results of a matrix leave as ONE 16-byte store where the
        //      four columns exist and the address is aligned (one store instruction instead of four per matrix and tile)
        float prv[4], dbv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dpos = ed0 + k, gd = 32 * c + dpos;
            prv[k] = 0.f; dbv[k] = 0.f;
            if (gd >= D) continue;
            const float l = bdec[k] + lsel[k];
            const bool on = (mk >> dpos) & 1u;
            const float pr = fast_sigmoid(l);
            const float qr = fast_sigmoid(-l);               // 1-p without cancellation
            lp += on ? nm_ln(NADE_EPS + pr) : nm_ln(NADE_EPS + qr);
            prv[k] = pr;
            const float dnll_dp = on ? -fast_rcp(NADE_EPS + pr) : fast_rcp(NADE_EPS + qr);
            dbv[k] = rw * dnll_dp * pr * qr;
        }
        if (evalid) {
            const int gd0 = 32 * c + ed0;
            const bool full = gd0 + 3 < D;
            if (cond_p != nullptr) {
                float* dst = cond_p + ((size_t)m * N + erow) * D + gd0;
                if (full && (((size_t)dst) & 15) == 0) NM_ST4(dst, prv);
                else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (gd0 + k < D) dst[k] = prv[k];
                }
            }
            if (d_bias != nullptr) {
                float* dst = d_bias + (size_t)erow * ld_bias + bd_off + gd0;
                if (full && (((size_t)dst) & 15) == 0) NM_ST4(dst, dbv);
                else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (gd0 + k < D) dst[k] = dbv[k];
                }
            }
        }
        NM_T(8);
    }
    lp += __shfl_xor(lp, 1);
    lp += __shfl_xor(lp, 2);
    lp += __shfl_xor(lp, 4);
    if ((tid & 7) == 0 && evalid && nll != nullptr) nll[(size_t)m * N + erow] = -lp;
    if (a_final != nullptr) {
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (rb + 8 * w + r < N)
                __builtin_nontemporal_store(__builtin_shufflevector(__builtin_bit_cast(nm_f2, a01[r]), __builtin_bit_cast(nm_f2, a23[r]), 0, 1, 2, 3),
                                            reinterpret_cast<nm_f4u*>(&a_final[((size_t)m * N + rb + 8 * w + r) * Hn + 4 * lane]));
    }
}

// two entry points over the one body: the split form is held to 256 registers (two workgroups per CU), the bf16 form keeps its own allocation
template <bool SPLIT> __global__ void nade_fwd_mfma_kernel(int, int, int, const uint8_t*, long, const float*, int, const float*, const bf16_t*, const float*,
                                                           float*, float*, float*, float*, const int*, int, const int*);
template <>
__global__ void __launch_bounds__(256)
nade_fwd_mfma_kernel<false>(int tracks, int N, int D, const uint8_t* __restrict__ v, long v_track_stride, const float* __restrict__ bias, int ld_bias,
                            const float* __restrict__ w_enc, const bf16_t* __restrict__ w_dec_bf, const float* __restrict__ row_weight,
                            float* __restrict__ nll, float* __restrict__ cond_p, float* __restrict__ d_bias, float* __restrict__ a_final,
                            const int* __restrict__ gate, int run_if, const int* __restrict__ n_rows_dev) {
    nade_fwd_mfma_body<false>(tracks, N, D, v, v_track_stride, bias, ld_bias, w_enc, w_dec_bf, row_weight, nll, cond_p, d_bias, a_final, gate, run_if, n_rows_dev);
}
template <>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
nade_fwd_mfma_kernel<true>(int tracks, int N, int D, const uint8_t* __restrict__ v, long v_track_stride, const float* __restrict__ bias, int ld_bias,
                           const float* __restrict__ w_enc, const bf16_t* __restrict__ w_dec_bf, const float* __restrict__ row_weight,
                           float* __restrict__ nll, float* __restrict__ cond_p, float* __restrict__ d_bias, float* __restrict__ a_final,
                           const int* __restrict__ gate, int run_if, const int* __restrict__ n_rows_dev) {
    nade_fwd_mfma_body<true>(tracks, N, D, v, v_track_stride, bias, ld_bias, w_enc, w_dec_bf, row_weight, nll, cond_p, d_bias, a_final, gate, run_if, n_rows_dev);
}

extern "C" int mnn_nade_mfma_ok(int Hn) { return Hn == NM_H ? 1 : 0; }

extern "C" int mnn_nade_logprob_fwd_mfma(mnn_stream_t s, int tracks, int N, int D, int Hn, const uint8_t* v, long v_track_stride,
                                         const float* bias, int ld_bias, const float* w_enc, const void* w_dec_bf16, const float* row_weight,
                                         float* nll, float* cond_p, float* d_bias, float* a_final) {
    return mnn_nade_logprob_fwd_mfma_gated(s, tracks, N, D, Hn, v, v_track_stride, bias, ld_bias, w_enc, w_dec_bf16, row_weight, nll, cond_p, d_bias,
                                           a_final, nullptr, 0, nullptr);
}

template <bool SPLIT>
static int nm_launch(mnn_stream_t s, int tracks, int N, int D, int Hn, const uint8_t* v, long v_track_stride, const float* bias, int ld_bias,
                     const float* w_enc, const void* w_dec16, const float* row_weight, float* nll, float* cond_p, float* d_bias, float* a_final,
                     const int* gate, int run_if, const int* n_rows_dev) {
    MNN_REQUIRE(tracks > 0 && N > 0 && D > 0 && Hn == NM_H, "mnn_nade_logprob_fwd_mfma: need tracks,N,D>0 and Hn == 256 (Hn=%d)", Hn);
    MNN_REQUIRE(v && bias && w_enc && w_dec16, "mnn_nade_logprob_fwd_mfma: null pointer");
    MNN_REQUIRE(ld_bias >= tracks * (Hn + D), "mnn_nade_logprob_fwd_mfma: ld_bias %d < tracks*(Hn+D)", ld_bias);
    MNN_REQUIRE(d_bias == nullptr || row_weight != nullptr, "mnn_nade_logprob_fwd_mfma: d_bias needs row_weight");
    MNN_REQUIRE(((uintptr_t)w_dec16 & 15) == 0, "mnn_nade_logprob_fwd_mfma: the 16-bit decoder weights must be 16-byte aligned");
    static_assert(sizeof(NadeFwdSmemT<SPLIT>) <= 80 * 1024, "two workgroups share a CU's 160 KB of LDS");
    static MnnPerDeviceOnce raised;                            // (per SPLIT: this function is instantiated once per form)
    MNN_HIP(mnn_once_per_device(raised, [] { return mnn_raise_dynamic_lds((const void*)nade_fwd_mfma_kernel<SPLIT>, (int)sizeof(NadeFwdSmemT<SPLIT>)); }));
    dim3 grid(cdiv(N, 32), tracks);
    hipLaunchKernelGGL(nade_fwd_mfma_kernel<SPLIT>, grid, dim3(256), sizeof(NadeFwdSmemT<SPLIT>), (hipStream_t)s, tracks, N, D, v, v_track_stride, bias,
                       ld_bias, w_enc, (const bf16_t*)w_dec16, row_weight, nll, cond_p, d_bias, a_final, gate, run_if, n_rows_dev);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

extern "C" int mnn_nade_logprob_fwd_mfma_gated(mnn_stream_t s, int tracks, int N, int D, int Hn, const uint8_t* v, long v_track_stride,
                                               const float* bias, int ld_bias, const float* w_enc, const void* w_dec_bf16, const float* row_weight,
                                               float* nll, float* cond_p, float* d_bias, float* a_final, const int* gate, int run_if, const int* n_rows_dev) {
    return nm_launch<false>(s, tracks, N, D, Hn, v, v_track_stride, bias, ld_bias, w_enc, w_dec_bf16, row_weight, nll, cond_p, d_bias, a_final, gate, run_if, n_rows_dev);
}

extern "C" int mnn_nade_logprob_fwd_mfma_f32(mnn_stream_t s, int tracks, int N, int D, int Hn, const uint8_t* v, long v_track_stride,
                                             const float* bias, int ld_bias, const float* w_enc, const void* w_dec_packed, const float* row_weight,
                                             float* nll, float* cond_p, float* d_bias, float* a_final, const int* gate, int run_if, const int* n_rows_dev) {
    return nm_launch<true>(s, tracks, N, D, Hn, v, v_track_stride, bias, ld_bias, w_enc, w_dec_packed, row_weight, nll, cond_p, d_bias, a_final, gate, run_if, n_rows_dev);
}

// w_dec f32 [rows, Hn] -> f16 [rows][hi | lo][Hn]: the B operand of the split-operand form (4 bytes per weight, as the f32 original)
__global__ void __launch_bounds__(256) nade_f32_pack_kernel(const float* __restrict__ w, long n, int Hn, float* __restrict__ out) {
    f16_t* o = reinterpret_cast<f16_t*>(out);
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long row = e / Hn;
        const int k = (int)(e - row * Hn);
        const float x = w[e];
        const f16_t hi = (f16_t)x;
        o[row * 2 * Hn + k] = hi;
        o[row * 2 * Hn + Hn + k] = (f16_t)(x - (float)hi);
    }
}
extern "C" int mnn_nade_f32_pack(mnn_stream_t s, const float* w_dec, long rows, int Hn, float* out) {
    MNN_REQUIRE(w_dec && out && rows > 0 && Hn > 0 && Hn % 8 == 0, "mnn_nade_f32_pack: bad arguments (Hn must be a multiple of 8)");
    MNN_REQUIRE(((uintptr_t)out & 15) == 0, "mnn_nade_f32_pack: the packed buffer must be 16-byte aligned");
    const long n = rows * Hn;
    hipLaunchKernelGGL(nade_f32_pack_kernel, dim3((int)std::min(2048L, (n + 255) / 256)), dim3(256), 0, (hipStream_t)s, w_dec, n, Hn, out);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}
