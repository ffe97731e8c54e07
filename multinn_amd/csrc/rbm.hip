// RBM CD-k Gibbs chain (single launches), half-steps and free energy for gfx950.
// Reference: /root/reference/multinn/models/common/rbm.py:148-263, 337-387.
//
// The chain itself -- bodies, kernels and the dispatch between its three forms -- is rbm_chain.h, shared with the grouped launches of
// rbm_multi.hip; this file holds the entry points of the single chain, which fill a one-job argument block and call that dispatch.
// Summation order is ascending input index with one fma per term, and the sigmoid uses IEEE ops
// only, so Bernoulli draws are bit-identical to oracle/det_ref.c.
#include "rbm_chain.h"      // the chain, RBM_R, rbm_phase, the matrix-core helpers

// ----------------------------------------------------------------------------------------------
// k-step Gibbs chain (rbm.py:192-231)
//
// GIVEN (the clamped chain of conditional sampling; every form has one): `given` u8 [N, ld_given], 0 / 1 clamp the visible to that
// value, 255 leaves it free.  The chain starts from v0 with the clamped cells replaced by their codes; every hidden phase is today's; in every
// visible phase a clamped cell keeps its code and leaves its uniform unused, a free cell draws from the uniform it draws unconditioned (the
// counters are per cell: nothing shifts).  p_v is sigmoid(logit) at every cell, clamped ones included.
// TEMPERED (sampling at a temperature other than 1: generation only, training's stepped chain has none): see GibbsView.  A temperature of
// exactly 1 is the untempered kernels, bit for bit and launch for launch.
// ----------------------------------------------------------------------------------------------
extern "C" size_t mnn_rbm_workspace_bytes(int D, int Hn) { return (size_t)D * Hn * sizeof(float); }

static int gibbs_single(const char* who, mnn_stream_t s, int N, int D, int Hn, int k, const uint8_t* v0, const float* W, const float* bh, int ld_bh,
                        const float* bv, int ld_bv, uint64_t seed, uint32_t row0, const uint32_t* row_ids, uint32_t sub0, float* p_v, uint8_t* v_out,
                        void* workspace, const int* seed_step, const uint8_t* given, int ld_given, float temperature,
                        const uint32_t* sub_base = nullptr) {
    const uint32_t sub_scale = (uint32_t)(k > 1 ? k : 1);      // a generated step uses max(k, 1) sub-counters
    MNN_REQUIRE(temperature > 0.f && temperature <= 3.0e38f, "%s: the temperature is a positive finite number (%g)", who, (double)temperature);
    MNN_REQUIRE(given == nullptr || ld_given >= D, "%s: ld_given=%d < D=%d", who, ld_given, D);
    if (temperature != 1.0f) {
        GibbsArgs<true> A{N, D, Hn, k, v0, W, nullptr, bh, ld_bh, bv, ld_bv, seed, row0, row_ids, sub0, p_v, v_out, given, ld_given, temperature, seed_step, sub_base, sub_scale};
        return rbm_gibbs_dispatch(who, s, A, workspace);
    }
    GibbsArgs<false> A{N, D, Hn, k, v0, W, nullptr, bh, ld_bh, bv, ld_bv, seed, row0, row_ids, sub0, p_v, v_out, given, ld_given, 1.0f, seed_step, sub_base, sub_scale};
    return rbm_gibbs_dispatch(who, s, A, workspace);
}

extern "C" int mnn_rbm_gibbs_temp(mnn_stream_t s, int N, int D, int Hn, int k, const uint8_t* v0, const float* W, const float* bh, int ld_bh,
                                  const float* bv, int ld_bv, uint64_t seed, uint32_t row0, const uint32_t* row_ids, uint32_t sub0, float* p_v,
                                  uint8_t* v_out, void* workspace, const uint8_t* given, int ld_given, float temperature) {
    return gibbs_single("mnn_rbm_gibbs_temp", s, N, D, Hn, k, v0, W, bh, ld_bh, bv, ld_bv, seed, row0, row_ids, sub0, p_v, v_out, workspace, nullptr, given,
                        ld_given, temperature);
}

// mnn_rbm_gibbs_temp with a sub-counter base read on the device (sub_base: NULL, or one u32 -- the generated steps before this launch): the
// chain draws with sub-counters sub0 + *sub_base * max(k, 1) + iteration.  A captured launch follows the cell from replay to replay.
extern "C" int mnn_rbm_gibbs_at(mnn_stream_t s, int N, int D, int Hn, int k, const uint8_t* v0, const float* W, const float* bh, int ld_bh,
                                const float* bv, int ld_bv, uint64_t seed, uint32_t row0, const uint32_t* row_ids, uint32_t sub0, float* p_v,
                                uint8_t* v_out, void* workspace, const uint8_t* given, int ld_given, float temperature, const uint32_t* sub_base) {
    return gibbs_single("mnn_rbm_gibbs_at", s, N, D, Hn, k, v0, W, bh, ld_bh, bv, ld_bv, seed, row0, row_ids, sub0, p_v, v_out, workspace, nullptr, given,
                        ld_given, temperature, sub_base);
}

extern "C" int mnn_rbm_gibbs_stepped(mnn_stream_t s, int N, int D, int Hn, int k, const uint8_t* v0, const float* W, const float* bh, int ld_bh,
                                     const float* bv, int ld_bv, uint64_t seed, uint32_t row0, const uint32_t* row_ids, uint32_t sub0, float* p_v,
                                     uint8_t* v_out, void* workspace, const int* seed_step) {
    return gibbs_single("mnn_rbm_gibbs_stepped", s, N, D, Hn, k, v0, W, bh, ld_bh, bv, ld_bv, seed, row0, row_ids, sub0, p_v, v_out, workspace, seed_step,
                        nullptr, 0, 1.0f);
}

extern "C" int mnn_rbm_gibbs(mnn_stream_t s, int N, int D, int Hn, int k, const uint8_t* v0, const float* W, const float* bh, int ld_bh,
                             const float* bv, int ld_bv, uint64_t seed, uint32_t row0, const uint32_t* row_ids, uint32_t sub0, float* p_v,
                             uint8_t* v_out, void* workspace, const uint8_t* given, int ld_given) {
    return gibbs_single("mnn_rbm_gibbs", s, N, D, Hn, k, v0, W, bh, ld_bh, bv, ld_bv, seed, row0, row_ids, sub0, p_v, v_out, workspace, nullptr, given,
                        ld_given, 1.0f);
}

// ----------------------------------------------------------------------------------------------
// half-steps (rbm.py:148-190) -- also the DBN encode / decode steps (dbn.py:136-180)
// ----------------------------------------------------------------------------------------------
template <typename TV>
__global__ void __launch_bounds__(256)
rbm_half_kernel(int N, int K, int n_out, const TV* __restrict__ in, const float* __restrict__ Wk, int ldw, const float* __restrict__ b, int ld_b,
                int stream_id, uint64_t seed, uint32_t row0, uint32_t sub, float* __restrict__ p_out, uint8_t* __restrict__ s_out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Kp = (K + 3) & ~3;
    const int n0 = blockIdx.x * RBM_R;
    rbm_load_rows<TV>(in, N, n0, K, Kp, smem);
    __syncthreads();
    rbm_phase(smem, Kp, K, Wk, ldw, n_out, b, ld_b, n0, N, [&](int r, int o, float z) {
        const int n = n0 + r;
        if (n >= N) return;
        const float p = det_sigmoid(z);
        if (p_out) p_out[(size_t)n * n_out + o] = p;
        if (s_out) {
            const float u = philox_uniform1(seed, (uint32_t)stream_id, row0 + (uint32_t)n, sub, (uint32_t)o);
            s_out[(size_t)n * n_out + o] = u < p ? 1 : 0;
        }
    });
}

// The half-step on the f32 matrix cores (same ascending fmaf chain per output: see rbm_gibbs_mfma_body): 64 rows per workgroup, the rows'
// inputs in LDS as f32 [64][odd pitch], Wk [K][n_out] in LDS, C[out unit][row] tiles of 32 x 32 spread over the 8 waves; a lane's accumulator
// quad = four consecutive outputs of one row = one Philox block.  From 2048 rows on (DBN encode / decode of a training batch, dbn.py:136-180,
// and the free-energy gradient's hidden passes).
template <typename TV>
__global__ void __launch_bounds__(512)
rbm_half_mfma_kernel(int N, int K, int n_out, const TV* __restrict__ in, const float* __restrict__ Wk, int ldw, const float* __restrict__ b, int ld_b,
                     int stream_id, uint64_t seed, uint32_t row0, uint32_t sub, float* __restrict__ p_out, uint8_t* __restrict__ s_out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Ke = (K + 1) & ~1, lw = n_out | 1, pin = Ke | 1;
    float* Ws = smem;                       // [Ke][lw]
    float* xs = smem + (size_t)Ke * lw;     // [64][pin]
    float* tile_p = xs + (size_t)GM_ROWS * pin;                                   // [8 waves][32][33] f32: a job's probabilities, [row][unit]
    uint8_t* tile_s = reinterpret_cast<uint8_t*>(tile_p + 8 * 32 * 33);           // [8 waves][32][36] u8: its draws
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int k = w; k < Ke; k += 8)
        for (int o = lane; o < lw; o += 64) Ws[k * lw + o] = o < n_out ? Wk[(size_t)min(k, K - 1) * ldw + o] : 0.f;
    const int r = lane & 31, hh = lane >> 5;
    const int not_ = (n_out + 31) / 32;
    // persistent over 64-row tiles: the weights are fetched into LDS once per workgroup (one workgroup per CU), not once per 64 rows -- a
    // half-step has a single K-long chain per output, so a per-tile weight load (59 KB for 5.6 KB of inputs at 88 -> 168) was most of its time
    for (int tile = blockIdx.x; tile * GM_ROWS < N; tile += gridDim.x) {
        const int n0 = tile * GM_ROWS;
        __syncthreads();                                        // the previous tile's chains have read xs (first pass: Ws is complete)
        {   // the 64 rows' inputs: thread t -> row t >> 3, eight lanes walk its columns; sixteen loads in flight per thread (unconditional, clamped)
            const int rr = threadIdx.x >> 3, sub = threadIdx.x & 7, n = n0 + rr;
            const TV* __restrict__ src = in + (size_t)min(n, N - 1) * K;
            float* d = xs + rr * pin;
            for (int kb = sub; kb < pin; kb += 128) {
                TV v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = src[min(kb + 8 * q, K - 1)];
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (kb + 8 * q < pin) d[kb + 8 * q] = (n < N && kb + 8 * q < K) ? (float)v[q] : 0.f;
            }
        }
        __syncthreads();
        for (int job = w; job < 2 * not_; job += 8) {
            const int rt = job / not_, ot = job - rt * not_;
            gm_f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            const float* ap = Ws + (size_t)hh * lw + min(32 * ot + r, n_out - 1);
            const float* bp = xs + (32 * rt + r) * pin + hh;
            for (int s2 = 0; s2 < Ke / 2; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[(size_t)s2 * 2 * lw], bp[2 * s2], acc, 0, 0, 0);
            const int row = min(n0 + 32 * rt + r, N - 1);       // (rows past N repeat the last row; masked at the stores)
            // results through a wave-private LDS tile [row][unit], then out row-major: a lane holds four units of ONE row, so direct stores
            // would be 64 scattered 4-byte (and 1-byte) writes per instruction; from the tile every instruction writes two rows' 128-byte runs
            float* tp = tile_p + w * (32 * 33);
            uint8_t* ts = tile_s + w * (32 * 36);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int o0 = 32 * ot + 8 * g4 + 4 * hh;
                float u[4] = {0.f, 0.f, 0.f, 0.f};
                if (s_out) philox_uniform4(seed, (uint32_t)stream_id, row0 + (uint32_t)row, sub, (uint32_t)(o0 >> 2), u);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = min(o0 + e, n_out - 1);
                    const float p = det_sigmoid(acc[4 * g4 + e] + b[(size_t)row * ld_b + o]);
                    tp[r * 33 + 8 * g4 + 4 * hh + e] = p;
                    ts[r * 36 + 8 * g4 + 4 * hh + e] = u[e] < p ? 1 : 0;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's own LDS writes, then its reads (LDS serves a wave in order)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int idx = i * 64 + lane, rr = idx >> 5, cc = idx & 31;
                const int row2 = n0 + 32 * rt + rr, o = 32 * ot + cc;
                if (row2 < N && o < n_out) {
                    if (p_out) p_out[(size_t)row2 * n_out + o] = tp[rr * 33 + cc];
                    if (s_out) s_out[(size_t)row2 * n_out + o] = ts[rr * 36 + cc];
                }
            }
        }
    }
}
static size_t half_mfma_lds_bytes(int K, int n_out) {
    const int Ke = (K + 1) & ~1;
    return ((size_t)Ke * (n_out | 1) + (size_t)GM_ROWS * (Ke | 1) + 8 * 32 * 33) * sizeof(float) + 8 * 32 * 36;
}

static int launch_half(hipStream_t st, int N, int K, int n_out, const void* in, int in_dtype, const float* Wk, int ldw, const float* b,
                       int ld_b, int stream_id, uint64_t seed, uint32_t row0, uint32_t sub, float* p_out, uint8_t* s_out) {
    // matrix-core form for SAMPLING half-steps of training batches (DBN encode / decode: its accumulator layout gives every Philox block to one
    // lane); a probabilities-only pass (the free-energy gradient's hidden activations) stays on the vector kernel, whose stores are
    // coalesced -- measured at [32768, 88 -> 256]: 0.11 ms vector vs 0.19 ms matrix-core per call
    if (N >= 2048 && s_out != nullptr && half_mfma_lds_bytes(K, n_out) <= 158 * 1024 && !mnn_switch_set(MNN_SW_RBM_NO_MFMA)) {
        static MnnPerDeviceOnce raised;
        MNN_HIP(mnn_once_per_device(raised, [] {
            const hipError_t e = mnn_raise_dynamic_lds(reinterpret_cast<const void*>(&rbm_half_mfma_kernel<uint8_t>), 160 * 1024);
            return e != hipSuccess ? e : mnn_raise_dynamic_lds(reinterpret_cast<const void*>(&rbm_half_mfma_kernel<float>), 160 * 1024);
        }));
        const size_t l2 = half_mfma_lds_bytes(K, n_out);
        const int grid = min(cdiv(N, GM_ROWS), max(mnn_cu_count(), 1));        // one workgroup per CU walks the row tiles
        if (in_dtype == MNN_U8)
            hipLaunchKernelGGL(rbm_half_mfma_kernel<uint8_t>, dim3(grid), dim3(512), l2, st, N, K, n_out, (const uint8_t*)in, Wk, ldw, b, ld_b,
                               stream_id, seed, row0, sub, p_out, s_out);
        else
            hipLaunchKernelGGL(rbm_half_mfma_kernel<float>, dim3(grid), dim3(512), l2, st, N, K, n_out, (const float*)in, Wk, ldw, b, ld_b,
                               stream_id, seed, row0, sub, p_out, s_out);
        MNN_LAUNCH_CHECK();
        return MNN_OK;
    }
    const size_t lds = (size_t)RBM_R * ((K + 3) & ~3) * sizeof(float);
    if (in_dtype == MNN_U8)
        hipLaunchKernelGGL(rbm_half_kernel<uint8_t>, dim3(cdiv(N, RBM_R)), dim3(256), lds, st, N, K, n_out, (const uint8_t*)in, Wk, ldw, b, ld_b,
                           stream_id, seed, row0, sub, p_out, s_out);
    else
        hipLaunchKernelGGL(rbm_half_kernel<float>, dim3(cdiv(N, RBM_R)), dim3(256), lds, st, N, K, n_out, (const float*)in, Wk, ldw, b, ld_b,
                           stream_id, seed, row0, sub, p_out, s_out);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

extern "C" int mnn_rbm_hidden(mnn_stream_t s, int N, int D, int Hn, const void* v, int v_dtype, const float* W, const float* bh, int ld_bh,
                              int stream_id, uint64_t seed, uint32_t row0, uint32_t sub, float* p_h, uint8_t* h) {
    MNN_REQUIRE(N > 0 && D > 0 && Hn > 0 && v && W && bh && (p_h || h), "mnn_rbm_hidden: bad arguments");
    MNN_REQUIRE(v_dtype == MNN_U8 || v_dtype == MNN_F32, "mnn_rbm_hidden: v dtype must be u8/f32");
    MNN_REQUIRE(ld_bh == 0 || ld_bh >= Hn, "mnn_rbm_hidden: bad ld_bh");
    return launch_half((hipStream_t)s, N, D, Hn, v, v_dtype, W, Hn, bh, ld_bh, stream_id, seed, row0, sub, p_h, h);
}

extern "C" int mnn_rbm_visible(mnn_stream_t s, int N, int D, int Hn, const void* h, int h_dtype, const float* W, const float* bv, int ld_bv,
                               int stream_id, uint64_t seed, uint32_t row0, uint32_t sub, float* p_v, uint8_t* v, void* workspace) {
    MNN_REQUIRE(N > 0 && D > 0 && Hn > 0 && h && W && bv && workspace && (p_v || v), "mnn_rbm_visible: bad arguments");
    MNN_REQUIRE(h_dtype == MNN_U8 || h_dtype == MNN_F32, "mnn_rbm_visible: h dtype must be u8/f32");
    MNN_REQUIRE(ld_bv == 0 || ld_bv >= D, "mnn_rbm_visible: bad ld_bv");
    int rc = mnn_transpose(s, W, MNN_F32, D, Hn, Hn, workspace, MNN_F32, D);
    if (rc != MNN_OK) return rc;
    return launch_half((hipStream_t)s, N, Hn, D, h, h_dtype, (const float*)workspace, D, bv, ld_bv, stream_id, seed, row0, sub, p_v, v);
}

// ----------------------------------------------------------------------------------------------
// free energy, per row (rbm.py:256-258; R4):  F[n] = -sum_j softplus((vW)_j + bh[n,j]) - v.bv[n]
// ----------------------------------------------------------------------------------------------

// (a one-job call of the grouped launch: one kernel, rbm_free_energy_multi_kernel, serves both)
extern "C" int mnn_rbm_free_energy(mnn_stream_t s, int N, int D, int Hn, const uint8_t* v, const float* W, const float* bh, int ld_bh,
                                   const float* bv, int ld_bv, float* F, float* p_h) {
    const mnn_rbm_free_energy_job job{v, W, bh, bv, F, p_h};
    return mnn_rbm_free_energy_multi(s, 1, &job, N, D, Hn, ld_bh, ld_bv);
}

// ----------------------------------------------------------------------------------------------
// CD-k bias deltas (rbm.py:318-327):  dbv[d] += scale * sum_n (v[n,d] - p_v[n,d]),  dbh[j] += scale * sum_n (h[n,j] - p_h[n,j]).
// One pass over the four [N, .] arrays; a workgroup owns 64 columns of one of the two outputs and a slab of rows, threads of a
// wave read consecutive columns (coalesced), the 4 waves split the slab's rows; one f32 atomic per column and workgroup.
// ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rbm_cd_bias_delta_kernel(int N, int D, int Hn, const uint8_t* __restrict__ v, const float* __restrict__ p_v, const uint8_t* __restrict__ h,
                         const float* __restrict__ p_h, float scale, float* __restrict__ dbv, float* __restrict__ dbh) {
    __shared__ float part[4][64];
    const int nbv = (D + 63) / 64;
    const bool vis = (int)blockIdx.x < nbv;
    const int cols = vis ? D : Hn;
    const int c = (vis ? blockIdx.x : blockIdx.x - nbv) * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
    const uint8_t* s = vis ? v : h;
    const float* p = vis ? p_v : p_h;
    float acc = 0.f;
    if (c < cols)
        for (int r = blockIdx.y * 4 + w; r < N; r += gridDim.y * 4) acc += (float)s[(size_t)r * cols + c] - p[(size_t)r * cols + c];
    part[w][threadIdx.x & 63] = acc;
    __syncthreads();
    if (w == 0 && c < cols) atomicAdd((vis ? dbv : dbh) + c, scale * (part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]));
}

extern "C" int mnn_rbm_cd_bias_delta(mnn_stream_t s, int N, int D, int Hn, const uint8_t* v, const float* p_v, const uint8_t* h, const float* p_h,
                                     float scale, float* dbv, float* dbh) {
    MNN_REQUIRE(N > 0 && D > 0 && Hn > 0 && v && p_v && h && p_h && dbv && dbh, "mnn_rbm_cd_bias_delta: bad arguments");
    const int slabs = N >= 4096 ? 64 : (N >= 256 ? 8 : 1);
    hipLaunchKernelGGL(rbm_cd_bias_delta_kernel, dim3((D + 63) / 64 + (Hn + 63) / 64, slabs), dim3(256), 0, (hipStream_t)s, N, D, Hn, v, p_v, h, p_h,
                       scale, dbv, dbh);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

// out[i] = a * x[i] + b * y[i]  (f32; out may alias x or y; y may be NULL when b == 0): the `assign_add` of the CD deltas
// (rbm.py:329-333) and the combination of their positive / negative phase products.
__global__ void __launch_bounds__(256) axpby_kernel(long n, float a, const float* x, float b, const float* y, float* out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = a * x[i] + (y ? b * y[i] : 0.f);
}
extern "C" int mnn_axpby_f32(mnn_stream_t s, long n, float a, const float* x, float b, const float* y, float* out) {
    MNN_REQUIRE(n > 0 && x && out && (y || b == 0.f), "mnn_axpby_f32: bad arguments");
    hipLaunchKernelGGL(axpby_kernel, dim3((int)min(1024L, (n + 255) / 256)), dim3(256), 0, (hipStream_t)s, n, a, x, b, y, out);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

// rbm.py:286-297: bv[d] = log(1e-6 + p/(1-p)) with p = colsum[d] / count (utils/auxiliary.py:9-11 safe_log); colsum comes from
// mnn_bias_grad over the f32 batch (summed over ranks by the caller under data parallelism).
__global__ void __launch_bounds__(256) rbm_visible_bias_init_kernel(int D, const float* __restrict__ colsum, float count, float* __restrict__ bv) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d < D) {
        const float p = colsum[d] / count;
        bv[d] = logf(1e-6f + p / (1.f - p));
    }
}
extern "C" int mnn_rbm_visible_bias_init(mnn_stream_t s, int D, const float* colsum, float count, float* bv) {
    MNN_REQUIRE(D > 0 && colsum && bv && count > 0.f, "mnn_rbm_visible_bias_init: bad arguments");
    hipLaunchKernelGGL(rbm_visible_bias_init_kernel, dim3(cdiv(D, 256)), dim3(256), 0, (hipStream_t)s, D, colsum, count, bv);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

// Rows of the LSTM-RBM cost gradient (rnn_rbm.py:113-126 through rbm.py:229: cost = F(v) - F(v_s), v_s constant):
//   d cost / d bh_t = w (sigmoid(z(v_s)) - sigmoid(z(v))),   d cost / d bv_t = w (v_s - v),   w = row_weight * scale
// written into the Dense-output-shaped block d_out [N, ld] (columns [Hn + D, ld) zeroed), together with the two scaled hidden blocks whose
// products with v_s^T and v^T give d cost / d W = v_s^T (w ss) - v^T (w sv):  pos = w ss,  neg = -w sv  (so that both GEMMs ACCUMULATE).
__global__ void __launch_bounds__(256) rbm_cd_rows_kernel(int N, int D, int Hn, int ld, const uint8_t* __restrict__ v, const uint8_t* __restrict__ vs,
                                                          const float* __restrict__ sv, const float* __restrict__ ss, const float* __restrict__ rw,
                                                          float scale, float* __restrict__ d_out, float* __restrict__ pos, float* __restrict__ neg) {
    const int n = blockIdx.x;
    const float w = rw[n] * scale;
    for (int j = threadIdx.x; j < ld; j += 256) {
        float o = 0.f;
        if (j < Hn) {
            const float a = ss[(size_t)n * Hn + j], b = sv[(size_t)n * Hn + j];
            o = w * (a - b);
            pos[(size_t)n * Hn + j] = w * a;
            neg[(size_t)n * Hn + j] = -(w * b);
        } else if (j < Hn + D) {
            const int i = j - Hn;
            o = w * ((float)vs[(size_t)n * D + i] - (float)v[(size_t)n * D + i]);
        }
        d_out[(size_t)n * ld + j] = o;
    }
}
extern "C" int mnn_rbm_cd_rows(mnn_stream_t s, int N, int D, int Hn, int ld, const uint8_t* v, const uint8_t* v_s, const float* sv, const float* ss,
                               const float* row_weight, float scale, float* d_out, float* pos, float* neg) {
    MNN_REQUIRE(N > 0 && D > 0 && Hn > 0 && ld >= Hn + D && v && v_s && sv && ss && row_weight && d_out && pos && neg, "mnn_rbm_cd_rows: bad arguments");
    hipLaunchKernelGGL(rbm_cd_rows_kernel, dim3(N), dim3(256), 0, (hipStream_t)s, N, D, Hn, ld, v, v_s, sv, ss, row_weight, scale, d_out, pos, neg);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

// dz[i] = dy[i] * y[i] * (1 - y[i])  (f32; dz may alias dy): backward of y = sigmoid(z), the activation of the Dense feedback module
// (dnn.py:60-76 / multinn_feedback.py:48-52)
__global__ void __launch_bounds__(256) sigmoid_grad_kernel(long n, const float* __restrict__ dy, const float* __restrict__ y, float* dz) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float yy = y[i];
        dz[i] = dy[i] * (yy * (1.f - yy));       // (not yy - yy * yy: the rounding of yy * yy is amplified by yy / (1 - yy) in the difference)
    }
}
extern "C" int mnn_sigmoid_grad_f32(mnn_stream_t s, long n, const float* dy, const float* y, float* dz) {
    MNN_REQUIRE(n > 0 && dy && y && dz, "mnn_sigmoid_grad_f32: bad arguments");
    hipLaunchKernelGGL(sigmoid_grad_kernel, dim3((int)min(2048L, (n + 255) / 256)), dim3(256), 0, (hipStream_t)s, n, dy, y, dz);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}
