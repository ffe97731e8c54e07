// Importance-sampling estimate of log p(x_G) for a partly given NADE row (DESIGN.md section 4 "NADE importance estimator";
// include/multinn_hip.h: mnn_nade_given_is).  G: the given cells of a row, F the free ones.  The clamped ancestral scan -- the free cells drawn in
// visible order with the given cells held -- is a proposal q(x_F) whose weight w = prod_{i in G} p(x_i = g_i | v_<i) has E_q[w] = p(x_G).
// A PARTICLE is one such scan of one (row, track): nade_particle.h has the scan, its bit-for-bit contract and the weight pass behind it.
//
// Shape of the work.  One wave per particle, and the four waves of a workgroup take particles of the SAME row: the row's b_dec, its codes and
// its data cells are staged in LDS once per workgroup.  A workgroup strides over its row's particle groups (c = 4 slot + wave, + 4 G, ...),
// so any C runs the one code path.  The scan stops behind the row's last given visible unless the samples are asked for (nothing behind it
// enters w, and nothing before it depends on it).
// A second small launch reduces a row's C log weights in double, in a fixed order: log_pg, the effective sample size and the standard error.
#include "common.h"
#include "nade_particle.h"

struct IsArgs {
    int tracks, N, D, Hn, C, G;                              // G: workgroups per (row, track)
    const float* bias; int ld_bias;
    const float* w_enc; const float* w_dec;
    const uint8_t* given; long g_track_stride;
    const uint8_t* data; long d_track_stride;                // NULL: the lower side
    uint64_t seed; uint32_t row0; const uint32_t* row_ids;
    float* log_w;                                            // [tracks, N, C]: the caller's, or the workspace
    uint8_t* v_out;                                          // [tracks, N, C, D] or NULL
};

static size_t is_lds_bytes(int D) { return (size_t)6 * nade_dq(D) + 4 * nade_wave_lds_bytes(D); }     // <= 44032 (D <= 1536)

// FULL: Hn == 256, no lane is idle (as nade_sample_kernel)
template <bool FULL>
__global__ void __launch_bounds__(256) nade_is_kernel(IsArgs A) {
    // workgroup: b_dec [Dq] f32 | codes [Dq] u8 | codes with the free cells at the data [Dq] u8; then the four waves' parts (NadeWaveLds)
    extern __shared__ __attribute__((aligned(16))) unsigned char nade_is_smem[];
    const int D = A.D, Hn = A.Hn, C = A.C;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.x / A.G, slot = blockIdx.x - n * A.G;       // n < N by the grid
    const int m = blockIdx.y;
    const int Dq = nade_dq(D);
    float* sbd = reinterpret_cast<float*>(nade_is_smem);
    unsigned char* sg = nade_is_smem + (size_t)4 * Dq;
    unsigned char* sgd = sg + Dq;
    const NadeWaveLds W = nade_wave_lds(nade_is_smem + (size_t)6 * Dq, wv, D);
    const float* __restrict__ bias = A.bias + (size_t)n * A.ld_bias;
    {   // the row's b_dec, codes and data cells: one coalesced pass of the workgroup, a broadcast read per visible afterwards
        const float* __restrict__ bd = bias + A.tracks * Hn + m * D;
        const uint8_t* __restrict__ gv = A.given + (size_t)m * A.g_track_stride + (size_t)n * D;
        const uint8_t* __restrict__ dt = A.data != nullptr ? A.data + (size_t)m * A.d_track_stride + (size_t)n * D : nullptr;
        for (int i = threadIdx.x; i < D; i += 256) {
            sbd[i] = bd[i];
            const uint8_t g = gv[i];
            sg[i] = g;
            sgd[i] = (g == NADE_FREE && dt != nullptr) ? (uint8_t)(dt[i] != 0) : g;
        }
    }
    __syncthreads();                                         // the only barrier: every wave reaches it, the particle loop below has none
    int last = -1;                                           // the row's last given visible
    for (int i = lane; i < D; i += 64) last = sg[i] != NADE_FREE ? i : last;
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o));
    const int Ds = A.v_out != nullptr ? D : last + 1;        // visibles to scan (wave-uniform)
    const NadeLane L = nade_lane_setup<FULL>(bias, m * Hn, Hn, lane);
    const uint32_t rid = A.row_ids != nullptr ? A.row_ids[n] : A.row0 + (uint32_t)n;
    const uint32_t stream = A.data != nullptr ? MNN_STREAM_NADE_IS_DATA : MNN_STREAM_NADE_IS;
    NadeParticle P;
    P.D = D, P.Hn = Hn, P.Ds = Ds;
    P.we = A.w_enc + (size_t)m * D * Hn, P.wd = A.w_dec + (size_t)m * D * Hn;
    P.sbd = sbd;
    P.seed = A.seed, P.stream = stream, P.row = rid, P.block0 = 0u;
    P.e0 = (uint32_t)m * (uint32_t)D;
    P.stt = nullptr, P.tix = 0, P.tn = 0;
    for (int c = slot * 4 + wv; c < C; c += 4 * A.G) {       // wave-uniform
        const bool own = A.data != nullptr && c == 0;        // the upper side's particle 0: its free cells are the data's, no uniform is consumed
        float lw = 0.f;
        if (Ds > 0) {
            P.codes = own ? sgd : sg, P.held = own;
            P.sub = (uint32_t)c;
            nade_particle_scan<FULL, false>(P, L, W, lane);
            lw = nade_given_log_weight(W.sp, sg, Ds, lane);  // the codes, not the data: particle 0's free cells carry no weight
        }
        const size_t pc = ((size_t)m * A.N + n) * C + c;
        if (lane == 0) A.log_w[pc] = lw;
        if (A.v_out != nullptr)                              // (then Ds == D)
            for (int i = lane; i < D; i += 64) A.v_out[pc * D + i] = W.son[i];
    }
}

// One workgroup per (track, row): log_pg = m + log(sum_c exp(lw_c - m)) - log C, m = max_c lw_c, in double; stats = (ESS = (sum w)^2 / sum w^2,
// standard error of log_pg by the delta method on the mean of w = sqrt((C / ESS - 1) / (C - 1)); one particle: inf) -- mnn_rbm_ais's formulas.
// Lane l takes particles l, l + 64, ... in order; the tree over the lanes is fixed.
__global__ void __launch_bounds__(64) nade_is_reduce_kernel(int C, const float* __restrict__ lw, float* __restrict__ log_pg, float* __restrict__ stats) {
    __shared__ double buf[64];
    const size_t r = blockIdx.x;
    const float* x = lw + r * C;
    const int t = threadIdx.x;
    double m = -INFINITY;
    for (int c = t; c < C; c += 64) m = fmax(m, (double)x[c]);
    buf[t] = m;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (t < o) buf[t] = fmax(buf[t], buf[t + o]);
        __syncthreads();
    }
    m = buf[0];
    __syncthreads();
    double a = 0.0, b = 0.0;
    for (int c = t; c < C; c += 64) {
        const double e = exp((double)x[c] - m);
        a += e;
        b += e * e;
    }
    buf[t] = a;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (t < o) buf[t] += buf[t + o];
        __syncthreads();
    }
    a = buf[0];
    __syncthreads();
    buf[t] = b;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (t < o) buf[t] += buf[t + o];
        __syncthreads();
    }
    b = buf[0];
    if (t == 0) {
        log_pg[r] = (float)(m + log(a) - log((double)C));
        if (stats != nullptr) {
            const double ess = a * a / b;
            stats[2 * r] = (float)ess;
            stats[2 * r + 1] = C > 1 ? (float)sqrt(fmax((double)C / ess - 1.0, 0.0) / (double)(C - 1)) : INFINITY;
        }
    }
}

static size_t is_lw_bytes(int tracks, int N, int C) { return nade_align256((size_t)tracks * (size_t)N * (size_t)C * sizeof(float)); }

extern "C" size_t mnn_nade_given_is_workspace_bytes(int tracks, int N, int n_particles) {
    if (tracks <= 0 || N <= 0 || n_particles <= 0) return 0;
    return is_lw_bytes(tracks, N, n_particles);
}

extern "C" int mnn_nade_given_is(mnn_stream_t s, int tracks, int N, int D, int Hn, const float* bias, int ld_bias, const float* w_enc,
                                 const float* w_dec, const uint8_t* given, long g_track_stride, const uint8_t* data, long d_track_stride,
                                 int n_particles, uint64_t seed, uint32_t row0, const uint32_t* row_ids, float* log_pg, float* log_w,
                                 uint8_t* v_out, float* stats, void* workspace) {
    MNN_REQUIRE(n_particles >= 1, "mnn_nade_given_is: n_particles=%d < 1", n_particles);
    int G;
    if (const int rc = nade_particle_check("mnn_nade_given_is", "row", tracks, N, D, Hn, ld_bias, n_particles, &G)) return rc;
    MNN_REQUIRE((long)N * tracks <= 0x7fffffffL, "mnn_nade_given_is: N * workgroups per row = %ld exceeds the grid", (long)N * G);     // (the reduce launch)
    MNN_REQUIRE(bias && w_enc && w_dec && given && log_pg && workspace, "mnn_nade_given_is: null pointer");
    MNN_REQUIRE(g_track_stride >= (long)N * D || tracks == 1, "mnn_nade_given_is: g_track_stride=%ld < N D", g_track_stride);
    MNN_REQUIRE(data == nullptr || d_track_stride >= (long)N * D || tracks == 1, "mnn_nade_given_is: d_track_stride=%ld < N D", d_track_stride);
    hipStream_t st = (hipStream_t)s;
    float* lw = log_w != nullptr ? log_w : reinterpret_cast<float*>(workspace);
    IsArgs a{tracks, N, D, Hn, n_particles, G, bias, ld_bias, w_enc, w_dec, given, g_track_stride, data, d_track_stride, seed, row0, row_ids, lw, v_out};
    const dim3 grid((unsigned)((long)N * G), (unsigned)tracks);
    if (Hn == 256) hipLaunchKernelGGL(nade_is_kernel<true>, grid, dim3(256), is_lds_bytes(D), st, a);
    else hipLaunchKernelGGL(nade_is_kernel<false>, grid, dim3(256), is_lds_bytes(D), st, a);
    MNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(nade_is_reduce_kernel, dim3((unsigned)((long)tracks * N)), dim3(64), 0, st, n_particles, (const float*)lw, log_pg, stats);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}
