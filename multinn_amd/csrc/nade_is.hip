// Importance-sampling estimate of log p(x_G) for a partly given NADE row (DESIGN.md section 4 "NADE importance estimator";
// include/multinn_hip.h: mnn_nade_given_is).  G: the given cells of a row, F the free ones.  The clamped ancestral scan -- the free cells drawn in
// visible order with the given cells held -- is a proposal q(x_F) whose weight w = prod_{i in G} p(x_i = g_i | v_<i) has E_q[w] = p(x_G).
// A PARTICLE is one such scan of one (row, track): the scan of nade_sample_kernel<1, FULL, SPEC, GIVEN> (nade.hip), the same dot product, xor
// butterfly and draw, so oracle/det.py: nade_sample on clamped uniforms reproduces every particle bit for bit.
//
// Shape of the work.  One wave per particle (a lane owns four hidden units), and the four waves of a workgroup take particles of the SAME row:
// the row's b_dec, its codes and its data cells are staged in LDS once per workgroup, b_enc and h(b_enc) are kept in registers across a
// wave's particles.  A workgroup strides over its row's particle groups (c = 4 slot + wave, + 4 G, ...), so any C runs the one code path.
// Off the serial chain: a particle's logits are parked in LDS as in the sampling kernel; behind the scan the given cells' log terms are formed
// 64 at a time, summed per lane in visible order and across the lanes by the xor butterfly -- a fixed order.  The scan stops behind the row's
// last given visible unless the samples are asked for (nothing behind it enters w, and nothing before it depends on it).
// A second small launch reduces a row's C log weights in double, in a fixed order: log_pg, the effective sample size and the standard error.
#include "common.h"
#include "nade_scan.h"

#define IS_FREE 255

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

static size_t is_lds_bytes(int D) { return (size_t)26 * ((D + 15) & ~15) + 4096; }     // <= 44032 (D <= 1536)

// FULL: Hn == 256, no lane is idle (as nade_sample_kernel)
template <bool FULL>
__global__ void __launch_bounds__(256) nade_is_kernel(IsArgs A) {
    // workgroup: b_dec [Dq] f32 | codes [Dq] u8 | codes with the free cells at the data [Dq] u8; then per wave: logits [Dq] f32 | 256 uniforms |
    // draws [Dq] u8.  Dq = D rounded up to 16: every carve offset is a multiple of 16 bytes.
    extern __shared__ __attribute__((aligned(16))) unsigned char nade_is_smem[];
    const int D = A.D, Hn = A.Hn, C = A.C;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.x / A.G, slot = blockIdx.x - n * A.G;       // n < N by the grid
    const int m = blockIdx.y;
    const int Dq = (D + 15) & ~15;
    float* sbd = reinterpret_cast<float*>(nade_is_smem);
    unsigned char* sg = nade_is_smem + (size_t)4 * Dq;
    unsigned char* sgd = sg + Dq;
    unsigned char* wbase = nade_is_smem + (size_t)6 * Dq + (size_t)wv * ((size_t)5 * Dq + 1024);
    float* sp = reinterpret_cast<float*>(wbase);
    float* su = reinterpret_cast<float*>(wbase + (size_t)4 * Dq);
    unsigned char* son = wbase + (size_t)4 * Dq + 1024;
    const float* __restrict__ bias = A.bias + (size_t)n * A.ld_bias;
    const float* __restrict__ we = A.w_enc + (size_t)m * D * Hn;
    const float* __restrict__ wd = A.w_dec + (size_t)m * D * Hn;
    {   // the row's b_dec, codes and data cells: one coalesced pass of the workgroup, a broadcast read per visible afterwards
        const float* __restrict__ bd = bias + A.tracks * Hn + m * D;
        const uint8_t* __restrict__ gv = A.given + (size_t)m * A.g_track_stride + (size_t)n * D;
        const uint8_t* __restrict__ dt = A.data != nullptr ? A.data + (size_t)m * A.d_track_stride + (size_t)n * D : nullptr;
        for (int i = threadIdx.x; i < D; i += 256) {
            sbd[i] = bd[i];
            const uint8_t g = gv[i];
            sg[i] = g;
            sgd[i] = (g == IS_FREE && dt != nullptr) ? (uint8_t)(dt[i] != 0) : g;
        }
    }
    __syncthreads();                                         // the only barrier: every wave reaches it, the particle loop below has none
    int last = -1;                                           // the row's last given visible
    for (int i = lane; i < D; i += 64) last = sg[i] != IS_FREE ? i : last;
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o));
    const int Ds = A.v_out != nullptr ? D : last + 1;        // visibles to scan (wave-uniform)
    float a0[4], h0[4];
    bool in[4];
    int off[4];                                              // hidden index of (lane, q), 0 where there is none: loads are never predicated
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        in[q] = FULL || lane + 64 * q < Hn;
        off[q] = in[q] ? lane + 64 * q : 0;
        const float av = bias[m * Hn + off[q]];
        a0[q] = in[q] ? av : 0.f;
        h0[q] = det_sigmoid(a0[q]);
    }
    const uint32_t rid = A.row_ids != nullptr ? A.row_ids[n] : A.row0 + (uint32_t)n;
    const uint32_t stream = A.data != nullptr ? MNN_STREAM_NADE_IS_DATA : MNN_STREAM_NADE_IS;
    const uint32_t e0 = (uint32_t)m * (uint32_t)D;           // element index of visible 0 (RNG contract: elem = m D + i)
    constexpr int RING = 8;                                  // visibles in flight, as nade_sample_kernel
    for (int c = slot * 4 + wv; c < C; c += 4 * A.G) {       // wave-uniform
        const bool own = A.data != nullptr && c == 0;        // the upper side's particle 0: its free cells are the data's, no uniform is consumed
        const unsigned char* sc = own ? sgd : sg;
        float lw = 0.f;
        if (Ds > 0) {
            float a[4], h[4];
            // the hidden indices through an opaque zero: the addresses of the prologue's loads do not depend on the particle, and hoisted out of
            // this loop they are held in registers across it (Hn == 256: 163 -> 138 vector registers; idle lanes: 256 + 5 accumulation
            // registers and one wave per SIMD -> 142 and three; profiles/nade_is.md)
            int zero = 0;
            asm volatile("" : "+v"(zero));
            int offp[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = a0[q];
                h[q] = h0[q];
                offp[q] = off[q] + zero;
            }
            float wdr[RING][4], wer[RING][4];                // ring: the weight rows of visibles i .. i + RING - 1
            auto fetch = [&](int k, int i) {
                const int ii = min(i, D - 1);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    wdr[k][q] = wd[(size_t)ii * Hn + offp[q]];
                    wer[k][q] = we[(size_t)ii * Hn + offp[q]];
                }
            };
#pragma unroll
            for (int k = 0; k < RING; ++k) {
                fetch(k, k);
                __builtin_amdgcn_sched_barrier(0);           // issue order = ring order (the waits count loads)
            }
            uint32_t b0 = e0 >> 2;                           // lane l holds the uniforms of Philox block b0 + l
            auto refill = [&]() {
                if (own) return;                             // wave-uniform
                float u4[4];
                philox_uniform4(A.seed, stream, rid, (uint32_t)c, b0 + (uint32_t)lane, u4);
                *reinterpret_cast<float4*>(su + 4 * lane) = make_float4(u4[0], u4[1], u4[2], u4[3]);
            };
            refill();
            auto dot = [&](int k) {                          // sum_j h_j w_dec[visible of ring slot k][j], the contract's order
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = fmaf(h[q], in[q] ? wdr[k][q] : 0.f, acc);
                return wave_xor_sum(acc);
            };
            auto uniform_of = [&](int i) {                   // fetched one visible ahead, with the rare Philox refill
                const uint32_t e = e0 + (uint32_t)min(i, D - 1);
                if ((e >> 2) >= b0 + 64u) {
                    b0 += 64u;
                    refill();
                }
                return su[e - 4u * b0];
            };
            float u_cur = uniform_of(0);
            float acc = dot(0);
            for (int i0 = 0; i0 < Ds; i0 += RING) {
#pragma unroll
                for (int k = 0; k < RING; ++k) {
                    const int i = i0 + k;
                    if (i < Ds) {                            // uniform
                        // speculation (Hn == 256, as the sampling kernel runs it): a 0 leaves the hidden state, so visible i + 1's dot product is this one
                        const float spec = FULL ? dot((k + 1) % RING) : 0.f;
                        const float l = sbd[i] + acc;
                        const int code = __builtin_amdgcn_readfirstlane((int)sc[i]);     // the same byte in every lane: a uniform branch
                        bool on;
                        if (code != IS_FREE) on = code != 0;  // held: moves a / h like a draw, its uniform is left unused
                        else on = draw_below(u_cur, l);
                        if (on) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                a[q] = a[q] + (in[q] ? wer[k][q] : 0.f);
                                h[q] = det_sigmoid(a[q]);
                            }
                            acc = dot((k + 1) % RING);
                        } else {
                            acc = FULL ? spec : dot((k + 1) % RING);
                        }
                        sp[i] = l;                           // every lane holds the same logit and draw: one merged LDS write each
                        son[i] = on ? 1 : 0;
                        u_cur = uniform_of(i + 1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    fetch(k, i + RING);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // behind the scan: the log terms of the GIVEN cells (the codes, not the data: particle 0's free cells carry no weight), 64 at a time;
            // lane l adds visibles l, l + 64, ... in order, the butterfly adds the lanes
            float part = 0.f;
            for (int i = lane; i < Ds; i += 64) {
                const int code = sg[i];
                if (code != IS_FREE) {
                    const float p = det_sigmoid(sp[i]);
                    part += code != 0 ? logf(NADE_EPS + p) : logf(NADE_EPS + (1.0f - p));
                }
            }
            lw = wave_xor_sum(part);
        }
        const size_t pc = ((size_t)m * A.N + n) * C + c;
        if (lane == 0) A.log_w[pc] = lw;
        if (A.v_out != nullptr)                              // (then Ds == D)
            for (int i = lane; i < D; i += 64) A.v_out[pc * D + i] = son[i];
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

static size_t is_lw_bytes(int tracks, int N, int C) { return ((size_t)tracks * (size_t)N * (size_t)C * sizeof(float) + 255) & ~(size_t)255; }

extern "C" size_t mnn_nade_given_is_workspace_bytes(int tracks, int N, int n_particles) {
    if (tracks <= 0 || N <= 0 || n_particles <= 0) return 0;
    return is_lw_bytes(tracks, N, n_particles);
}

extern "C" int mnn_nade_given_is(mnn_stream_t s, int tracks, int N, int D, int Hn, const float* bias, int ld_bias, const float* w_enc,
                                 const float* w_dec, const uint8_t* given, long g_track_stride, const uint8_t* data, long d_track_stride,
                                 int n_particles, uint64_t seed, uint32_t row0, const uint32_t* row_ids, float* log_pg, float* log_w,
                                 uint8_t* v_out, float* stats, void* workspace) {
    MNN_REQUIRE(tracks > 0 && tracks <= 65535 && N > 0 && D > 0 && Hn > 0 && Hn <= 256,
                "mnn_nade_given_is: need 0<tracks<=65535, N,D>0 and 0<Hn<=256 (tracks=%d N=%d D=%d Hn=%d)", tracks, N, D, Hn);
    MNN_REQUIRE(D <= 1536, "mnn_nade_given_is: D <= 1536 (a row's b_dec and codes and a particle's logits and draws are parked in LDS; D=%d)", D);
    MNN_REQUIRE(n_particles >= 1, "mnn_nade_given_is: n_particles=%d < 1", n_particles);
    MNN_REQUIRE(bias && w_enc && w_dec && given && log_pg && workspace, "mnn_nade_given_is: null pointer");
    MNN_REQUIRE(ld_bias >= tracks * (Hn + D), "mnn_nade_given_is: ld_bias too small");
    MNN_REQUIRE(g_track_stride >= (long)N * D || tracks == 1, "mnn_nade_given_is: g_track_stride=%ld < N D", g_track_stride);
    MNN_REQUIRE(data == nullptr || d_track_stride >= (long)N * D || tracks == 1, "mnn_nade_given_is: d_track_stride=%ld < N D", d_track_stride);
    // workgroups per (row, track): a workgroup's four waves take four particles at a time and stride over the row's groups; rows that fill the
    // device on their own get fewer, longer-lived workgroups (the staging and b_enc are then read once per several groups), in equal shares
    const int groups = cdiv(n_particles, 4);
    const long most = cdiv(65536, (long)N * tracks);
    const int per = cdiv(groups, most < 1 ? 1 : most);
    const int G = cdiv(groups, per);
    MNN_REQUIRE((long)N * G <= 0x7fffffffL && (long)N * tracks <= 0x7fffffffL, "mnn_nade_given_is: N * workgroups per row = %ld exceeds the grid",
                (long)N * G);
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
