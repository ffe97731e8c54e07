// Conditional generation for a partly given NADE by sampling-importance-resampling (DESIGN.md section 4 "NADE importance resampling";
// include/multinn_hip.h: mnn_nade_sample_sir_at).  A SCAN is one (row, track, generated step).  G: its given cells, F the free ones.  The
// clamped ancestral scan of nade_sample_kernel<., ., ., GIVEN> (nade.hip) draws x_F from a proposal q whose weight is
// w = prod_{i in G} p(x_i = g_i | v_<i); C such scans with one of them picked with probability w_c / sum w is an approximate draw from
// p(x_F | x_G, past) that becomes exact as C grows.
//   particles = C: 2 <= C <= 1024 (C <= 1, no mnn_sir or no codes: mnn_nade_sample_temps_at, launch for launch).
//   PARTICLE 0 is the scan the call without particles runs: stream MNN_STREAM_NADE, row row0 + n, sub-counter sub + *sub_base, element
//     e = m D + i, the same clamp, the same bits.
//   PARTICLE c >= 1 is the same clamped scan on stream MNN_STREAM_NADE_SIR at the same row and sub-counter and element (c - 1) E4 + e,
//     E4 = tracks D rounded up to a multiple of 4 (the layout of the redraw attempts on stream 10): a particle's draws depend on its own counters
//     only -- not on C, the rows launched with it or the chunking of a session -- and a larger C extends a smaller C's particle set.
//   WEIGHT: log w_c = sum_{i in G} log(1e-6 + q_i), q_i the conditional of the emitted (given) value AT THE SCAN'S TEMPERATURE, the number the
//     tempered draw compares its uniform against (the target is the tempered step distribution restricted to x_G); at temperature 1 this is
//     mnn_nade_given_is's weight term for term: lane l adds visibles l, l + 64, ... in order, the xor butterfly adds the lanes.
//   PICK: one uniform u on stream MNN_STREAM_NADE_SIR_PICK at (row, sub-counter, element = track).  In float64: e_c = exp(log w_c - max_c log w_c),
//     a running sum over c = 0 .. C - 1 IN THAT ORDER (one lane adds them), total = the last running sum; the pick is the smallest c whose
//     running sum exceeds u total, C - 1 if none does.  ESS = total^2 / sum_c e_c^2 (the same serial order).
//   SHORT CUT, decided per scan on the device from the staged codes (wave-uniform): no given cell ordered behind a free one -- nothing given,
//     everything given, a given prefix -- means equal weights whatever is drawn: the scan runs particle 0 alone and emits it, ESS = C, pick = 0,
//     log_w (where asked for) = particle 0's, C times.
//   OUTPUTS: the picked particle's vector through the sample strides of mnn_nade_sample, nll = the model's own NLL of it (untempered, summed in
//     visible order like nade_sample_kernel's), ess and pick per scan [tracks, N].
//
// Shape of the work, as nade_is_kernel: one wave per particle, the four waves of a workgroup take particles of the SAME scan -- its b_dec,
// codes and temperatures are staged in LDS once -- and a workgroup strides over the scan's particle groups.  The particle's scan and the given
// cells' weight pass are nade_particle.h's; behind them the particle's vector leaves for the workspace and all cells' log terms (the model's
// own) are formed 64 at a time and summed in visible order.
// Between the two launches a scan's particles live in the workspace: log w f32 [tracks, N, C] | nll f32 [tracks, N, C] | short-cut flag u8
// [tracks, N] | vectors u8 [tracks, N, C, D] (mnn_nade_sample_sir_workspace_bytes).  The second launch, one wave per scan, picks and copies.
#include "common.h"
#include "nade_particle.h"

#define SIR_MAX_C 1024

struct SirArgs {
    int tracks, N, D, Hn, C, G;                              // G: workgroups per scan
    const float* bias; int ld_bias;
    const float* w_enc; const float* w_dec;
    const uint8_t* given; long s_track_stride; long s_row_stride; int s_elem_stride;      // the codes, with the strides of the samples
    uint64_t seed; uint32_t row0, sub; const uint32_t* sub_base;
    uint32_t eq;                                             // Philox blocks per particle on MNN_STREAM_NADE_SIR: E4 / 4
    SampleTemps TT;                                          // by_visible == 0: track m draws at t[m] (a scalar: eight times)
    float* log_w; float* nll_c; uint8_t* flag; uint8_t* v;   // the workspace (log_w: or the caller's)
};

static size_t sir_lds_bytes(int D) { return 64 + (size_t)5 * nade_dq(D) + 4 * nade_wave_lds_bytes(D); }      // <= 42560 (D <= 1536)

// FULL: Hn == 256, no lane is idle.  TEMP: some temperature of the launch is not 1 (the table; without it the scan is nade_is_kernel's)
template <bool FULL, bool TEMP>
__global__ void __launch_bounds__(256) nade_sir_kernel(SirArgs A) {
    // workgroup: temperatures [8] f32 (+ pad to 64 B) | b_dec [Dq] f32 | codes [Dq] u8; then the four waves' parts (NadeWaveLds; the logits
    // make room for the log terms)
    extern __shared__ __attribute__((aligned(16))) unsigned char nade_sir_smem[];
    const int D = A.D, Hn = A.Hn, C = A.C;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.x / A.G, slot = blockIdx.x - n * A.G;       // n < N by the grid
    const int m = blockIdx.y;
    const int Dq = nade_dq(D);
    float* stt = reinterpret_cast<float*>(nade_sir_smem);
    float* sbd = reinterpret_cast<float*>(nade_sir_smem + 64);
    unsigned char* sg = nade_sir_smem + 64 + (size_t)4 * Dq;
    const NadeWaveLds W = nade_wave_lds(nade_sir_smem + 64 + (size_t)5 * Dq, wv, D);
    const float* __restrict__ bias = A.bias + (size_t)n * A.ld_bias;
    {   // the scan's b_dec, codes and temperatures: one pass of the workgroup, a broadcast read per visible afterwards
        const float* __restrict__ bd = bias + A.tracks * Hn + m * D;
        const uint8_t* __restrict__ gv = A.given + (size_t)m * A.s_track_stride + (size_t)n * A.s_row_stride;
        for (int i = threadIdx.x; i < D; i += 256) {
            sbd[i] = bd[i];
            sg[i] = gv[(size_t)i * A.s_elem_stride];
        }
        if (TEMP) sample_temps_park(A.TT, (int)threadIdx.x, stt);
    }
    __syncthreads();                                         // the only barrier: every wave reaches it, the particle loop below has none
    // the short cut: no given cell behind a free one (first free visible > last given visible), from the staged codes -- wave-uniform
    int last = -1, first = D;
    for (int i = D - 1 - lane; i >= 0; i -= 64) first = sg[i] == NADE_FREE ? i : first;
    for (int i = lane; i < D; i += 64) last = sg[i] != NADE_FREE ? i : last;
    for (int o = 32; o > 0; o >>= 1) {
        last = max(last, __shfl_xor(last, o));
        first = min(first, __shfl_xor(first, o));
    }
    const bool shortcut = last < first;
    const NadeLane L = nade_lane_setup<FULL>(bias, m * Hn, Hn, lane);
    const uint32_t rid = A.row0 + (uint32_t)n;
    uint32_t sub = A.sub;
    if (A.sub_base != nullptr) sub += *A.sub_base;           // one wave-uniform read, behind the loads above (nade_sample_kernel)
    // a per-track table has n == tracks <= MNN_TEMPS_MAX entries; a scalar fills all of them, and is entry 0 for the tracks past the table
    const int tix = A.TT.by_visible || m >= MNN_TEMPS_MAX ? 0 : m;
    const int tn = A.TT.by_visible ? A.TT.n : 0;
    NadeParticle P;
    P.D = D, P.Hn = Hn, P.Ds = D;
    P.we = A.w_enc + (size_t)m * D * Hn, P.wd = A.w_dec + (size_t)m * D * Hn;
    P.sbd = sbd, P.codes = sg, P.held = false;
    P.seed = A.seed, P.row = rid, P.sub = sub;
    P.e0 = (uint32_t)m * (uint32_t)D;
    P.stt = stt, P.tix = tix, P.tn = tn;
    for (int c = slot * 4 + wv; c < C; c += 4 * A.G) {       // wave-uniform
        if (shortcut && c > 0) break;                        // equal weights: particle 0 is the scan's vector
        P.stream = c == 0 ? MNN_STREAM_NADE : MNN_STREAM_NADE_SIR;
        P.block0 = c == 0 ? 0u : (uint32_t)(c - 1) * A.eq;
        nade_particle_scan<FULL, TEMP>(P, L, W, lane);
        // behind the scan: the vector out; the log terms 64 at a time -- the given cells' (at the scan's temperature) summed per lane in visible
        // order and across the lanes by the butterfly (the order of nade_given_log_weight, in this pass: no cell's term is formed twice), all
        // cells' (the model's own) left in LDS for the sum in visible order
        const size_t pc = ((size_t)m * A.N + n) * C + c;
        float part = 0.f;
        for (int i = lane; i < D; i += 64) {
            const float l = W.sp[i];
            const bool on = W.son[i] != 0;
            A.v[pc * D + i] = on ? 1 : 0;
            const float term = nade_log_term(l, on);
            if (sg[i] != NADE_FREE) part += TEMP ? nade_log_term(l / stt[tn != 0 ? i % tn : tix], on) : term;     // (tn != 0: tix == 0)
            W.sp[i] = term;
        }
        const float lw = wave_xor_sum(part);
        float logp = 0.f;                                    // (LDS operations of one wave execute in order)
        for (int i = 0; i < D; ++i) logp += W.sp[i];
        if (lane == 0) {
            A.log_w[pc] = lw;
            A.nll_c[pc] = -logp;
            if (c == 0) A.flag[(size_t)m * A.N + n] = shortcut ? 1 : 0;
        }
    }
}

struct SirPickArgs {
    int tracks, N, D, C;
    uint64_t seed; uint32_t row0, sub; const uint32_t* sub_base;
    float* log_w; const float* nll_c; const uint8_t* flag; const uint8_t* v;
    uint8_t* samples; long s_track_stride; long s_row_stride; int s_elem_stride;
    float* nll; float* ess; int32_t* pick;                   // [tracks, N]; nll may be NULL
};

// One wave per scan.  The lanes form e_c = exp(log w_c - max) in double; lane 0 adds them in the order c = 0 .. C - 1 (the documented order of
// the pick) and finds the pick; the lanes copy the picked vector out.
__global__ void __launch_bounds__(64) nade_sir_pick_kernel(SirPickArgs A) {
    __shared__ double se[SIR_MAX_C];
    __shared__ int spick;
    const int n = blockIdx.x, m = blockIdx.y, lane = threadIdx.x, C = A.C;
    const size_t r = (size_t)m * A.N + n;
    float* lw = A.log_w + r * C;
    int pick = 0;
    float ess = (float)C;
    if (A.flag[r] != 0) {                                    // the short cut: particle 0, equal weights
        const float w0 = lw[0];
        for (int c = 1 + lane; c < C; c += 64) lw[c] = w0;
    } else {
        double mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmax(mx, (double)lw[c]);
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
        for (int c = lane; c < C; c += 64) se[c] = exp((double)lw[c] - mx);
        __syncthreads();
        if (lane == 0) {
            uint32_t sub = A.sub;
            if (A.sub_base != nullptr) sub += *A.sub_base;
            float u4[4];
            philox_uniform4(A.seed, MNN_STREAM_NADE_SIR_PICK, A.row0 + (uint32_t)n, sub, (uint32_t)m >> 2, u4);
            const int w = m & 3;
            const double u = (double)(w == 0 ? u4[0] : w == 1 ? u4[1] : w == 2 ? u4[2] : u4[3]);
            double run = 0.0, sq = 0.0;
            for (int c = 0; c < C; ++c) {
                const double e = se[c];
                run += e;
                sq += e * e;
                se[c] = run;
            }
            const double thr = u * run;
            int p = C - 1;
            for (int c = 0; c < C; ++c)
                if (se[c] > thr) { p = c; break; }
            spick = p;
            A.ess[r] = (float)(run * run / sq);
            A.pick[r] = p;
        }
        __syncthreads();
        pick = spick;
    }
    if (A.flag[r] != 0 && lane == 0) {
        A.ess[r] = ess;
        A.pick[r] = 0;
    }
    const uint8_t* __restrict__ v = A.v + (r * C + pick) * A.D;
    uint8_t* __restrict__ out = A.samples + (size_t)m * A.s_track_stride + (size_t)n * A.s_row_stride;
    for (int i = lane; i < A.D; i += 64) out[(size_t)i * A.s_elem_stride] = v[i];
    if (A.nll != nullptr && lane == 0) A.nll[r] = A.nll_c[r * C + pick];
}

// no codes: every scan is the short cut and the launch is mnn_nade_sample_temps_at's; its statistics are constants
__global__ void __launch_bounds__(256) nade_sir_const_kernel(long count, float C, float* __restrict__ ess, int32_t* __restrict__ pick) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) {
        if (ess != nullptr) ess[i] = C;
        if (pick != nullptr) pick[i] = 0;
    }
}

extern "C" size_t mnn_nade_sample_sir_workspace_bytes(int tracks, int N, int D, int particles) {
    if (tracks <= 0 || N <= 0 || D <= 0 || particles <= 1) return 0;
    const size_t scans = (size_t)tracks * (size_t)N;
    return 2 * nade_align256(scans * (size_t)particles * sizeof(float)) + nade_align256(scans) + nade_align256(scans * (size_t)particles * (size_t)D);
}

extern "C" int mnn_nade_sample_sir_at(mnn_stream_t s, int tracks, int N, int D, int Hn, const float* bias, int ld_bias, const float* w_enc,
                                      const float* w_dec, const mnn_temps* temps, uint64_t seed, uint32_t row0, uint32_t sub, uint8_t* samples,
                                      long s_track_stride, int s_row_stride, int s_elem_stride, float* nll, const uint8_t* given,
                                      const uint32_t* sub_base, const mnn_sir* sir, float* log_w) {
    if (sir == nullptr || sir->particles <= 1)
        return mnn_nade_sample_temps_at(s, tracks, N, D, Hn, bias, ld_bias, w_enc, w_dec, temps, seed, row0, sub, samples, s_track_stride, s_row_stride,
                                        s_elem_stride, nll, given, sub_base);
    const int C = sir->particles;
    MNN_REQUIRE(C <= SIR_MAX_C, "mnn_nade_sample_sir: particles=%d > %d", C, SIR_MAX_C);
    MNN_REQUIRE(temps != nullptr && temps->n > 0, "mnn_nade_sample_sir: particles need a temperature (threshold decoding draws nothing)");
    int G;                                                   // (the grid bound is checked here, ahead of the hand-off of a call without codes below)
    if (const int rc = nade_particle_check("mnn_nade_sample_sir", "scan", tracks, N, D, Hn, ld_bias, C, &G)) return rc;
    MNN_REQUIRE(bias && w_enc && w_dec && samples && sir->ess && sir->pick, "mnn_nade_sample_sir: null pointer");
    MNN_REQUIRE(temps->n <= MNN_TEMPS_MAX && (temps->n == 1 || temps->by_visible != 0 || temps->n == tracks),
                "mnn_nade_sample_sir: temps: 1..%d positive finite temperatures, per track one or `tracks` of them", MNN_TEMPS_MAX);
    for (int e = 0; e < temps->n; ++e)
        MNN_REQUIRE(temps->t[e] > 0.f && temps->t[e] <= 3.0e38f, "mnn_nade_sample_sir: temps: entry %d is not a positive finite temperature", e);
    const long E4 = ((long)tracks * D + 3) / 4 * 4;
    MNN_REQUIRE(E4 * (long)(C - 1) < (1L << 32), "mnn_nade_sample_sir: the particles' elements pass 2^32");
    hipStream_t st = (hipStream_t)s;
    if (given == nullptr) {                                  // nothing to condition on: the call without particles, and its constant statistics
        const int rc = mnn_nade_sample_temps_at(s, tracks, N, D, Hn, bias, ld_bias, w_enc, w_dec, temps, seed, row0, sub, samples, s_track_stride,
                                                s_row_stride, s_elem_stride, nll, given, sub_base);
        if (rc != MNN_OK) return rc;
        const long count = (long)tracks * N;
        hipLaunchKernelGGL(nade_sir_const_kernel, dim3(cdiv(count, 256)), dim3(256), 0, st, count, (float)C, sir->ess, sir->pick);
        MNN_LAUNCH_CHECK();
        return MNN_OK;
    }
    const size_t need = mnn_nade_sample_sir_workspace_bytes(tracks, N, D, C);
    MNN_REQUIRE(sir->workspace && sir->workspace_bytes >= need && ((uintptr_t)sir->workspace & 255) == 0,
                "mnn_nade_sample_sir: workspace of mnn_nade_sample_sir_workspace_bytes() = %zu bytes, 256-byte aligned", need);
    const size_t scans = (size_t)tracks * (size_t)N;
    char* wp = static_cast<char*>(sir->workspace);
    float* lw = log_w != nullptr ? log_w : reinterpret_cast<float*>(wp);
    wp += nade_align256(scans * C * sizeof(float));
    float* nll_c = reinterpret_cast<float*>(wp);
    wp += nade_align256(scans * C * sizeof(float));
    uint8_t* flag = reinterpret_cast<uint8_t*>(wp);
    wp += nade_align256(scans);
    uint8_t* v = reinterpret_cast<uint8_t*>(wp);
    SampleTemps TT;
    memset(&TT, 0, sizeof(TT));
    bool tempered = false;
    if (temps->by_visible && temps->n > 1) {
        TT.n = temps->n; TT.by_visible = 1;
        for (int e = 0; e < temps->n; ++e) TT.t[e] = temps->t[e];
        for (int e = 0; e < temps->n && e < D; ++e) tempered = tempered || temps->t[e] != 1.0f;
    } else {
        TT.n = MNN_TEMPS_MAX; TT.by_visible = 0;
        for (int j = 0; j < MNN_TEMPS_MAX; ++j) TT.t[j] = temps->n == 1 ? temps->t[0] : (j < temps->n ? temps->t[j] : 1.0f);
        for (int j = 0; j < tracks && j < MNN_TEMPS_MAX; ++j) tempered = tempered || TT.t[j] != 1.0f;
    }
    SirArgs a{tracks, N, D, Hn, C, G, bias, ld_bias, w_enc, w_dec, given, s_track_stride, (long)s_row_stride, s_elem_stride, seed, row0, sub, sub_base,
              (uint32_t)(E4 >> 2), TT, lw, nll_c, flag, v};
    const dim3 grid((unsigned)((long)N * G), (unsigned)tracks);
    const size_t lds = sir_lds_bytes(D);
    if (Hn == 256) { if (tempered) hipLaunchKernelGGL((nade_sir_kernel<true, true>), grid, dim3(256), lds, st, a); else hipLaunchKernelGGL((nade_sir_kernel<true, false>), grid, dim3(256), lds, st, a); }
    else { if (tempered) hipLaunchKernelGGL((nade_sir_kernel<false, true>), grid, dim3(256), lds, st, a); else hipLaunchKernelGGL((nade_sir_kernel<false, false>), grid, dim3(256), lds, st, a); }
    MNN_LAUNCH_CHECK();
    SirPickArgs p{tracks, N, D, C, seed, row0, sub, sub_base, lw, nll_c, flag, v, samples, s_track_stride, (long)s_row_stride, s_elem_stride, nll, sir->ess, sir->pick};
    hipLaunchKernelGGL(nade_sir_pick_kernel, dim3((unsigned)N, (unsigned)tracks), dim3(64), 0, st, p);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}
