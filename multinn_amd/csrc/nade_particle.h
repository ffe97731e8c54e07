// The clamped particle scan of a partly given NADE, and what its launches share on the host.  Users: nade_is.hip (nade_is_kernel: the
// importance estimator, mnn_nade_given_is) and nade_sir.hip (nade_sir_kernel: importance resampling, mnn_nade_sample_sir_at).
//
// A PARTICLE is one clamped ancestral scan of one (row, track): the free cells (code NADE_FREE) drawn in visible order, the given cells held.  It
// is the scan of nade_sample_kernel<., FULL, SPEC, GIVEN> (nade.hip) -- the same dot product, xor butterfly and draw (nade_scan.h) -- so
// oracle/det.py: nade_sample on clamped uniforms reproduces every particle bit for bit.  One wave runs one particle, a lane owns four hidden
// units, and a wave runs several particles of the same (row, track) one after the other: b_enc and h(b_enc) (NadeLane) stay in registers across
// them.  A particle's logits and draws are parked in the wave's LDS (NadeWaveLds); behind the scan the given cells' log terms are formed 64 at
// a time (nade_given_log_weight).  nade_sample_kernel and nade_sample_chunk_kernel keep scan bodies of their own (CAP and REDRAW live in them).
#pragma once
#include "nade_scan.h"

#define NADE_FREE 255                                        // the code of a free cell; 0 / 1: the cell is held at that value

// what a lane keeps across a wave's particles: its four hidden units' b_enc and h(b_enc)
struct NadeLane {
    float a0[4], h0[4];
    bool in[4];
    int off[4];                                              // hidden index of (lane, q), 0 where there is none: loads are never predicated
};
// b_enc of the track: bias[enc ..] of the row (an index, not a pointer: three vector registers less in nade_is_kernel<true>).
// FULL: Hn == 256, no lane is idle (as nade_sample_kernel)
template <bool FULL>
__device__ __forceinline__ NadeLane nade_lane_setup(const float* __restrict__ bias, int enc, int Hn, int lane) {
    NadeLane L;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        L.in[q] = FULL || lane + 64 * q < Hn;
        L.off[q] = L.in[q] ? lane + 64 * q : 0;
        const float av = bias[enc + L.off[q]];
        L.a0[q] = L.in[q] ? av : 0.f;
        L.h0[q] = det_sigmoid(L.a0[q]);
    }
    return L;
}

// A wave's own LDS: logits [Dq] f32 | 256 uniforms | draws [Dq] u8.  Dq = D rounded up to 16: every carve offset is a multiple of 16 bytes if
// the workgroup's own part in front of the four waves' is one.
__host__ __device__ inline int nade_dq(int D) { return (D + 15) & ~15; }
__host__ __device__ inline size_t nade_wave_lds_bytes(int D) { return (size_t)5 * nade_dq(D) + 1024; }      // <= 8704 (D <= 1536)
struct NadeWaveLds { float* sp; float* su; unsigned char* son; };
__device__ __forceinline__ NadeWaveLds nade_wave_lds(unsigned char* waves, int wv, int D) {     // waves: behind the workgroup's own part
    unsigned char* wbase = waves + (size_t)wv * nade_wave_lds_bytes(D);
    return {reinterpret_cast<float*>(wbase), reinterpret_cast<float*>(wbase + (size_t)4 * nade_dq(D)), wbase + (size_t)4 * nade_dq(D) + 1024};
}

// one particle: what differs between the callers and between a caller's particles (filled field by field, by name: several are u32 counters)
struct NadeParticle {
    int D, Hn, Ds;                                           // Ds: visibles to scan, 0 < Ds <= D (wave-uniform)
    const float* we; const float* wd;                        // the track's [D, Hn]
    const float* sbd; const unsigned char* codes;            // LDS, staged by the workgroup: b_dec [D], codes [D]
    bool held;                                               // true: no cell of `codes` is free, no uniform is drawn (wave-uniform)
    uint64_t seed; uint32_t stream, row, sub, block0;        // the uniform of visible i: word (e0 + i) % 4 of Philox block block0 + (e0 + i) / 4
    uint32_t e0;                                             // element index of visible 0 (RNG contract: elem = m D + i)
    const float* stt; int tix, tn;                           // TEMP: the parked table; visible i draws at stt[(tix + i) % tn], tn == 0: at stt[tix]
};

// Runs the scan: W.sp[i] = the logit of visible i, W.son[i] = its value, i < Ds.  No workgroup barrier.
// FULL: Hn == 256.  TEMP: a free cell's logit is divided by its temperature before the draw.
template <bool FULL, bool TEMP>
__device__ __forceinline__ void nade_particle_scan(const NadeParticle P, const NadeLane& L, const NadeWaveLds W, int lane) {
    constexpr int RING = 8;                                  // visibles in flight, as nade_sample_kernel
    const int D = P.D, Hn = P.Hn, Ds = P.Ds;
    float a[4], h[4];
    // the hidden indices through an opaque zero: the addresses of the prologue's loads do not depend on the particle, and hoisted out of the
    // caller's particle loop they are held in registers across it (nade_is_kernel, Hn == 256: 163 -> 138 vector registers; idle lanes: 256 + 5
    // accumulation registers and one wave per SIMD -> 142 and three; profiles/nade_is.md)
    int zero = 0;
    asm volatile("" : "+v"(zero));
    int offp[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a[q] = L.a0[q];
        h[q] = L.h0[q];
        offp[q] = L.off[q] + zero;
    }
    float wdr[RING][4], wer[RING][4];                        // ring: the weight rows of visibles i .. i + RING - 1
    auto fetch = [&](int k, int i) {
        const int ii = min(i, D - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            wdr[k][q] = P.wd[(size_t)ii * Hn + offp[q]];
            wer[k][q] = P.we[(size_t)ii * Hn + offp[q]];
        }
    };
#pragma unroll
    for (int k = 0; k < RING; ++k) {
        fetch(k, k);
        __builtin_amdgcn_sched_barrier(0);                   // issue order = ring order (the waits count loads)
    }
    uint32_t b0 = P.e0 >> 2;                                 // lane l holds the uniforms of Philox block b0 + l
    auto refill = [&]() {
        if (P.held) return;                                  // wave-uniform
        float u4[4];
        philox_uniform4(P.seed, P.stream, P.row, P.sub, P.block0 + b0 + (uint32_t)lane, u4);
        *reinterpret_cast<float4*>(W.su + 4 * lane) = make_float4(u4[0], u4[1], u4[2], u4[3]);
    };
    refill();
    auto dot = [&](int k) {                                  // sum_j h_j w_dec[visible of ring slot k][j], the contract's order
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = fmaf(h[q], L.in[q] ? wdr[k][q] : 0.f, acc);
        return wave_xor_sum(acc);
    };
    auto uniform_of = [&](int i) {                           // fetched one visible ahead, with the rare Philox refill
        const uint32_t e = P.e0 + (uint32_t)min(i, D - 1);
        if ((e >> 2) >= b0 + 64u) {
            b0 += 64u;
            refill();
        }
        return W.su[e - 4u * b0];
    };
    int tix = P.tix;                                         // TEMP: the temperature of visible i is stt[tix]; tix = i % n carried along, or the track
    float t_cur = TEMP ? P.stt[tix] : 1.0f;
    float u_cur = uniform_of(0);
    float acc = dot(0);
    for (int i0 = 0; i0 < Ds; i0 += RING) {
#pragma unroll
        for (int k = 0; k < RING; ++k) {
            const int i = i0 + k;
            if (i < Ds) {                                    // uniform
                // speculation (Hn == 256, as the sampling kernel runs it): a 0 leaves the hidden state, so visible i + 1's dot product is this one
                const float spec = FULL ? dot((k + 1) % RING) : 0.f;
                const float l = P.sbd[i] + acc;
                const int code = __builtin_amdgcn_readfirstlane((int)P.codes[i]);     // the same byte in every lane: a uniform branch
                bool on;
                if (code != NADE_FREE) on = code != 0;       // held: moves a / h like a draw, its uniform is left unused
                else on = draw_below(u_cur, TEMP ? l / t_cur : l);
                if (on) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        a[q] = a[q] + (L.in[q] ? wer[k][q] : 0.f);
                        h[q] = det_sigmoid(a[q]);
                    }
                    acc = dot((k + 1) % RING);
                } else {
                    acc = FULL ? spec : dot((k + 1) % RING);
                }
                W.sp[i] = l;                                 // every lane holds the same logit and draw: one merged LDS write each
                W.son[i] = on ? 1 : 0;
                u_cur = uniform_of(i + 1);
                if (TEMP && P.tn != 0) {                     // uniform; fetched one visible ahead like the uniform
                    tix = tix + 1 == P.tn ? 0 : tix + 1;
                    t_cur = P.stt[tix];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            fetch(k, i + RING);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// the log term of a cell of value `on` whose logit is l
__device__ __forceinline__ float nade_log_term(float l, bool on) {
    const float p = det_sigmoid(l);
    return on ? logf(NADE_EPS + p) : logf(NADE_EPS + (1.0f - p));
}
// Behind the scan: log w = the sum of the GIVEN cells' log terms (`given`: the codes; a free cell carries no weight).  64 at a time: lane l adds
// visibles l, l + 64, ... in order, the butterfly adds the lanes.  (nade_sir_kernel adds the same terms in the same order inside the pass
// that forms all cells' terms, at the scan's temperature.)
__device__ __forceinline__ float nade_given_log_weight(const float* sp, const unsigned char* given, int Ds, int lane) {
    float part = 0.f;
    for (int i = lane; i < Ds; i += 64) {
        const int code = given[i];
        if (code != NADE_FREE) part += nade_log_term(sp[i], code != 0);
    }
    return wave_xor_sum(part);
}

// ---- host ----
static inline size_t nade_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Workgroups per (row, track): a workgroup's four waves take four particles at a time and stride over the row's groups (c = 4 slot + wave,
// + 4 G, ...); rows that fill the device on their own get fewer, longer-lived workgroups (the staging and b_enc are then read once per several
// groups), in equal shares.  N, tracks, C > 0.
static inline int nade_particle_workgroups(int N, int tracks, int C) {
    const int groups = cdiv(C, 4);
    const long most = cdiv(65536, (long)N * tracks);
    const int per = cdiv(groups, most < 1 ? 1 : most);
    return cdiv(groups, per);
}

// The checks every launch of the scan needs, in the words of entry point `who`, which scans a `unit` ("row" / "scan"); *G: the workgroups per unit.
static inline int nade_particle_check(const char* who, const char* unit, int tracks, int N, int D, int Hn, int ld_bias, int C, int* G) {
    MNN_REQUIRE(tracks > 0 && tracks <= 65535 && N > 0 && D > 0 && Hn > 0 && Hn <= 256,
                "%s: need 0<tracks<=65535, N,D>0 and 0<Hn<=256 (tracks=%d N=%d D=%d Hn=%d)", who, tracks, N, D, Hn);
    MNN_REQUIRE(D <= 1536, "%s: D <= 1536 (a %s's b_dec and codes and a particle's logits and draws are parked in LDS; D=%d)", who, unit, D);
    MNN_REQUIRE(ld_bias >= tracks * (Hn + D), "%s: ld_bias too small", who);
    *G = nade_particle_workgroups(N, tracks, C);
    MNN_REQUIRE((long)N * *G <= 0x7fffffffL, "%s: N * workgroups per %s = %ld exceeds the grid", who, unit, (long)N * *G);
    return MNN_OK;
}
