// Device helpers of the NADE visible-order scans that more than one translation unit uses (nade.hip: log_prob, sampling; nade_particle.h: the
// clamped particle scan of nade_is.hip and nade_sir.hip).  The arithmetic of the sampling contract lives here, so every scan that states "the
// dot product and the draw of nade_sample_kernel" runs the same instructions.
#pragma once
#include "common.h"

#define NADE_EPS 1e-6f

// The temperatures of a launch (nade.hip: TMODE 2 only, the other modes never read it; nade_sir.hip: the TEMP instantiations).  by_visible == 0:
// job / track j (blockIdx.y) draws at t[j] -- the launcher fills all eight entries, a scalar eight times; by_visible == 1: visible i of every
// job draws at t[i % n] (the joint NADE orders its visibles p M + m: one temperature per track).
struct SampleTemps { float t[MNN_TEMPS_MAX]; int n; int by_visible; };
// the table parked in LDS (eight floats at `stt`): every lane selects its entry with constant indices -- the by-value argument stays in scalar
// registers -- and the scan then reads the entry of a running index, a broadcast (visible-at-a-time scans) or per-lane (chunk kernel) LDS read
__device__ __forceinline__ void sample_temps_park(const SampleTemps& TT, int lane, float* stt) {
    float tv = TT.t[0];
#pragma unroll
    for (int k = 1; k < MNN_TEMPS_MAX; ++k) tv = (lane & (MNN_TEMPS_MAX - 1)) == k ? TT.t[k] : tv;
    if (lane < MNN_TEMPS_MAX) stt[lane] = tv;
}

__device__ __forceinline__ float dpp_xor8(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, false)); }
// x[l ^ 4] without the LDS crossbar (a ds_swizzle is ~100 cycles on a dependent chain): two row shifts by four lanes, each written to the
// banks (groups of four lanes) it is right for -- row_shl:4 (lane l reads l + 4) into banks 0 and 2, row_shr:4 (l - 4) into banks 1 and 3
__device__ __forceinline__ float dpp_xor4(float x) {
    int t = __builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x104, 0xf, 0x5, false);
    t = __builtin_amdgcn_update_dpp(t, __float_as_int(x), 0x114, 0xf, 0xa, false);
    return __int_as_float(t);
}
__device__ __forceinline__ float dpp_xor2(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, false)); }
__device__ __forceinline__ float dpp_xor1(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, false)); }

// the xor butterfly 32..1 of the sampling contract (DESIGN.md "Deterministic sampling") on permlane swaps / DPP: each step adds the same two
// numbers as the shuffle form, so every lane ends with the same bits
__device__ __forceinline__ float wave_xor_sum(float x) {
    {
        auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);     // x[l] + x[l ^ 32]
        x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    {
        auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);     // x[l] + x[l ^ 16]
        x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    x = x + dpp_xor8(x);
    x = x + dpp_xor4(x);
    x = x + dpp_xor2(x);
    x = x + dpp_xor1(x);
    return x;
}

// The draw 1[u < det_sigmoid(x)] (or det_sigmoid(x) >= 1/2) decided WITHOUT the 35-operation deterministic sigmoid on the serial chain:
// the hardware exp2 / rcp give the probability to ~1e-5 relative (argument scaling of exp2 included), which settles every draw
// whose uniform is not within 1e-4 (relative) of it; the rare rest takes the exact comparison.  The outcome is the exact one always.
__device__ __forceinline__ float sig_approx(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-x * 1.4426950408889634f));
}
__device__ __forceinline__ bool draw_below(float u, float x) {          // u < det_sigmoid(x); wave-uniform operands
    const float r = sig_approx(x);
    const float d = u - r;
    if (__builtin_amdgcn_ballot_w64(fabsf(d) > 1e-4f * r + 1e-30f) != 0ull) return __builtin_amdgcn_ballot_w64(d < 0.f) != 0ull;
    return __builtin_amdgcn_ballot_w64(u < det_sigmoid(x)) != 0ull;
}
__device__ __forceinline__ bool prob_at_least_half(float x) {           // det_sigmoid(x) >= 0.5f
    const float d = sig_approx(x) - 0.5f;
    if (__builtin_amdgcn_ballot_w64(fabsf(d) > 1e-4f) != 0ull) return __builtin_amdgcn_ballot_w64(d > 0.f) != 0ull;
    return __builtin_amdgcn_ballot_w64(det_sigmoid(x) >= 0.5f) != 0ull;
}
