// Training windows cut out of a device-resident dataset (multinn_amd/device_data.py): out[b, t, d] = X[ids[b], j + t, e0 + d * es].
#include "common.h"

// One byte vector of V in {1, 2, 4, 8, 16} bytes.
template <int V> struct WinVec;
template <> struct WinVec<1> { typedef uint8_t type; };
template <> struct WinVec<2> { typedef uint16_t type; };
template <> struct WinVec<4> { typedef uint32_t type; };
template <> struct WinVec<8> { typedef uint2 type; };
template <> struct WinVec<16> { typedef uint4 type; };

#define WIN_THREADS 256
#define WIN_PER_THREAD 4                                // vectors in flight per lane: 16 KiB per workgroup at V = 16

// the song of output row b, or -1 for an id outside [0, S): that row is zeros with length 0 and nothing of X is read for it
__device__ __forceinline__ long window_song(const int32_t* __restrict__ ids, int b, long S) {
    const long id = ids[b];
    return id >= 0 && id < S ? id : -1;
}
__device__ __forceinline__ void window_length(const int32_t* __restrict__ lengths, long id, int j, int Tw, int32_t* __restrict__ out_len, int b) {
    if (out_len != nullptr && blockIdx.x == 0 && threadIdx.x == 0) out_len[b] = id < 0 ? 0 : min(max(lengths[id] - j, 0), Tw);
}

// The joint window: row b is ONE contiguous run of n = Tw * D bytes at byte (ids[b] * T + j) * D of X.  Both that offset and b * n are
// multiples of D, so with 16-byte aligned bases every row starts on a multiple of V = gcd(D, 16) bytes and n is a whole number of vectors
// (no byte tail is left).  Grid: x over chunks of WIN_THREADS * WIN_PER_THREAD vectors of a row, y over rows; the last chunk of a row may be
// partial and is copied vector by vector under its bound.
template <int V>
__global__ void __launch_bounds__(WIN_THREADS) window_copy_kernel(const uint8_t* __restrict__ X, long S, long row_pitch /* T * D */, long n_vec,
                                                                  const int32_t* __restrict__ ids, int B, long j_off /* j * D */, int j, int Tw,
                                                                  const int32_t* __restrict__ lengths, uint8_t* __restrict__ out,
                                                                  int32_t* __restrict__ out_len) {
    typedef typename WinVec<V>::type vec_t;
    const long v0 = (long)blockIdx.x * (WIN_THREADS * WIN_PER_THREAD) + threadIdx.x;
    const bool whole = ((long)blockIdx.x + 1) * (WIN_THREADS * WIN_PER_THREAD) <= n_vec;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long id = window_song(ids, b, S);
        window_length(lengths, id, j, Tw, out_len, b);
        vec_t* __restrict__ dst = reinterpret_cast<vec_t*>(out + (long)b * n_vec * V);
        const vec_t* __restrict__ src = reinterpret_cast<const vec_t*>(X + max(id, 0L) * row_pitch + j_off);   // not read when id < 0
        if (id >= 0 && whole) {                                  // an interior chunk: every load of the lane in flight before its first store
            vec_t q[WIN_PER_THREAD];
#pragma unroll
            for (int k = 0; k < WIN_PER_THREAD; ++k) q[k] = src[v0 + k * WIN_THREADS];
#pragma unroll
            for (int k = 0; k < WIN_PER_THREAD; ++k) dst[v0 + k * WIN_THREADS] = q[k];
            continue;
        }
#pragma unroll
        for (int k = 0; k < WIN_PER_THREAD; ++k) {               // the row's last, partial chunk; the zeros of a bad id
            const long v = v0 + k * WIN_THREADS;
            if (v < n_vec) dst[v] = id >= 0 ? src[v] : vec_t{};
        }
    }
}

// The strided byte gather (one track of a [S, T, P, M] roll: es = M, e0 = m, Dout = P): one output byte per lane, 64-bit offsets.
__global__ void __launch_bounds__(WIN_THREADS) window_gather_kernel(const uint8_t* __restrict__ X, long S, long row_pitch, int D,
                                                                    const int32_t* __restrict__ ids, int B, int j, int Tw, int e0, int es, int Dout,
                                                                    const int32_t* __restrict__ lengths, uint8_t* __restrict__ out,
                                                                    int32_t* __restrict__ out_len) {
    const long n = (long)Tw * Dout;
    const long e = (long)blockIdx.x * WIN_THREADS + threadIdx.x;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long id = window_song(ids, b, S);
        window_length(lengths, id, j, Tw, out_len, b);
        if (e >= n) continue;
        const long t = e / Dout, d = e - t * Dout;
        out[(long)b * n + e] = id < 0 ? (uint8_t)0 : X[id * row_pitch + (j + t) * D + e0 + d * es];
    }
}

template <int V>
static void window_copy_launch(hipStream_t st, const uint8_t* X, long S, int T, int D, const int32_t* ids, int B, int j, int Tw, const int32_t* lengths,
                               uint8_t* out, int32_t* out_len) {
    const long n_vec = (long)Tw * D / V;
    const dim3 grid(cdiv(n_vec, WIN_THREADS * WIN_PER_THREAD), std::min(B, 65535));
    hipLaunchKernelGGL(window_copy_kernel<V>, grid, dim3(WIN_THREADS), 0, st, X, S, (long)T * D, n_vec, ids, B, (long)j * D, j, Tw, lengths, out, out_len);
}

extern "C" int mnn_window_gather(mnn_stream_t s, const uint8_t* X, long S, int T, int D, const int32_t* ids, int B, int j, int Tw, int e0, int es, int Dout,
                                 const int32_t* lengths, uint8_t* out, int32_t* out_len) {
    MNN_REQUIRE(S > 0 && T > 0 && D > 0 && B > 0 && Tw > 0 && Dout > 0, "mnn_window_gather: S, T, D, B, Tw and Dout must be positive (got %ld, %d, %d, %d, %d, %d)",
                S, T, D, B, Tw, Dout);
    MNN_REQUIRE(j >= 0 && (long)j + Tw <= T, "mnn_window_gather: the window j = %d, Tw = %d leaves the %d steps of the dataset", j, Tw, T);
    MNN_REQUIRE(es >= 1 && e0 >= 0 && (long)e0 + (long)(Dout - 1) * es < D, "mnn_window_gather: features e0 = %d, es = %d, Dout = %d leave the D = %d of the dataset",
                e0, es, Dout, D);
    MNN_REQUIRE(X && ids && out, "mnn_window_gather: X, ids and out must not be NULL");
    MNN_REQUIRE(out_len == nullptr || lengths != nullptr, "mnn_window_gather: out_len needs lengths");
    MNN_REQUIRE((long)Tw * Dout / WIN_THREADS < (1L << 31), "mnn_window_gather: a window row of %ld bytes is too long", (long)Tw * Dout);
    const hipStream_t st = (hipStream_t)s;
    if (es == 1 && Dout == D) {
        // the widest power of two that divides D and both bases (<= 16): every row of either side starts on a multiple of it
        const uintptr_t bits = (uintptr_t)D | (uintptr_t)X | (uintptr_t)out | 16u;
        switch ((int)(bits & (~bits + 1))) {
            case 16: window_copy_launch<16>(st, X, S, T, D, ids, B, j, Tw, lengths, out, out_len); break;
            case 8: window_copy_launch<8>(st, X, S, T, D, ids, B, j, Tw, lengths, out, out_len); break;
            case 4: window_copy_launch<4>(st, X, S, T, D, ids, B, j, Tw, lengths, out, out_len); break;
            case 2: window_copy_launch<2>(st, X, S, T, D, ids, B, j, Tw, lengths, out, out_len); break;
            default: window_copy_launch<1>(st, X, S, T, D, ids, B, j, Tw, lengths, out, out_len); break;
        }
    } else {
        const dim3 grid(cdiv((long)Tw * Dout, WIN_THREADS), std::min(B, 65535));
        hipLaunchKernelGGL(window_gather_kernel, grid, dim3(WIN_THREADS), 0, st, X, S, (long)T * D, D, ids, B, j, Tw, e0, es, Dout, lengths, out, out_len);
    }
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

// ---- transposition (pitch shift) inside the gather ------------------------------------------------------------------------------------
// Feature f of a [P, M] step is cell (p, m) = (f / M, f % M).  An output byte that reads feature f of a MOVING track (bit m of `moving`)
// reads cell (p - shifts[b], m) instead, or nothing (0) where p - shifts[b] leaves 0..P-1; a byte of a track that stays is the plain
// gather's.  One output byte per lane, like window_gather_kernel, for the joint row (e0 = 0, es = 1, Dout = D) and the single track
// (e0 = m, es = M, Dout = P) alike.  p - shifts[b] is formed in 64 bits and compared with [0, P) BEFORE it is used, so no int32 shift
// indexes outside the time step it belongs to: every read is X[id, j + t, q * M + m] with 0 <= q < P, m < M, q * M + m < D.
__global__ void __launch_bounds__(WIN_THREADS) window_gather_shift_kernel(const uint8_t* __restrict__ X, long S, long row_pitch, int D,
                                                                          const int32_t* __restrict__ ids, const int32_t* __restrict__ shifts, int B,
                                                                          int j, int Tw, int e0, int es, int Dout, int M, uint32_t moving,
                                                                          const int32_t* __restrict__ lengths, uint8_t* __restrict__ out,
                                                                          int32_t* __restrict__ out_len) {
    const unsigned n = (unsigned)Tw * (unsigned)Dout;                     // < 2^31 (checked on the host)
    const unsigned e = blockIdx.x * WIN_THREADS + threadIdx.x;
    const unsigned t = e / (unsigned)Dout, d = e - t * (unsigned)Dout;
    const unsigned f = (unsigned)e0 + d * (unsigned)es;                   // < D for e < n
    const unsigned p = f / (unsigned)M, m = f - p * (unsigned)M;
    const bool moves = (moving >> m) & 1u;
    const long P = D / M;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long id = window_song(ids, b, S);
        window_length(lengths, id, j, Tw, out_len, b);
        if (e >= n) continue;
        const long q = moves ? (long)p - (long)shifts[b] : (long)p;
        uint8_t v = 0;
        if (id >= 0 && q >= 0 && q < P) v = X[id * row_pitch + (long)(j + t) * D + q * M + m];
        out[(long)b * n + e] = v;
    }
}

extern "C" int mnn_window_gather_shift(mnn_stream_t s, const uint8_t* X, long S, int T, int D, const int32_t* ids, int B, int j, int Tw, int e0, int es,
                                       int Dout, const int32_t* lengths, uint8_t* out, int32_t* out_len, const int32_t* shifts, int M, uint32_t moving) {
    MNN_REQUIRE(S > 0 && T > 0 && D > 0 && B > 0 && Tw > 0 && Dout > 0,
                "mnn_window_gather_shift: S, T, D, B, Tw and Dout must be positive (got %ld, %d, %d, %d, %d, %d)", S, T, D, B, Tw, Dout);
    MNN_REQUIRE(j >= 0 && (long)j + Tw <= T, "mnn_window_gather_shift: the window j = %d, Tw = %d leaves the %d steps of the dataset", j, Tw, T);
    MNN_REQUIRE(es >= 1 && e0 >= 0 && (long)e0 + (long)(Dout - 1) * es < D,
                "mnn_window_gather_shift: features e0 = %d, es = %d, Dout = %d leave the D = %d of the dataset", e0, es, Dout, D);
    MNN_REQUIRE(X && ids && out, "mnn_window_gather_shift: X, ids and out must not be NULL");
    MNN_REQUIRE(shifts != nullptr, "mnn_window_gather_shift: shifts must not be NULL (mnn_window_gather is the gather without shifts)");
    MNN_REQUIRE(M >= 1 && M <= 32 && D % M == 0, "mnn_window_gather_shift: tracks M = %d must lie in 1..32 and divide D = %d", M, D);
    MNN_REQUIRE(out_len == nullptr || lengths != nullptr, "mnn_window_gather_shift: out_len needs lengths");
    MNN_REQUIRE((long)Tw * Dout < (1L << 31), "mnn_window_gather_shift: a window row of %ld bytes is too long", (long)Tw * Dout);
    const dim3 grid(cdiv((long)Tw * Dout, WIN_THREADS), std::min(B, 65535));
    hipLaunchKernelGGL(window_gather_shift_kernel, grid, dim3(WIN_THREADS), 0, (hipStream_t)s, X, S, (long)T * D, D, ids, shifts, B, j, Tw, e0, es, Dout, M,
                       moving, lengths, out, out_len);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

// The pitch range a song's moving tracks occupy: lo[s] / hi[s] = the smallest / largest p with X[s, t, p, m] != 0 for some t < lengths[s]
// (all T steps without lengths) and some moving m; lo = P, hi = -1 where there is none.  Runs once per dataset and set of tracks: one
// workgroup per song, each lane walks the steps of its features (p and m fixed per lane: consecutive lanes read consecutive bytes), then
// a min / max over the wave by shuffles and over the workgroup through LDS.
__global__ void __launch_bounds__(WIN_THREADS) pitch_extent_kernel(const uint8_t* __restrict__ X, int T, int D, int M, uint32_t moving,
                                                                   const int32_t* __restrict__ lengths, int32_t* __restrict__ lo,
                                                                   int32_t* __restrict__ hi) {
    __shared__ int32_t s_lo[WIN_THREADS / 64], s_hi[WIN_THREADS / 64];
    const long song = blockIdx.x;
    const int len = lengths == nullptr ? T : min(max(lengths[song], 0), T);
    const uint8_t* __restrict__ x = X + song * (long)T * D;
    int32_t l = D / M, h = -1;
    for (int f = threadIdx.x; f < D; f += WIN_THREADS) {
        const int p = f / M, m = f - p * M;
        if (!((moving >> m) & 1u)) continue;
        uint32_t any = 0;
        for (int t = 0; t < len; ++t) any |= x[(long)t * D + f];
        if (any) l = min(l, p), h = max(h, p);
    }
    for (int o = 32; o > 0; o >>= 1) l = min(l, __shfl_down(l, o, 64)), h = max(h, __shfl_down(h, o, 64));
    if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = l, s_hi[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WIN_THREADS / 64; ++w) l = min(l, s_lo[w]), h = max(h, s_hi[w]);
        lo[song] = l;
        hi[song] = h;
    }
}

extern "C" int mnn_pitch_extent(mnn_stream_t s, const uint8_t* X, long S, int T, int D, int M, uint32_t moving, const int32_t* lengths, int32_t* lo,
                                int32_t* hi) {
    MNN_REQUIRE(S > 0 && S < (1L << 31) && T > 0 && D > 0, "mnn_pitch_extent: S, T and D must be positive, S below 2^31 (got %ld, %d, %d)", S, T, D);
    MNN_REQUIRE(M >= 1 && M <= 32 && D % M == 0, "mnn_pitch_extent: tracks M = %d must lie in 1..32 and divide D = %d", M, D);
    MNN_REQUIRE(X && lo && hi, "mnn_pitch_extent: X, lo and hi must not be NULL");
    hipLaunchKernelGGL(pitch_extent_kernel, dim3((unsigned)S), dim3(WIN_THREADS), 0, (hipStream_t)s, X, T, D, M, moving, lengths, lo, hi);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}
