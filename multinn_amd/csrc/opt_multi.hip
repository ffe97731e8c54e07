// Grouped optimiser launches for gfx950: the global-norm reduction, the clipped TF-Adam step and the step-counter update of up to
// OPT_MULTI_MAX_JOBS flat parameter stores in ONE launch each, and the segment copy that packs / unpacks their gradients into one arena.
//
// A mode that trains several generators on one loss (modes.MultINNJamming, the feedback modes) steps M + 1 stores behind ONE global norm:
// per store that was sumsq + clip_adam_step + step_increment, 3 (M + 1) launches of which most cover a few hundred KB.  Here the job table
// travels by value in the argument block (the idiom of rbm_multi.hip); a workgroup finds its job by a uniform scan of the table's prefix
// of workgroup starts and then grid-strides over that job alone, with the workgroup count the single launch gives the job.  Per element
// the arithmetic of elementwise.hip's clip_adam_kernel / step_increment_kernel is restated exactly (this library is built with
// -ffp-contract=off): for the same sumsq word every job's theta / m / v / skipped / step_dev / ls_dyn / ls_good are bit for bit what
// mnn_clip_adam_step + mnn_step_increment leave.  Nothing is read on the host and there are no memset / memcpy nodes: capture-safe.
#include "common.h"

#define OPT_MULTI_MAX_JOBS 16

struct OptMultiArgs {
    mnn_opt_job job[OPT_MULTI_MAX_JOBS];
    int start[OPT_MULTI_MAX_JOBS + 1];      // workgroup j's job: start[job] <= j < start[job + 1]
    int njobs;
};
struct CopySegArgs {
    mnn_copy_seg seg[OPT_MULTI_MAX_JOBS];
    int start[OPT_MULTI_MAX_JOBS + 1];
    int nsegs;
};

// the job of this workgroup (uniform: blockIdx and the argument block are scalar)
__device__ __forceinline__ int job_of_block(const int* start, int njobs) {
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= start[j + 1]) ++j;
    return j;
}

__device__ __forceinline__ float opt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float opt_block_sum_256(float v) {
    __shared__ float part[4];
    v = opt_wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// sumsq_kernel per job: few workgroups and 16-byte loads, ONE atomic per workgroup -- every partial sum of every job lands on the one word,
// and same-address float atomics serialise (elementwise.hip: sumsq_kernel)
__global__ void __launch_bounds__(256) sumsq_multi_kernel(OptMultiArgs A, float* __restrict__ out) {
    const int j = job_of_block(A.start, A.njobs);
    const float* __restrict__ x = A.job[j].grad;
    const long n = A.job[j].n;
    const long bid = (int)blockIdx.x - A.start[j], nb = A.start[j + 1] - A.start[j];
    float acc = 0.f;
    const long n4 = (((uintptr_t)x & 15) == 0) ? n / 4 : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (long i = bid * 256L + threadIdx.x; i < n4; i += nb * 256) {
        const float4 q = x4[i];
        acc = fmaf(q.x, q.x, acc); acc = fmaf(q.y, q.y, acc); acc = fmaf(q.z, q.z, acc); acc = fmaf(q.w, q.w, acc);
    }
    for (long i = n4 * 4 + bid * 256L + threadIdx.x; i < n; i += nb * 256) acc = fmaf(x[i], x[i], acc);
    acc = opt_block_sum_256(acc);
    if (threadIdx.x == 0) atomicAdd(out, acc);
}

// clip_adam_kernel per job (step_dev form): the non-finite-norm skip, lr_t from the job's own step counter in double once per workgroup,
// the tf.clip_by_global_norm scale, 16-byte accesses where the job's own four pointers allow them
__global__ void __launch_bounds__(256) clip_adam_multi_kernel(OptMultiArgs A, const float* __restrict__ sumsq, float clip, float lr, float b1,
                                                              float b2, float eps, int sgd) {
    const int j = job_of_block(A.start, A.njobs);
    float* __restrict__ theta = A.job[j].theta;
    const float* __restrict__ grad = A.job[j].grad;
    float* __restrict__ m = A.job[j].m;
    float* __restrict__ v = A.job[j].v;
    const long n = A.job[j].n;
    const int32_t* __restrict__ step_dev = A.job[j].step_dev;
    int32_t* __restrict__ skipped = A.job[j].skipped;
    const long bid = (int)blockIdx.x - A.start[j], nb = A.start[j + 1] - A.start[j];
    if (clip > 0.f && sumsq != nullptr && !isfinite(sumsq[0])) {
        if (skipped != nullptr && bid == 0 && threadIdx.x == 0) atomicAdd(skipped, 1);
        return;
    }
    __shared__ float s_lr_t;
    if (threadIdx.x == 0) {
        const double t = (double)(step_dev[0] + 1);
        s_lr_t = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
    }
    __syncthreads();
    const float lr_t = s_lr_t;
    float scale = 1.f;
    if (clip > 0.f && sumsq != nullptr) {
        const float gn = sqrtf(sumsq[0]);
        scale = gn > 0.f ? clip * fminf(1.0f / gn, 1.0f / clip) : 1.f;   // tf.clip_by_global_norm
    }
    const bool al = ((((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    const long n4 = al ? n / 4 : 0;
    if (!sgd) {
        float4* t4 = reinterpret_cast<float4*>(theta);
        const float4* g4 = reinterpret_cast<const float4*>(grad);
        float4* m4 = reinterpret_cast<float4*>(m);
        float4* v4 = reinterpret_cast<float4*>(v);
        for (long i = bid * 256L + threadIdx.x; i < n4; i += nb * 256) {
            const float4 gq = g4[i];
            float4 mq = m4[i], vq = v4[i], tq = t4[i];
            const float ge[4] = {gq.x * scale, gq.y * scale, gq.z * scale, gq.w * scale};
            float me[4] = {mq.x, mq.y, mq.z, mq.w}, ve[4] = {vq.x, vq.y, vq.z, vq.w}, te[4] = {tq.x, tq.y, tq.z, tq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                me[e] = b1 * me[e] + (1.f - b1) * ge[e];
                ve[e] = b2 * ve[e] + (1.f - b2) * ge[e] * ge[e];
                te[e] -= lr_t * me[e] / (sqrtf(ve[e]) + eps);
            }
            m4[i] = make_float4(me[0], me[1], me[2], me[3]);
            v4[i] = make_float4(ve[0], ve[1], ve[2], ve[3]);
            t4[i] = make_float4(te[0], te[1], te[2], te[3]);
        }
    }
    for (long i = (sgd ? 0 : n4 * 4) + bid * 256L + threadIdx.x; i < n; i += nb * 256) {
        const float g = grad[i] * scale;
        if (sgd) {
            theta[i] -= lr * g;
        } else {
            const float mi = b1 * m[i] + (1.f - b1) * g;
            const float vi = b2 * v[i] + (1.f - b2) * g * g;
            m[i] = mi;
            v[i] = vi;
            theta[i] -= lr_t * mi / (sqrtf(vi) + eps);
        }
    }
}

// step_increment_kernel, lane j on job j
__global__ void __launch_bounds__(64) step_increment_multi_kernel(OptMultiArgs A, const float* __restrict__ sumsq, float clip, int grow_after,
                                                                   float m_min) {
    if ((int)threadIdx.x >= A.njobs) return;
    int32_t* step_dev = A.job[threadIdx.x].step_dev;
    float* ls_dyn = A.job[threadIdx.x].ls_dyn;
    int32_t* ls_good = A.job[threadIdx.x].ls_good;
    const bool skippedstep = clip > 0.f && sumsq != nullptr && !isfinite(sumsq[0]);
    if (ls_dyn != nullptr) {
        float m = ls_dyn[0];
        if (skippedstep) {
            m = fmaxf(m * 0.5f, m_min);
            ls_good[0] = 0;
        } else if (++ls_good[0] >= grow_after && m < 1.0f) {
            m = fminf(m * 2.0f, 1.0f);
            ls_good[0] = 0;
        }
        ls_dyn[0] = m;
        ls_dyn[1] = 1.0f / m;
    }
    if (skippedstep) return;
    step_dev[0] += 1;
}

// dst[0, n) = src[0, n) per segment: 16-byte words where the segment's two pointers allow them
__global__ void __launch_bounds__(256) segments_copy_kernel(CopySegArgs A) {
    const int j = job_of_block(A.start, A.nsegs);
    const float* __restrict__ src = A.seg[j].src;
    float* __restrict__ dst = A.seg[j].dst;
    const long n = A.seg[j].n;
    const long bid = (int)blockIdx.x - A.start[j], nb = A.start[j + 1] - A.start[j];
    const long n4 = ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) ? n / 4 : 0;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (long i = bid * 256L + threadIdx.x; i < n4; i += nb * 256) d4[i] = s4[i];
    for (long i = n4 * 4 + bid * 256L + threadIdx.x; i < n; i += nb * 256) dst[i] = src[i];
}

// the argument block of a job list: `need_update` asks for what the Adam step touches, `need_step` for the counter
static int opt_multi_args(const char* who, int njobs, const mnn_opt_job* jobs, bool need_update, bool need_step, int sgd, long per_group,
                          long max_groups, OptMultiArgs& A) {
    MNN_REQUIRE(njobs > 0 && njobs <= OPT_MULTI_MAX_JOBS && jobs, "%s: 1..%d jobs", who, OPT_MULTI_MAX_JOBS);
    memset(&A, 0, sizeof(A));
    for (int j = 0; j < njobs; ++j) {
        const mnn_opt_job& q = jobs[j];
        MNN_REQUIRE(q.grad && q.n > 0, "%s: job %d: grad is non-null, n > 0 (%ld)", who, j, q.n);
        MNN_REQUIRE(!need_update || (q.theta && (sgd || (q.m && q.v))), "%s: job %d: null theta / m / v", who, j);
        MNN_REQUIRE(!(need_update || need_step) || q.step_dev, "%s: job %d: step_dev is required (the step count is read on the device)", who, j);
        MNN_REQUIRE((q.ls_dyn == nullptr) == (q.ls_good == nullptr), "%s: job %d: ls_dyn [2] and ls_good [1] come together", who, j);
        A.job[j] = q;
        const long g = (q.n + per_group - 1) / per_group;
        A.start[j + 1] = A.start[j] + (int)(g < max_groups ? g : max_groups);
    }
    A.njobs = njobs;
    return MNN_OK;
}

extern "C" int mnn_sumsq_multi(mnn_stream_t s, int njobs, const mnn_opt_job* jobs, float* out) {
    OptMultiArgs A;
    const int rc = opt_multi_args("mnn_sumsq_multi", njobs, jobs, false, false, 0, 1024, 256, A);
    if (rc != MNN_OK) return rc;
    MNN_REQUIRE(out, "mnn_sumsq_multi: null out");
    hipLaunchKernelGGL(sumsq_multi_kernel, dim3(A.start[njobs]), dim3(256), 0, (hipStream_t)s, A, out);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

extern "C" int mnn_clip_adam_step_multi(mnn_stream_t s, int njobs, const mnn_opt_job* jobs, const float* sumsq, float clip_norm, float lr,
                                        float beta1, float beta2, float eps, int sgd) {
    OptMultiArgs A;
    const int rc = opt_multi_args("mnn_clip_adam_step_multi", njobs, jobs, true, true, sgd, 256, 2048, A);
    if (rc != MNN_OK) return rc;
    hipLaunchKernelGGL(clip_adam_multi_kernel, dim3(A.start[njobs]), dim3(256), 0, (hipStream_t)s, A, sumsq, clip_norm, lr, beta1, beta2, eps, sgd);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

extern "C" int mnn_step_increment_multi(mnn_stream_t s, int njobs, const mnn_opt_job* jobs, const float* sumsq, float clip_norm, int grow_after) {
    OptMultiArgs A;
    const int rc = opt_multi_args("mnn_step_increment_multi", njobs, jobs, false, true, 0, 1024, 1, A);
    if (rc != MNN_OK) return rc;
    for (int j = 0; j < njobs; ++j)
        MNN_REQUIRE(jobs[j].ls_dyn == nullptr || grow_after > 0, "mnn_step_increment_multi: job %d: grow_after > 0 (%d)", j, grow_after);
    hipLaunchKernelGGL(step_increment_multi_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, A, sumsq, clip_norm, grow_after, 1.0f / 1048576.0f);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

extern "C" int mnn_segments_copy(mnn_stream_t s, int nsegs, const mnn_copy_seg* segs) {
    MNN_REQUIRE(nsegs > 0 && nsegs <= OPT_MULTI_MAX_JOBS && segs, "mnn_segments_copy: 1..%d segments", OPT_MULTI_MAX_JOBS);
    CopySegArgs A;
    memset(&A, 0, sizeof(A));
    for (int j = 0; j < nsegs; ++j) {
        MNN_REQUIRE(segs[j].src && segs[j].dst && segs[j].n > 0, "mnn_segments_copy: segment %d: null pointer or n <= 0 (%ld)", j, segs[j].n);
        MNN_REQUIRE((((uintptr_t)segs[j].src | (uintptr_t)segs[j].dst) & 3) == 0, "mnn_segments_copy: segment %d: pointers are 4-byte aligned", j);
        A.seg[j] = segs[j];
        const long g = (segs[j].n + 1023) / 1024;
        A.start[j + 1] = A.start[j] + (int)(g < 1024 ? g : 1024);
    }
    A.nsegs = nsegs;
    hipLaunchKernelGGL(segments_copy_kernel, dim3(A.start[nsegs]), dim3(256), 0, (hipStream_t)s, A);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}
