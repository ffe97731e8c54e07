// Grouped RBM launches for gfx950: the Gibbs chains / free energies of up to RBM_MULTI_MAX_JOBS RBMs of one shape in ONE launch.
//
// A composer-mode LSTM-RBM (generators.RnnMultiRBM) has M per-track RBMs behind one shared LSTM: the M chains of a step are independent
// given the Dense outputs, so they are one grid with a job dimension (blockIdx.y) instead of M launches -- a sampling step at 72 intros is
// 36 two-row workgroups per track: five launches of 36 on 256 CUs become one of 180.  Every workgroup builds the GibbsView of ITS job from
// the by-value job table and runs the chain body of rbm_chain.h, the same templated body the single launches of rbm.hip instantiate:
// per job the results are bit for bit those of mnn_rbm_gibbs / mnn_rbm_gibbs_stepped on contiguous copies.  The bodies run with
// STRIDED addressing: cell (n, d) of v0 / p_v / v_out lies at n * rs + d * es, so track m of a composer-layout row (feature d * M + m;
// es = M) is read and written in place, and es = 1 addresses de-interleaved track planes.
#include "rbm_chain.h"

#define RBM_MULTI_MAX_JOBS 8

struct GibbsMultiJob {
    const float* W; const float* Wt; const float* bh; const float* bv; uint64_t seed;
    const uint8_t* v0; float* p_v; uint8_t* v_out; const uint8_t* given;
};
struct GibbsMultiArgs {
    GibbsMultiJob job[RBM_MULTI_MAX_JOBS];
    int N, D, Hn, k, ld_bh, ld_bv;
    uint32_t row0; const uint32_t* row_ids; uint32_t sub0; const int* seed_step;
    long rs, rs_given; int es;
};

__device__ __forceinline__ GibbsView gibbs_multi_view(const GibbsMultiArgs& A) {
    const GibbsMultiJob& j = A.job[blockIdx.y];
    uint64_t seed = j.seed;
    if (A.seed_step != nullptr) seed += (uint64_t)(int64_t)*A.seed_step;      // step counter on the device: a captured launch draws anew every replay
    return GibbsView{A.N, A.D, A.Hn, A.k, j.v0, j.W, j.Wt, j.bh, A.ld_bh, j.bv, A.ld_bv, seed, A.row0, A.row_ids, A.sub0, j.p_v, j.v_out,
                     j.given, A.rs_given, A.rs, A.es};
}

// a grouped launch with temperatures: the same table with one temperature per job behind it.  The kernels that take it are the TEMPERED
// instantiations; a launch whose temperatures are all 1 never comes here (the kernels and the argument block below it are unchanged)
struct GibbsMultiTempArgs { GibbsMultiArgs A; float temp[RBM_MULTI_MAX_JOBS]; };
__device__ __forceinline__ GibbsView gibbs_multi_view(const GibbsMultiTempArgs& T) {
    GibbsView v = gibbs_multi_view(T.A);
    v.temp = T.temp[blockIdx.y];
    return v;
}

template <int R, int RGH, int RGV, bool GIVEN>
__global__ void __launch_bounds__(256) rbm_gibbs_multi_lds_kernel(GibbsMultiArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_lds_body<R, RGH, RGV, GIVEN, true>(gibbs_multi_view(A), blockIdx.x * R, smem);
}

template <bool GIVEN>
__global__ void __launch_bounds__(512) rbm_gibbs_multi_mfma_kernel(GibbsMultiArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_mfma_body<GIVEN, true>(gibbs_multi_view(A), blockIdx.x * GM_ROWS, smem);
}

template <bool GIVEN>
__global__ void __launch_bounds__(256) rbm_gibbs_multi_stream_kernel(GibbsMultiArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_stream_body<GIVEN, true>(gibbs_multi_view(A), blockIdx.x * RBM_R, smem);
}

template <int R, int RGH, int RGV, bool GIVEN>
__global__ void __launch_bounds__(256) rbm_gibbs_multi_temp_lds_kernel(GibbsMultiTempArgs T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_lds_body<R, RGH, RGV, GIVEN, true, true>(gibbs_multi_view(T), blockIdx.x * R, smem);
}
template <bool GIVEN>
__global__ void __launch_bounds__(512) rbm_gibbs_multi_temp_mfma_kernel(GibbsMultiTempArgs T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_mfma_body<GIVEN, true, true>(gibbs_multi_view(T), blockIdx.x * GM_ROWS, smem);
}
template <bool GIVEN>
__global__ void __launch_bounds__(256) rbm_gibbs_multi_temp_stream_kernel(GibbsMultiTempArgs T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rbm_gibbs_stream_body<GIVEN, true, true>(gibbs_multi_view(T), blockIdx.x * RBM_R, smem);
}

// dynamic LDS above 64 KB has to be asked for once per kernel and device
static bool raise_lds(const void* fn, bool (&flags)[64]) {
    bool& raised = mnn_dev_flag(flags);
    if (!raised) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        raised = true;
    }
    return true;
}

// T == nullptr: the untempered kernels; otherwise the TEMPERED ones with T's temperatures
template <int R, int RGH, int RGV, bool GIVEN>
static bool launch_multi_lds(hipStream_t st, const GibbsMultiArgs& A, int njobs, const GibbsMultiTempArgs* T) {
    static bool raised_[64], raised_t_[64];
    const dim3 grid(cdiv(A.N, R), njobs);
    const size_t lds = rbm_lds_resident_bytes(R, A.D, A.Hn);
    if (T != nullptr) {
        if (!raise_lds(reinterpret_cast<const void*>(&rbm_gibbs_multi_temp_lds_kernel<R, RGH, RGV, GIVEN>), raised_t_)) return false;
        hipLaunchKernelGGL((rbm_gibbs_multi_temp_lds_kernel<R, RGH, RGV, GIVEN>), grid, dim3(256), lds, st, *T);
        return true;
    }
    if (!raise_lds(reinterpret_cast<const void*>(&rbm_gibbs_multi_lds_kernel<R, RGH, RGV, GIVEN>), raised_)) return false;
    hipLaunchKernelGGL((rbm_gibbs_multi_lds_kernel<R, RGH, RGV, GIVEN>), grid, dim3(256), lds, st, A);
    return true;
}

// the instantiation for this shape: the choice of rbm.hip's try_gibbs_lds
template <bool GIVEN>
static bool try_multi_lds(hipStream_t st, const GibbsMultiArgs& A, int njobs, const GibbsMultiTempArgs* T) {
    const int gh = 256 / A.Hn, gv = 256 / A.D;
    if (rbm_lds_resident_bytes(2, A.D, A.Hn) > 158 * 1024) return false;
    return gv >= 2 ? (gh >= 2 ? launch_multi_lds<2, 1, 1, GIVEN>(st, A, njobs, T) : launch_multi_lds<2, 2, 1, GIVEN>(st, A, njobs, T))
                   : (gh >= 2 ? launch_multi_lds<2, 1, 2, GIVEN>(st, A, njobs, T) : launch_multi_lds<2, 2, 2, GIVEN>(st, A, njobs, T));
}

extern "C" int mnn_transpose(mnn_stream_t s, const void* in, int in_dtype, int R, int C, int ld_in, void* out, int out_dtype, int ld_out);

// temps: NULL (every job at temperature 1) or njobs positive finite temperatures; all of them 1 is NULL
extern "C" int mnn_rbm_gibbs_multi_temps(mnn_stream_t s, int njobs, const mnn_rbm_gibbs_job* jobs, int N, int D, int Hn, int k, int ld_bh, int ld_bv,
                                         uint32_t row0, const uint32_t* row_ids, uint32_t sub0, const int* seed_step, long row_stride, int elem_stride,
                                         long given_row_stride, void* workspace, const float* temps) {
    MNN_REQUIRE(njobs > 0 && njobs <= RBM_MULTI_MAX_JOBS && jobs, "mnn_rbm_gibbs_multi: 1..%d jobs", RBM_MULTI_MAX_JOBS);
    MNN_REQUIRE(N > 0 && D > 0 && Hn > 0 && k >= 0, "mnn_rbm_gibbs_multi: bad sizes N=%d D=%d Hn=%d k=%d", N, D, Hn, k);
    MNN_REQUIRE((ld_bh == 0 || ld_bh >= Hn) && (ld_bv == 0 || ld_bv >= D), "mnn_rbm_gibbs_multi: bad bias leading dimension");
    MNN_REQUIRE(elem_stride >= 1 && (row_stride >= (long)(D - 1) * elem_stride + 1 || N == 1), "mnn_rbm_gibbs_multi: bad strides (row %ld, element %d)",
                row_stride, elem_stride);
    MNN_REQUIRE(workspace, "mnn_rbm_gibbs_multi: null workspace");
    const bool given = jobs[0].given != nullptr;
    MNN_REQUIRE(!given || given_row_stride >= (long)(D - 1) * elem_stride + 1 || N == 1, "mnn_rbm_gibbs_multi: given row stride %ld", given_row_stride);
    GibbsMultiArgs A;
    memset(&A, 0, sizeof(A));
    for (int j = 0; j < njobs; ++j) {
        const mnn_rbm_gibbs_job& q = jobs[j];
        MNN_REQUIRE(q.W && q.bh && q.bv && q.v0, "mnn_rbm_gibbs_multi: job %d: null pointer", j);
        MNN_REQUIRE((q.given != nullptr) == given, "mnn_rbm_gibbs_multi: job %d: `given` must be set on every job or on none", j);
        A.job[j] = GibbsMultiJob{q.W, nullptr, q.bh, q.bv, q.seed, q.v0, q.p_v, q.v_out, q.given};
    }
    A.N = N; A.D = D; A.Hn = Hn; A.k = k; A.ld_bh = ld_bh; A.ld_bv = ld_bv;
    A.row0 = row0; A.row_ids = row_ids; A.sub0 = sub0; A.seed_step = seed_step;
    A.rs = row_stride; A.rs_given = given_row_stride; A.es = elem_stride;
    bool tempered = false;
    GibbsMultiTempArgs TA;
    memset(&TA, 0, sizeof(TA));
    for (int j = 0; j < njobs && temps != nullptr; ++j) {
        MNN_REQUIRE(temps[j] > 0.f && temps[j] <= 3.0e38f, "mnn_rbm_gibbs_multi_temps: job %d: the temperature is a positive finite number (%g)", j, (double)temps[j]);
        TA.temp[j] = temps[j];
        tempered = tempered || temps[j] != 1.0f;
    }
    const GibbsMultiTempArgs* T = tempered ? &TA : nullptr;      // (the streaming form completes A -- and TA.A -- below)
    TA.A = A;
    const size_t codes_lds = given ? (size_t)RBM_R * ((D + 3) & ~3) : 0;
    MNN_REQUIRE(rbm_lds_bytes(D, Hn) + codes_lds <= 160 * 1024, "mnn_rbm_gibbs_multi: D+Hn too large for LDS");
    hipStream_t st = (hipStream_t)s;
    // the dispatch of mnn_rbm_gibbs, with a job dimension on the grid
    if (N < 2048 && Hn <= 256 && D <= 256 && getenv("MNN_RBM_STREAM_W") == nullptr) {
        // sampling-sized batches: W resident in LDS, two rows per workgroup, every workgroup loads its job's W
        if (given ? try_multi_lds<true>(st, A, njobs, T) : try_multi_lds<false>(st, A, njobs, T)) {
            MNN_LAUNCH_CHECK();
            return MNN_OK;
        }
    }
    if (gibbs_mfma_lds_bytes(D, Hn) <= 158 * 1024 && getenv("MNN_RBM_NO_MFMA") == nullptr) {
        // training batches: the chains on the f32 matrix cores, 64 rows per workgroup
        static bool raised_[64], raised_g_[64], raised_t_[64], raised_tg_[64];
        const void* fn = tempered ? (given ? reinterpret_cast<const void*>(&rbm_gibbs_multi_temp_mfma_kernel<true>) : reinterpret_cast<const void*>(&rbm_gibbs_multi_temp_mfma_kernel<false>))
                                  : (given ? reinterpret_cast<const void*>(&rbm_gibbs_multi_mfma_kernel<true>) : reinterpret_cast<const void*>(&rbm_gibbs_multi_mfma_kernel<false>));
        bool& raised = tempered ? (given ? mnn_dev_flag(raised_tg_) : mnn_dev_flag(raised_t_)) : (given ? mnn_dev_flag(raised_g_) : mnn_dev_flag(raised_));
        if (!raised) {
            MNN_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            raised = true;
        }
        if (tempered && given)
            hipLaunchKernelGGL(rbm_gibbs_multi_temp_mfma_kernel<true>, dim3(cdiv(N, GM_ROWS), njobs), dim3(512), gibbs_mfma_lds_bytes(D, Hn), st, TA);
        else if (tempered)
            hipLaunchKernelGGL(rbm_gibbs_multi_temp_mfma_kernel<false>, dim3(cdiv(N, GM_ROWS), njobs), dim3(512), gibbs_mfma_lds_bytes(D, Hn), st, TA);
        else if (given)
            hipLaunchKernelGGL(rbm_gibbs_multi_mfma_kernel<true>, dim3(cdiv(N, GM_ROWS), njobs), dim3(512), gibbs_mfma_lds_bytes(D, Hn), st, A);
        else
            hipLaunchKernelGGL(rbm_gibbs_multi_mfma_kernel<false>, dim3(cdiv(N, GM_ROWS), njobs), dim3(512), gibbs_mfma_lds_bytes(D, Hn), st, A);
        MNN_LAUNCH_CHECK();
        return MNN_OK;
    }
    // neither fits: the streaming chain (W and a transposed copy per job from L2), still one launch over the jobs
    for (int j = 0; j < njobs; ++j) {
        float* wt = (float*)workspace + (size_t)j * D * Hn;
        int rc = mnn_transpose(s, A.job[j].W, MNN_F32, D, Hn, Hn, wt, MNN_F32, D);
        if (rc != MNN_OK) return rc;
        A.job[j].Wt = wt;
    }
    TA.A = A;
    if (tempered && given)
        hipLaunchKernelGGL(rbm_gibbs_multi_temp_stream_kernel<true>, dim3(cdiv(N, RBM_R), njobs), dim3(256), rbm_lds_bytes(D, Hn) + codes_lds, st, TA);
    else if (tempered)
        hipLaunchKernelGGL(rbm_gibbs_multi_temp_stream_kernel<false>, dim3(cdiv(N, RBM_R), njobs), dim3(256), rbm_lds_bytes(D, Hn), st, TA);
    else if (given)
        hipLaunchKernelGGL(rbm_gibbs_multi_stream_kernel<true>, dim3(cdiv(N, RBM_R), njobs), dim3(256), rbm_lds_bytes(D, Hn) + codes_lds, st, A);
    else
        hipLaunchKernelGGL(rbm_gibbs_multi_stream_kernel<false>, dim3(cdiv(N, RBM_R), njobs), dim3(256), rbm_lds_bytes(D, Hn), st, A);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}

extern "C" int mnn_rbm_gibbs_multi(mnn_stream_t s, int njobs, const mnn_rbm_gibbs_job* jobs, int N, int D, int Hn, int k, int ld_bh, int ld_bv,
                                   uint32_t row0, const uint32_t* row_ids, uint32_t sub0, const int* seed_step, long row_stride, int elem_stride,
                                   long given_row_stride, void* workspace) {
    return mnn_rbm_gibbs_multi_temps(s, njobs, jobs, N, D, Hn, k, ld_bh, ld_bv, row0, row_ids, sub0, seed_step, row_stride, elem_stride,
                                     given_row_stride, workspace, nullptr);
}

// ----------------------------------------------------------------------------------------------
// free energy (and optional hidden activations) of every job's rows in one launch: the body of mnn_rbm_free_energy, job = blockIdx.y
// ----------------------------------------------------------------------------------------------
struct FreeEnergyMultiArgs {
    mnn_rbm_free_energy_job job[RBM_MULTI_MAX_JOBS];
    int N, D, Hn, ld_bh, ld_bv;
};

__global__ void __launch_bounds__(256) rbm_free_energy_multi_kernel(FreeEnergyMultiArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float fsum[4 * RBM_R];
    const mnn_rbm_free_energy_job& j = A.job[blockIdx.y];
    rbm_free_energy_body(A.N, A.D, A.Hn, j.v, j.W, j.bh, A.ld_bh, j.bv, A.ld_bv, j.F, j.p_h, blockIdx.x * RBM_R, smem, fsum);
}

extern "C" int mnn_rbm_free_energy_multi(mnn_stream_t s, int njobs, const mnn_rbm_free_energy_job* jobs, int N, int D, int Hn, int ld_bh, int ld_bv) {
    MNN_REQUIRE(njobs > 0 && njobs <= RBM_MULTI_MAX_JOBS && jobs, "mnn_rbm_free_energy_multi: 1..%d jobs", RBM_MULTI_MAX_JOBS);
    MNN_REQUIRE(N > 0 && D > 0 && Hn > 0, "mnn_rbm_free_energy_multi: bad sizes");
    MNN_REQUIRE((ld_bh == 0 || ld_bh >= Hn) && (ld_bv == 0 || ld_bv >= D), "mnn_rbm_free_energy_multi: bad bias leading dimension");
    FreeEnergyMultiArgs A;
    memset(&A, 0, sizeof(A));
    for (int j = 0; j < njobs; ++j) {
        MNN_REQUIRE(jobs[j].v && jobs[j].W && jobs[j].bh && jobs[j].bv && jobs[j].F, "mnn_rbm_free_energy_multi: job %d: null pointer", j);
        A.job[j] = jobs[j];
    }
    A.N = N; A.D = D; A.Hn = Hn; A.ld_bh = ld_bh; A.ld_bv = ld_bv;
    const size_t lds = (size_t)RBM_R * ((D + 3) & ~3) * sizeof(float);
    hipLaunchKernelGGL(rbm_free_energy_multi_kernel, dim3(cdiv(N, RBM_R), njobs), dim3(256), lds, (hipStream_t)s, A);
    MNN_LAUNCH_CHECK();
    return MNN_OK;
}
