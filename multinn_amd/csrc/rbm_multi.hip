// Grouped RBM launches for gfx950: the Gibbs chains / free energies of up to RBM_MULTI_MAX_JOBS RBMs of one shape in ONE launch.
//
// A composer-mode LSTM-RBM (generators.RnnMultiRBM) has M per-track RBMs behind one shared LSTM: the M chains of a step are independent
// given the Dense outputs, so they are one grid with a job dimension (blockIdx.y) instead of M launches -- a sampling step at 72 intros is
// 36 two-row workgroups per track: five launches of 36 on 256 CUs become one of 180.  The entry points fill the job-table argument block of
// rbm_chain.h and call its dispatch -- the kernel templates, thresholds and forms of the single launches of rbm.hip: per job the results are
// bit for bit those of mnn_rbm_gibbs / _stepped / _temp on contiguous copies.  The bodies run with
// STRIDED addressing: cell (n, d) of v0 / p_v / v_out lies at n * rs + d * es, so track m of a composer-layout row (feature d * M + m;
// es = M) is read and written in place, and es = 1 addresses de-interleaved track planes.
#include "rbm_chain.h"

// temps: NULL (every job at temperature 1) or njobs positive finite temperatures; all of them 1 selects the untempered kernels
// sub_base: NULL, or one u32 on the device (the generated steps before this launch): sub-counters sub0 + *sub_base * max(k, 1) + iteration
extern "C" int mnn_rbm_gibbs_multi_at(mnn_stream_t s, int njobs, const mnn_rbm_gibbs_job* jobs, int N, int D, int Hn, int k, int ld_bh, int ld_bv,
                                      uint32_t row0, const uint32_t* row_ids, uint32_t sub0, const int* seed_step, long row_stride, int elem_stride,
                                      long given_row_stride, void* workspace, const float* temps, const uint32_t* sub_base) {
    const char* who = sub_base != nullptr ? "mnn_rbm_gibbs_multi_at" : temps != nullptr ? "mnn_rbm_gibbs_multi_temps" : "mnn_rbm_gibbs_multi";
    MNN_REQUIRE(njobs > 0 && njobs <= RBM_MULTI_MAX_JOBS && jobs, "%s: 1..%d jobs", who, RBM_MULTI_MAX_JOBS);
    MNN_REQUIRE(elem_stride >= 1 && (row_stride >= (long)(D - 1) * elem_stride + 1 || N == 1), "%s: bad strides (row %ld, element %d)", who, row_stride,
                elem_stride);
    MNN_REQUIRE(jobs[0].given == nullptr || given_row_stride >= (long)(D - 1) * elem_stride + 1 || N == 1, "%s: given row stride %ld", who, given_row_stride);
    bool tempered = false;
    for (int j = 0; j < njobs && temps != nullptr; ++j) {
        MNN_REQUIRE(temps[j] > 0.f && temps[j] <= 3.0e38f, "%s: job %d: the temperature is a positive finite number (%g)", who, j, (double)temps[j]);
        tempered = tempered || temps[j] != 1.0f;
    }
    auto run = [&](auto A) {
        memset(&A, 0, sizeof(A));
        for (int j = 0; j < njobs; ++j) {
            const mnn_rbm_gibbs_job& q = jobs[j];
            A.job[j] = GibbsJob{q.W, nullptr, q.bh, q.bv, q.seed, q.v0, q.p_v, q.v_out, q.given};
            A.temp[j] = tempered ? temps[j] : 1.0f;
        }
        A.njobs = njobs; A.N = N; A.D = D; A.Hn = Hn; A.k = k; A.ld_bh = ld_bh; A.ld_bv = ld_bv;
        A.row0 = row0; A.row_ids = row_ids; A.sub0 = sub0; A.seed_step = seed_step; A.sub_base = sub_base; A.sub_scale = (uint32_t)(k > 1 ? k : 1);
        A.rs_given = given_row_stride; A.rs = row_stride; A.es = elem_stride;
        return rbm_gibbs_dispatch(who, s, A, workspace);
    };
    return tempered ? run(GibbsTableArgs<true>()) : run(GibbsTableArgs<false>());
}

extern "C" int mnn_rbm_gibbs_multi_temps(mnn_stream_t s, int njobs, const mnn_rbm_gibbs_job* jobs, int N, int D, int Hn, int k, int ld_bh, int ld_bv,
                                         uint32_t row0, const uint32_t* row_ids, uint32_t sub0, const int* seed_step, long row_stride, int elem_stride,
                                         long given_row_stride, void* workspace, const float* temps) {
    return mnn_rbm_gibbs_multi_at(s, njobs, jobs, N, D, Hn, k, ld_bh, ld_bv, row0, row_ids, sub0, seed_step, row_stride, elem_stride, given_row_stride,
                                  workspace, temps, nullptr);
}

extern "C" int mnn_rbm_gibbs_multi(mnn_stream_t s, int njobs, const mnn_rbm_gibbs_job* jobs, int N, int D, int Hn, int k, int ld_bh, int ld_bv,
                                   uint32_t row0, const uint32_t* row_ids, uint32_t sub0, const int* seed_step, long row_stride, int elem_stride,
                                   long given_row_stride, void* workspace) {
    return mnn_rbm_gibbs_multi_temps(s, njobs, jobs, N, D, Hn, k, ld_bh, ld_bv, row0, row_ids, sub0, seed_step, row_stride, elem_stride,
                                     given_row_stride, workspace, nullptr);
}

// ----------------------------------------------------------------------------------------------
// free energy (and optional hidden activations) of every job's rows in one launch, job = blockIdx.y; mnn_rbm_free_energy is its one-job call
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
