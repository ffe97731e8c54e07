// The cross-workgroup hand-off of the persistent LSTM recurrences (gfx950): THE description of the protocol and the one definition of each
// of its pieces.  lstm_persist.hip (two layers, a workgroup per item), lstm_rowpar.hip (a wave per row tile) and lstm_cluster.hip (eight
// workgroups per row tile) hand state tiles to each other through global memory with it; lstm_resident.hip hands nothing between workgroups
// and uses only the counted wait, the LDS-only barrier and the LDS-DMA forms.  It is the one part of the library that can hang a device
// rather than return wrong numbers, so a change to the spin, the give-up rule or the store policy is made HERE, once.
//
// 1. Producer.  The storing waves write the tile (h[t], dz[t], partial sums) into the exchange area with 16-byte stores, write-through at
//    device scope (aux bit HF_SC1) -> EVERY storing wave waits for its own stores (`s_waitcnt vmcnt(0)`, or the counted hf_wait_all_but(N)
//    of 5.) -> where one lane signals for several waves, a workgroup barrier (pst_publish; in the row-parallel and cluster forms each
//    wave signals for itself and needs none) -> ONE lane stores the progress flag, device scope (hf_raise).  Flags only grow: the value is
//    the number of steps handed on.  (cdna_hip_programming.md G16 R1; MI355X_MICROARCH.md "Valid forms", first table row.)
// 2. Consumer.  ONE wave polls the 128-byte flag line of its row tile with relaxed agent-scope (sc1, L1-bypassing) loads, one flag per lane
//    (hf_wait; pst_wait for the two-threshold form of lstm_persist.hip), and only when every flag has reached the step does it -- and,
//    behind a workgroup barrier or an LDS word that wave then sets, the other waves -- issue the loads of the tile, every one of them an sc1
//    buffer load or an sc1 LDS-DMA (hf_dma16_sc1): no load of handed-off bytes goes through the L1, so no acquire is needed.
// 3. XCD probe.  At launch start every member of a row-tile group posts 0x100 | XCC_ID and one wave compares (hf_probe_xcd).  When all sit on
//    ONE XCD, tile and flag may be stored write-BACK (`local`: plain stores, hf_store_frag / hf_raise): they stay in that XCD's L2, which is
//    the level the consumers' sc1 loads are served from, so the consumer sees exactly the bytes it would have seen written through, only
//    sooner.  The probe therefore selects a store policy and nothing else: the values, their order and what is waited for are the same on
//    both paths, and results never depend on it.  (MNN_PERSIST_NO_LOCAL forces write-through; a form whose exchange area is only valid
//    on one XCD -- the cluster backward -- asks the host-side placement probe before it runs at all.)
// 4. Give-up.  Every spin is bounded (HF_LIMIT: 1 s of the 100 MHz wall clock) and the lanes that poll no flag watch the launch's status word.
//    A wave that runs out of time, or sees the status word set, sets the status word AND the sticky word (hf_give_up) and leaves; every other
//    waiter leaves at its next poll, so the grid always drains.  The status word is re-zeroed by the next launch, the sticky word never:
//    the host reads it (mnn_lstm_*_status) and knows that some launch on this workspace gave up and its outputs are not to be used.
// 5. Counted wait.  Loads, stores, atomics and LDS-DMA of one wave complete in issue order (MI355X_MICROARCH.md, cycle constants), and vmcnt
//    counts the ones outstanding.  So `s_waitcnt vmcnt(N)` with N the number of vector-memory operations issued BEHIND the hand-off stores
//    proves the hand-off stores complete while the younger ones (row-major outputs, next step's prefetch) stay in flight.  The count must
//    be exact: RP_HANDOFF_FENCE (lstm_rowpar.hip) keeps the compiler from moving an operation across the hand-off, and
//    tests/test_build_guards.py counts the operations in the compiler's output.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------- sync words (device and host)
// The sync area of a workspace, in 32-bit words: [HF_STATUS_WORD] status (non-zero: the launch is aborting), [HF_STICKY_WORD] sticky give-up,
// flag lines of 32 words from HF_FLAGS_OFF on (one per row tile, then one XCC-id line per row-tile group).  lstm_persist.hip keeps its sticky
// word at its own `sticky_off` BEHIND its edge slabs, because its launches zero the whole sync area with one memset: a layout difference,
// not a copy -- it passes that offset where the others take the default.
#define HF_STATUS_WORD 0
#define HF_STICKY_WORD 1
#define HF_FLAGS_OFF 32
#define HF_LIMIT 100000000LL       // spin bound: 1 s of wall_clock64() (100 MHz)
#define HF_SC1 16                  // aux bit of raw buffer loads/stores: device scope (write-through / L1-bypassing)

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned hf_gu32;
typedef __attribute__((address_space(3))) void* hf_lptr_t;

// ---------------------------------------------------------------------------------------------- device part
__device__ __forceinline__ unsigned hf_ld(const unsigned* p) { return __hip_atomic_load((hf_gu32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void hf_st(unsigned* p, unsigned v) { __hip_atomic_store((hf_gu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned hf_xcc_id() {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return xcc;
}
// one lane: the launch is aborting, and the workspace remembers it (`sticky`: word offset from `status`, never re-zeroed by a launch)
__device__ __forceinline__ void hf_give_up(unsigned* status, int sticky = HF_STICKY_WORD - HF_STATUS_WORD) {
    hf_st(status, 1u);
    hf_st(status + sticky, 1u);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t hf_rsrc(const void* base, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
// fragment f of an exchange slab ([k-step][lane][16 B]: one contiguous KiB per instruction).  `local`: see 3. above
__device__ __forceinline__ void hf_store_frag(const __amdgpu_buffer_rsrc_t rs, int f, int lane, u32x4_t v, bool local) {
    if (local) __builtin_amdgcn_raw_buffer_store_b128(v, rs, (f * 64 + lane) * 16, 0, 0);
    else __builtin_amdgcn_raw_buffer_store_b128(v, rs, (f * 64 + lane) * 16, 0, HF_SC1);
}
__device__ __forceinline__ void hf_raise(unsigned* flag, unsigned value, bool local) {        // one lane, after the storing waves' vmcnt wait
    if (local) __hip_atomic_store((hf_gu32*)flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // plain store: lands in the shared L2
    else hf_st(flag, value);
}

// One wave waits until the first n (<= 32) words of `line` are all >= need; the other lanes watch the status word.  false: the launch is aborting.
__device__ __forceinline__ bool hf_wait(const unsigned* line, unsigned* status, int n, unsigned need) {
    const int lane = threadIdx.x & 63;
    const bool mine = lane < n;
    const unsigned* p = mine ? line + lane : status;
    const long long t0 = wall_clock64();
    for (unsigned spins = 1;; ++spins) {
        const unsigned v = hf_ld(p);
        if (__all(mine ? v >= need : v == 0u)) return true;
        const bool dead = __any(!mine && v != 0u) || ((spins & 127u) == 0u && wall_clock64() - t0 > HF_LIMIT);
        if (dead) {
            if (lane == 0) hf_give_up(status);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Launch start: do the nb members (workgroups) of this row-tile group share an XCD?  Each posts 0x100 | XCC_ID (device scope) into its word of
// `xline`, wave 0 waits for the others (bounded) and compares; the answer reaches the other waves through LDS at the caller's next barrier.
__device__ __forceinline__ void hf_probe_xcd(unsigned* xline, unsigned* status, int member, int nb, int* s_local) {
    const unsigned xcc = hf_xcc_id();
    if (threadIdx.x == 0) hf_st(xline + member, 0x100u | (xcc & 0xfu));
    if (threadIdx.x < 64) {
        bool same = false;
        if (hf_wait(xline, status, nb, 1u)) {
            const unsigned v = hf_ld(xline + (threadIdx.x < (unsigned)nb ? threadIdx.x : 0));
            same = __all(v == __builtin_amdgcn_readfirstlane(v));
        }
        if (threadIdx.x == 0) *s_local = same ? 1 : 0;
    }
}

// `s_waitcnt vmcnt(n)`: everything but the n youngest vector-memory operations of this wave is complete (5. above).  n is a run-time count in
// the row-parallel kernels and a compile-time constant elsewhere (the switch folds); above 48 it waits for everything.
#define HF_VMC(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
__device__ __forceinline__ void hf_wait_all_but(int n) {
    switch (n) {
        HF_VMC(0) HF_VMC(1) HF_VMC(2) HF_VMC(3) HF_VMC(4) HF_VMC(5) HF_VMC(6) HF_VMC(7) HF_VMC(8) HF_VMC(9) HF_VMC(10) HF_VMC(11) HF_VMC(12)
        HF_VMC(13) HF_VMC(14) HF_VMC(15) HF_VMC(16) HF_VMC(17) HF_VMC(18) HF_VMC(19) HF_VMC(20) HF_VMC(21) HF_VMC(22) HF_VMC(23) HF_VMC(24)
        HF_VMC(25) HF_VMC(26) HF_VMC(27) HF_VMC(28) HF_VMC(29) HF_VMC(30) HF_VMC(31) HF_VMC(32) HF_VMC(33) HF_VMC(34) HF_VMC(35) HF_VMC(36)
        HF_VMC(37) HF_VMC(38) HF_VMC(39) HF_VMC(40) HF_VMC(41) HF_VMC(42) HF_VMC(43) HF_VMC(44) HF_VMC(45) HF_VMC(46) HF_VMC(47) HF_VMC(48)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// Workgroup barrier that waits for this wave's LDS traffic only: __syncthreads() also drains vmcnt(0), which would make every barrier of a
// step wait for the prefetch loads, LDS-DMA and deferred stores issued just before it (HBM latency on the chain of every step).
__device__ __forceinline__ void hf_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS-DMA (global -> LDS without registers) in inline assembly: behind __builtin_amdgcn_global_load_lds the compiler puts `s_waitcnt vmcnt(0)` in
// front of every LDS read that may alias its destination, i.e. the whole memory latency on the chain of every step.  The caller waits for its
// own DMA (hf_wait_all_but) one barrier ahead of the reads.  The sc1 form bypasses the L1: it is the consumer load of a hand-off (2. above).
__device__ __forceinline__ void hf_dma16(const void* g, const void* l) {
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"((unsigned)(uintptr_t)(hf_lptr_t)const_cast<void*>(l)), "v"(g) : "memory", "m0");
}
__device__ __forceinline__ void hf_dma16_sc1(const void* g, const void* l) {
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off sc1" :: "s"((unsigned)(uintptr_t)(hf_lptr_t)const_cast<void*>(l)), "v"(g) : "memory", "m0");
}
__device__ __forceinline__ void hf_dma4(const void* g, const void* l) {
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dword %1, off" :: "s"((unsigned)(uintptr_t)(hf_lptr_t)const_cast<void*>(l)), "v"(g) : "memory", "m0");
}

// ---------------------------------------------------------------------------------------------- host part
// The workspace that the row-parallel and the cluster form share: [sync words | zero edge slabs (h[-1], dz[T]) | exchange slabs from rp_xchg_off],
// and the per-launch reset of its sync words (everything but the sticky word back to zero).  Defined in lstm_rowpar.hip -- the library is
// built without relocatable device code, so the kernel lives in one translation unit and the other form launches it through mnn_rp_reset_launch.
size_t rp_sync_bytes(int nrt);                      // flag lines, then one XCC-id line per row-tile group
size_t rp_edge_bytes(int nrt, int U);
size_t rp_xchg_off(int nrt, int U);
__global__ void rp_reset_kernel(unsigned* sync, int words);
void mnn_rp_workspace_layout(int nrt, int U, size_t* sync_bytes, size_t* xchg_off);
int mnn_rp_reset_launch(hipStream_t st, void* workspace, int nrt);
