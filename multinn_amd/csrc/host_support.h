// Host-only launch support shared by every kernel family: the current device's index, per-device "done once" bookkeeping, the
// dynamic-LDS raise, the CU count, and the one table of development / test switches.  The non-inline parts live in elementwise.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

// ----------------------------------------------------------------------------------------------
// per-device state.  Things like hipFuncSetAttribute hold PER DEVICE (a process-wide flag would leave the second device of a process
// at the default dynamic-LDS limit), so every "done once" table is indexed by the current device's ordinal.
// ----------------------------------------------------------------------------------------------
#define MNN_MAX_DEVICES 64

// The one place that asks for the current device.  An ordinal outside [0, MNN_MAX_DEVICES) is hipErrorInvalidDevice for every caller:
// nothing aliases it to another device's slot and nothing skips its work silently.
hipError_t mnn_current_device(int* dev);

// compute units of the current device (cached per device); 0 on failure
int mnn_cu_count();

static inline hipError_t mnn_raise_dynamic_lds(const void* kernel, int bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// `f` runs once per device: the current device's flag is set only when f returned hipSuccess (a failure is reported and tried again by
// the next call).  The static MnnPerDeviceOnce stays at the call site, so every kernel family raises its own kernels.
struct MnnPerDeviceOnce { bool done[MNN_MAX_DEVICES]; };
template <class F>
static inline hipError_t mnn_once_per_device(MnnPerDeviceOnce& once, F&& f) {
    int dev = 0;
    hipError_t e = mnn_current_device(&dev);
    if (e != hipSuccess || once.done[dev]) return e;
    e = std::forward<F>(f)();
    if (e == hipSuccess) once.done[dev] = true;
    return e;
}

// ----------------------------------------------------------------------------------------------
// Development / test switches (environment variables): every one is declared here, once, and read through mnn_switch_set /
// mnn_switch_int -- the only getenv in the library.  A switch is read on EVERY call (tests flip them inside one process); that is one
// getenv per eager launch, on host paths that a captured step never re-executes.  README.md lists the same names.
// ----------------------------------------------------------------------------------------------
#define MNN_SWITCHES(X)                                                                                                                   \
    X(GEMM_BRES,          "=0: the LDS-staged GEMM kernels for the input projections instead of the weight-resident form")                \
    X(GEMM_BRES_VAR,      "ablation builds (BR_ABLATION) only: the weight-resident GEMM's kernel variant")                                \
    X(GEMM_NO256,         "set: 128 x 128 GEMM tiles only")                                                                               \
    X(GEMM_F32_KH,        "=0: four waves per f32 GEMM tile instead of eight with the in-workgroup K split")                              \
    X(GEMM_SPLITK_MAP,    "=0|1: forces the split-K workgroup mapping (default: by slice count)")                                         \
    X(PERSIST_NO_LOCAL,   "set: write-through hand-offs even when a row tile's workgroups share an XCD")                                  \
    X(PERSIST_TEST_ABORT, "set: test hook, a persistent launch gives up")                                                                 \
    X(ROWPAR_MAX_G,       "=n: test hook, at most n row-tile groups (several row tiles per workgroup at small batch)")                    \
    X(ROWPAR_NO_PAIR,     "set: one wave per (row tile, unit tile) item in the row-parallel recurrence instead of a wave pair")           \
    X(NADE_FWD_NO_UT,     "set: the dense NADE forward with direct sigmoids instead of multiplicatively advanced states")                 \
    X(SAMPLE_NO_CHUNK,    "set: the NADE sampling kernel of one visible per pass instead of the chunked one")                             \
    X(SAMPLE_G8,          "set: eight visibles per pass in the chunked NADE sampling kernel at small batch too (default there: sixteen)") \
    X(SAMPLE_NO_SPEC,     "set: the NADE sampling kernel without the speculative next-visible dot product")                               \
    X(RBM_STREAM_W,       "set: Gibbs chain with W streamed from L2 instead of resident in LDS")                                          \
    X(RBM_NO_MFMA,        "set: vector kernels for the Gibbs chain, AIS and the half-steps of training batches")

enum MnnSwitch {
#define X(name, meaning) MNN_SW_##name,
    MNN_SWITCHES(X)
#undef X
    MNN_SW_COUNT
};

bool mnn_switch_set(MnnSwitch sw);                  // the variable MNN_<name> exists (whatever its value)
int mnn_switch_int(MnnSwitch sw, int dflt);         // its value as an integer; dflt when it does not exist

// the persistent recurrences may hand off through an XCD's own L2: one reader for the _ok queries and the launches, so they cannot disagree
static inline bool mnn_persist_allow_local() { return !mnn_switch_set(MNN_SW_PERSIST_NO_LOCAL); }
