"""The environment switches of the Python side: every MULTINN_* variable is declared here, once, and read through flag() / value().

Both read os.environ at the moment of the call.  A class attribute such as `LstmStack.cluster = flag("MULTINN_CLUSTER")` is therefore
evaluated at import (tests and bench.py set such attributes directly), a call inside a function on every call (tests flip
MULTINN_GENERATE_GRAPH, MULTINN_TRAIN_GRAPH, MULTINN_COMM and MULTINN_DP_REHEARSAL with monkeypatch.setenv).  The C library's
MNN_* switches are declared in csrc/host_support.h; README.md lists both tables and tests/test_switches_cpu.py keeps it true.
"""
import os
from collections import namedtuple

Switch = namedtuple("Switch", "name default kind meaning")      # kind: "bool" | "int" | "float" | "str" | "path"

SWITCHES = {s.name: s for s in (
    # recurrence (lstm_stack.py)
    Switch("MULTINN_PERSIST", True, "bool", "=0: launch-per-timestep recurrence instead of the persistent kernels"),
    Switch("MULTINN_ROWPAR", True, "bool", "=0: the two-layer persistent recurrence at every batch size instead of the row-parallel form"),
    Switch("MULTINN_ROWPAR_MIN_BATCH", 512, "int", "sequences per GPU from which the row-parallel recurrence is used"),
    Switch("MULTINN_ROWPAR_XPROJ", "16", "str", "=f32: f32 input projections for the row-parallel recurrence (default: the 16-bit compute type)"),
    Switch("MULTINN_RESIDENT", True, "bool", "=0: row-parallel kernels for 256-unit layers too instead of the CU-resident recurrence"),
    Switch("MULTINN_CLUSTER", True, "bool", "=0: row-parallel kernels for the 512-unit layer instead of the cluster form"),
    Switch("MULTINN_MERGE_WGRADS", True, "bool", "=0: separate dWx / dWh GEMMs instead of one GEMM per layer over [x^T ; h^T]"),
    Switch("MULTINN_KBLOCK_WGRADS", True, "bool", "=0: plain dz^T [4u, N] instead of the K-blocked layout [N/32][4u][32]"),
    # generators (generators.py, modes.py)
    Switch("MULTINN_DET_SAMPLING", True, "bool", "=0: sampling scans on the throughput kernels instead of the deterministic f32 steps"),
    Switch("MULTINN_NADE_MFMA", True, "bool", "=0: f32 NADE forward instead of the matrix-core form"),
    Switch("MULTINN_NADE_DENSE_ABOVE", 0.07, "float", "input density above which the NADE forward takes the f32 form (decided on the device)"),
    Switch("MULTINN_NADE_EXACT_MFMA", True, "bool", "=0: f32 vector NADE forward in fp16 mode instead of the split-operand matrix-core form"),
    Switch("MULTINN_RAGGED_COMPACT", True, "bool", "=0: ragged windows keep their padding rows (weight 0) in the Dense + NADE part"),
    Switch("MULTINN_RAGGED_GEMM_ROWS", True, "bool", "=0: the Dense GEMMs of a compacted ragged window run over its padding rows too"),
    Switch("MULTINN_JAMMING_GROUP", True, "bool", "=0: the jamming generators one after the other instead of in lockstep"),
    # read on every call
    Switch("MULTINN_GENERATE_GRAPH", True, "bool", "=0: eager sampling loop instead of one hipGraph replay per generate()"),
    Switch("MULTINN_TRAIN_GRAPH", True, "bool", "=0: driver.train_epoch launches every step eagerly instead of replaying a captured step"),
    Switch("MULTINN_COMM", "", "str", "=capi: the data-parallel all-reduce through the library's own mnn_allreduce_flat instead of torch.distributed"),
    Switch("MULTINN_DP_REHEARSAL", False, "bool", "=1: one-rank rehearsal of the data-parallel step"),
    # paths, not switches: read where they are needed (_lib.py, which must load before anything else; build.py reads HIPCC)
    Switch("MULTINN_HIP_LIB", None, "path", "another build of the same C ABI to load (A/B runs)"),
)}


def value(name):
    """The variable's value in its declared kind, or its default when it is not set."""
    s = SWITCHES[name]
    raw = os.environ.get(name)
    if raw is None:
        return s.default
    if s.kind == "bool":                  # a default-on switch is turned off by "0" alone, a default-off one turned on by "1" alone
        return raw != "0" if s.default else raw == "1"
    return {"int": int, "float": float}.get(s.kind, str)(raw)


def flag(name):
    assert SWITCHES[name].kind == "bool", name
    return value(name)
