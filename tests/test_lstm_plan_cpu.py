"""LstmStack.plan: the one decision of a forward (which recurrence form runs; on the row-parallel path, each layer's forward and backward
kernel).  No library and no device: the stack stands on a stub rnn / store, and the library's shape predicates are replaced by their rules
for a 256-CU device.  The table below is written out by hand from the conditions of the dispatch the plan replaced."""
import ast
import inspect
import types

import pytest
import torch

from multinn_amd import ops
from multinn_amd.lstm_stack import LstmStack, Plan

CUS = 256
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
CR = ("cluster", "resident")


def _rowpar_ok(B, u):
    """Units 128 / 256 / 512, whole 32-row tiles, at most 4 row tiles per workgroup (3 for the backward of 512 units: both directions must fit)."""
    if u not in (128, 256, 512) or B <= 0 or B % 32:
        return False
    nrt = B // 32
    G = min(CUS // (u // 32), nrt)
    return -(-nrt // G) <= (3 if u == 512 else 4)


@pytest.fixture
def lib_rules(monkeypatch):
    """The shape rules of the library's predicates; `bwd_ok` is the XCD-placement answer of the cluster backward."""
    rules = types.SimpleNamespace(bwd_ok=True)
    cluster_ok = lambda B, u: u == 512 and B > 0 and B % 256 == 0 and (B // 32) * 8 <= CUS
    monkeypatch.setattr(ops, "lstm2_persist_ok", lambda B, u1, u2: B > 0 and all(u in (128, 256, 512) for u in (u1, u2)))
    monkeypatch.setattr(ops, "lstm_rowpar_ok", _rowpar_ok)
    monkeypatch.setattr(ops, "lstm_resident_ok", lambda B, u: u == 256 and B > 0 and B % 4 == 0)
    monkeypatch.setattr(ops, "lstm_cluster_ok", cluster_ok)
    monkeypatch.setattr(ops, "lstm_cluster_bwd_ok", lambda B, u: cluster_ok(B, u) and rules.bwd_ok)
    monkeypatch.setattr(ops, "lstm_fused_outputs", lambda dtype, u: dtype == BF16 and u in (128, 256, 512))
    monkeypatch.setattr(LstmStack, "_cluster_bwd_warned", True, raising=False)      # (the fall-back's one warning is not this test's subject)
    return rules


DEFAULTS = dict(persistent=True, fused_layers=True, rowpar=True, rowpar_min_batch=512, rowpar_xproj_f32=False, resident=True, cluster=True,
                merge_wgrads=True, group_rowpar=False, persist_single_step=True)


def make(dtype, units=(512, 256), **switches):
    rnn = types.SimpleNamespace(n_in=88, num_units=list(units), prefix="rnn")
    st = LstmStack(rnn, None, dtype)
    for k, v in {**DEFAULTS, **switches}.items():       # on the instance: independent of the MULTINN_* variables of the environment
        assert hasattr(LstmStack, k)
        setattr(st, k, v)
    st.packed, n_in = [], 88
    for l, u in enumerate(units):
        p = dict(u=u, ld=st.ld0 if l == 0 else n_in, n_in=n_in)
        if st.h16:
            p["wx_gm"] = object()
        st.packed.append(p)
        n_in = u
    return st


RP = lambda fwd, bwd=None, merged=True: Plan("rowpar", fwd, fwd if bwd is None else bwd, merged)
S0, SG = dict(state0=True), dict(state0=True, state_grad=True)

# (dtype, switches, bwd_ok, B, T, plan arguments, expected)
TABLE = [
    (F32, {}, True, 1024, 8, {}, Plan("seq")),                                      # f32: neither 16-bit form, no two-layer bf16 launches
    (F32, {}, True, 256, 8, {}, Plan("seq")),
    (F16, {}, True, 1024, 8, {}, RP(CR)),
    (BF16, {}, True, 1024, 8, {}, RP(CR)),
    (F16, {}, True, 1024, 8, dict(save=False), RP(CR, merged=False)),
    (F16, dict(merge_wgrads=False), True, 1024, 8, {}, RP(CR, merged=False)),
    (F16, {}, True, 1024, 8, S0, RP(CR)),                                           # every kernel takes a state: the row-parallel path stays
    (F16, {}, True, 1024, 8, SG, RP(CR)),
    (F16, {}, False, 1024, 8, {}, RP(CR, ("rowpar", "resident"))),                  # clusters not on single XCDs: that layer's backward falls back
    (F16, {}, False, 1024, 8, S0, Plan("persist")),                                 # ... which takes no state: the whole plan leaves the path
    (F16, {}, False, 1024, 8, SG, Plan("seq")),
    (BF16, {}, False, 1024, 8, SG, Plan("seq")),                                    # (768 blocks per launch: above the two-layer form's 512)
    (F16, {}, True, 1024, 3, {}, RP(CR, ("rowpar", "resident"))),                   # the cluster backward needs T >= 4
    (F16, {}, True, 1024, 3, S0, Plan("persist")),
    (F16, {}, True, 1024, 3, SG, Plan("seq")),
    (F16, {}, True, 1024, 4, S0, RP(CR)),
    (F16, {}, True, 256, 8, {}, Plan("persist")),                                   # below rowpar_min_batch
    (F16, dict(group_rowpar=True), True, 256, 8, {}, RP(CR)),
    (F16, dict(rowpar_min_batch=32), True, 64, 8, {}, RP(("rowpar", "resident"))),  # B % 256 != 0: no cluster form
    (F16, {}, True, 256, 8, S0, Plan("persist")),                                   # the persistent form has a state input ...
    (F16, {}, True, 256, 8, SG, Plan("seq")),                                       # ... but no state gradient
    (BF16, {}, True, 256, 8, SG, Plan("fused2")),
    (F16, {}, True, 256, 8, dict(state0=True, state_grad=True, save=False), Plan("persist")),
    (F16, {}, True, 256, 8, dict(state_grad=True), Plan("persist")),
    (F16, dict(persist_single_step=False), True, 256, 1, S0, Plan("seq")),
    (BF16, dict(persist_single_step=False), True, 256, 1, S0, Plan("fused2")),
    (F16, {}, True, 256, 1, S0, Plan("persist")),
    (F16, {}, True, 1024, 1, {}, Plan("persist")),                                  # one step: never the row-parallel path
    (F16, dict(rowpar_xproj_f32=True), True, 1024, 8, {}, RP(("rowpar", "rowpar"))),
    (F16, dict(rowpar_xproj_f32=True), True, 1024, 8, S0, Plan("persist")),
    (F16, {}, True, 1000, 8, {}, Plan("persist")),                                  # not a multiple of the 32-row tile
    (F16, {}, True, 2048, 8, {}, Plan("persist")),                                  # four row tiles per workgroup of the 512-unit backward
    (F16, {}, True, 1024, 512, {}, RP(("rowpar", "resident"))),                     # layer 1's saved gates pass 2 GB: no cluster form
    (F16, dict(persistent=False), True, 1024, 8, {}, RP(CR)),
    (F16, dict(persistent=False), True, 256, 8, {}, Plan("seq")),
    (BF16, dict(persistent=False), True, 256, 8, {}, Plan("fused2")),
    (BF16, dict(persistent=False, fused_layers=False), True, 256, 8, {}, Plan("seq")),
    (BF16, dict(persistent=False), True, 1024, 8, dict(state0=True), RP(CR)),
    (F16, dict(rowpar=False), True, 1024, 8, {}, Plan("persist")),
    (BF16, dict(rowpar=False, persistent=False), True, 1024, 8, {}, Plan("seq")),
    (BF16, dict(rowpar=False, persistent=False), True, 672, 8, {}, Plan("fused2")),  # 24 * 21 = 504 blocks
    (BF16, dict(rowpar=False, persistent=False), True, 673, 8, {}, Plan("seq")),     # 24 * 22 = 528
    (F16, dict(resident=False), True, 1024, 8, {}, RP(("cluster", "rowpar"))),
    (F16, dict(resident=False), True, 1024, 8, S0, Plan("persist")),
    (F16, dict(cluster=False), True, 1024, 8, {}, RP(("rowpar", "resident"))),
    (F16, dict(cluster=False), True, 1024, 8, S0, Plan("persist")),
    (F16, dict(units=(256,)), True, 1024, 8, SG, RP(("resident",))),                # one layer: no two-layer form
    (F16, dict(units=(256,)), True, 256, 8, {}, Plan("seq")),
    (BF16, dict(units=(256,)), True, 256, 8, {}, Plan("seq")),
    (BF16, dict(units=(128, 128)), True, 6, 9, {}, Plan("persist")),
    (BF16, dict(units=(128, 128), persistent=False), True, 6, 9, {}, Plan("fused2")),
]


@pytest.mark.parametrize("i", range(len(TABLE)))
def test_plan_table(i, lib_rules):
    dtype, switches, bwd_ok, B, T, args, want = TABLE[i]
    lib_rules.bwd_ok = bwd_ok
    st = make(dtype, **switches)
    got = st.plan(B, T, **args)
    assert isinstance(got, Plan) and got == want, (TABLE[i][:6], got)
    if got.path == "rowpar":
        assert len(got.fwd) == len(got.bwd) == len(st.packed)
    else:
        assert got.fwd == got.bwd == () and not got.merged
    with pytest.raises(AttributeError):
        got.path = "seq"                                 # immutable


def test_predicates_agree_with_the_plan(lib_rules):
    st = make(F16)
    assert st._rowpar(1024, 8) and not st._rowpar(1024, 8, state0=[None]) and not st._rowpar(1024, 1) and not st._rowpar(256, 8)
    assert st._rowpar_state0(1024, 8) and not st._rowpar_state0(1024, 3) and not st._rowpar_state0(256, 8)
    assert st._persist(256) and st._persist(1024, 8) and not st._fused2(256) and make(BF16)._fused2(256)
    assert st._cluster(0, 1024, 8) and st._cluster_bwd(0, 1024, 8) and not st._cluster_bwd(0, 1024, 3) and not st._cluster(1, 1024, 8)
    assert st._resident(1, 1024, 8) and not st._resident(0, 1024, 8)
    lib_rules.bwd_ok = False
    assert st._cluster(0, 1024, 8) and not st._cluster_bwd(0, 1024, 8) and not st._rowpar_state0(1024, 8) and st._rowpar(1024, 8)


def test_cluster_backward_fallback_is_said_once(lib_rules, monkeypatch):
    monkeypatch.setattr(LstmStack, "_cluster_bwd_warned", False, raising=False)
    lib_rules.bwd_ok = False
    st = make(F16)
    with pytest.warns(UserWarning, match="lstm_rowpar_bwd"):
        st.plan(1024, 8)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert st.plan(1024, 8).bwd == ("rowpar", "resident")


SIGNATURES = {
    "forward": "(self, x_tm, keep_prob=1.0, seed=0, row0=0, save=True, state0=None, step_dev=None, state_grad=False)",
    "forward_co": "(self, x_tm, keep_prob=1.0, seed=0, row0=0, save=True, state0=None, step_dev=None, state_grad=False)",
    "backward": "(self, dy, ctx, keep_prob=1.0, seed=0, row0=0, need_dx=False, step_dev=None, need_dstate=False)",
    "backward_co": "(self, dy, ctx, keep_prob=1.0, seed=0, row0=0, need_dx=False, step_dev=None, need_dstate=False)",
    "input_T": "(self, T, B, dev)",
    "single_step": "(self, x, state)",
    "_rowpar": "(self, B, T=2, state0=None)",
    "_rowpar_state0": "(self, B, T=2)",
    "_persist": "(self, B, T=2)",
    "_fused2": "(self, B=0)",
    "_resident": "(self, l, B, T)",
    "_cluster": "(self, l, B, T)",
    "_cluster_bwd": "(self, l, B, T)",
    "plan": "(self, B, T, state0=False, state_grad=False, save=True)",
}


def test_public_surface():
    for name, sig in SIGNATURES.items():
        assert str(inspect.signature(getattr(LstmStack, name))) == sig, name
    assert inspect.isgeneratorfunction(LstmStack.forward_co) and inspect.isgeneratorfunction(LstmStack.backward_co)
    assert not any(n.startswith("pipe") or n in ("chunk", "_lanes", "_chunks") for n in dir(LstmStack))     # the stream wavefront is gone
    assert not hasattr(LstmStack, "_forward_rowpar") and not hasattr(LstmStack, "_backward_rowpar")
    # the old import paths keep working: generators re-exports the moved names, the new module does not import generators
    from multinn_amd import generators, lstm_stack
    for name in ("LstmStack", "drive", "drive_group", "det_steps", "_SINGLE", "_det_f32"):
        assert getattr(generators, name) is getattr(lstm_stack, name)
    imports = [n for n in ast.walk(ast.parse(inspect.getsource(lstm_stack))) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert not any("generators" in ast.dump(n) for n in imports)
