"""Every form of the two-layer persistent recurrence (csrc/lstm_persist.hip), element by element against float64.

`lstm2_persist_fwd_kernel` / `lstm2_persist_bwd_kernel` are instantiated 18 times each (U1 x U2 over {128, 256, 512}^2, f16 | bf16).  Each case
below calls ops.lstm2_persist_fwd / ops.lstm2_persist_bwd directly on descriptors of ops.lstm2_fwd_layer / ops.lstm2_bwd_layer and compares every
output of both layers with tests/lstm2_float64.py -- tests/lstm_float64.py layer by layer on the kernel's own 16-bit operands and hand-offs.  The
16-bit outputs take the bounds of test_gpu_rowpar_kernels.py unchanged (units of eps = 2^-10 for f16, 2^-7 for bf16); `gates` and `c` are f32
in this form and get absolute bounds derived from their measured error (profiles/persist_kernel_tests.md).

A FORM is a rule for the batch size B, worked out at run time from the device's CU count through `plan`, a restatement of persist_plan:
    F1   32               one full row tile, one per workgroup, the fast tail only
    P6   6                one partial tile
    U33  33               two tiles, a one-row last tile, B % 8 != 0: no fast tail anywhere, unaligned transposed stores
    A72  72               B % 8 == 0 with a partial last tile: fast tail and predicated tail in one launch
    R2   32 nrt           two row tiles per workgroup in some workgroups and one in others (nrt = gmax + 1, or gmax + 2 where that is even:
                          with an even tile count every workgroup would own exactly two)
    R2p  32 nrt - 5       the same with a partial, unaligned last tile
    R3   32 (2 gmax + 1)  three row tiles per workgroup
test_case_table_covers_every_instantiation_and_option and test_checker_rejects_small_defects need no device."""
import collections
import json

import numpy as np
import pytest
import torch

import lstm2_float64 as L2_64
import lstm_float64 as L64

DEV = "cuda:0"
SENT = -768.0            # exactly representable in f16 / bf16 / f32 and outside the range of every output
DB0 = 0.5                # db_p is preloaded with this: the kernel adds to it atomically

UNITS = (128, 256, 512)
FORMS = ("F1", "P6", "U33", "A72", "R2", "R2p", "R3")
STATES = ("none", "both", "l1", "l2", "c0")     # which layers start from a given state: h0 and c0 of both / of one layer; c0 alone (both layers)

Case = collections.namedtuple("Case", "form u1 u2 dt T keep fold save hT yT pad state db nolocal bwd")


def C(form, u1, u2, dt, T, keep, fold=True, save=True, hT=True, yT=True, pad=0, state="none", db=True, nolocal=False, bwd=True):
    """fold: at keep < 1 layer 2's mask goes to the backward, which applies dh_ext / keep * mask itself (False: the caller hands the already dropped
    dh_ext and no mask); save = False: the inference variant (no gates, no transposed copies, no backward); pad: extra columns in the leading
    dimension of h^T, y^T and dz^T; db = False: no bias gradient."""
    if not save:
        hT = yT = bwd = False
    if keep >= 1.0 or not bwd:
        fold = False
    return Case(form, u1, u2, dt, T, keep, fold, save, hT, yT, pad, state, db and bwd, nolocal, bwd)


F, BF = "fp16", "bf16"
CASES = [
    C("F1", 128, 128, F, 2, 1.0),
    C("P6", 128, 256, F, 6, 0.9, yT=False, pad=8, state="both"),
    C("U33", 128, 512, F, 19, 0.9, fold=False, pad=24, state="l2", nolocal=True),
    C("A72", 256, 128, F, 6, 1.0, hT=False, state="c0"),
    C("R2", 256, 256, F, 2, 0.9, nolocal=True),
    C("R2p", 256, 512, F, 3, 1.0, pad=4, state="both"),
    C("A72", 512, 128, F, 19, 0.9, pad=8, db=False),
    C("R3", 512, 256, F, 2, 0.9, fold=False, state="c0"),
    C("U33", 512, 512, F, 6, 1.0, pad=24, state="l2"),
    C("R2p", 512, 512, F, 2, 0.9),
    C("U33", 128, 128, F, 1, 0.9, state="both"),                           # the sampling form with a backward
    C("P6", 256, 256, F, 1, 0.9, save=False, state="both"),                # the sampling step itself: forward only, nothing saved
    C("A72", 128, 512, F, 6, 1.0, save=False),
    C("R2", 512, 128, F, 3, 0.9, save=False, state="l1", nolocal=True),
    C("P6", 128, 128, BF, 6, 0.9, fold=False, pad=8, state="c0"),
    C("A72", 128, 256, BF, 19, 1.0, state="l2", nolocal=True),
    C("R2", 128, 512, BF, 3, 1.0, yT=False, pad=24),
    C("U33", 256, 128, BF, 2, 0.9, hT=False, state="both"),
    C("F1", 256, 256, BF, 19, 0.9, db=False),
    C("A72", 256, 512, BF, 6, 0.9, fold=False, pad=4, nolocal=True),
    C("R3", 512, 128, BF, 2, 1.0, state="l1"),
    C("U33", 512, 256, BF, 6, 0.9, pad=24, state="l2"),
    C("R2", 512, 512, BF, 2, 1.0, state="c0", nolocal=True),
    C("R2p", 128, 128, BF, 2, 0.9, fold=False),
    C("P6", 256, 128, BF, 1, 1.0, state="both"),
    C("F1", 512, 128, BF, 1, 1.0, save=False, state="both"),
    C("R2p", 256, 256, BF, 3, 0.9, save=False),
    C("U33", 512, 512, BF, 6, 0.9, save=False, state="c0"),
]


def case_id(c):
    opts = [c.form, f"u{c.u1}x{c.u2}", c.dt, f"T{c.T}", f"k{c.keep}"]
    opts += (["fold"] if c.fold else []) + ([] if c.save else ["nosave"])
    opts += [n for n, on in (("hT", c.hT), ("yT", c.yT)) if on] + ([f"pad{c.pad}"] if c.pad else [])
    opts += ([f"st-{c.state}"] if c.state != "none" else []) + ([] if c.db or not c.bwd else ["nodb"]) + (["nolocal"] if c.nolocal else [])
    return "-".join(opts)


def cdiv(a, b):
    return -(-a // b)


Plan = collections.namedtuple("Plan", "nm gmax nrt R G rvs")


def plan(B, u1, u2, cus):
    """persist_plan: nm workgroups per row-tile group, at most gmax groups resident, R row tiles per workgroup at the most, G groups; rvs: the
    set of row-tile counts Rv = ceil((nrt - grp) / G) the workgroups of one launch have."""
    nm = u1 // 32 + u2 // 32
    gmax = cus // nm
    nrt = cdiv(B, 32)
    R = cdiv(nrt, gmax)
    G = cdiv(nrt, R)
    return Plan(nm, gmax, nrt, R, G, frozenset(cdiv(nrt - grp, G) for grp in range(G)))


def form_batch(form, u1, u2, cus):
    gmax = cus // (u1 // 32 + u2 // 32)
    nrt2 = gmax + 1 if gmax % 2 == 0 else gmax + 2          # an odd tile count: G = (nrt2 + 1) / 2 groups, the last one owns a single tile
    return dict(F1=32, P6=6, U33=33, A72=72, R2=32 * nrt2, R2p=32 * nrt2 - 5, R3=32 * (2 * gmax + 1))[form]


def test_case_table_covers_every_instantiation_and_option():
    """No device: at 64, 256 and 304 CUs every R2 / R2p case runs workgroups with two row tiles next to workgroups with one, R3 runs three; all
    18 forward and 18 backward instantiations occur; every option of the descriptors occurs, per dtype where the kernels differ by dtype."""
    assert 26 <= len(CASES) <= 32 and len(set(CASES)) == len(CASES) and len({case_id(c) for c in CASES}) == len(CASES)
    for cus in (64, 256, 304):
        for c in CASES:
            p = plan(form_batch(c.form, c.u1, c.u2, cus), c.u1, c.u2, cus)
            assert p.nm <= 32 and p.nm <= cus and p.G * p.nm <= cus, (c, cus)
            if c.form in ("R2", "R2p"):
                assert p.R == 2 and p.rvs == {1, 2}, (c, cus, p)
            elif c.form == "R3":
                assert p.R == 3 and 3 in p.rvs, (c, cus, p)
            elif p.gmax >= 3:                   # at most three tiles: one per workgroup wherever three groups are resident (>= 96 CUs for every pair)
                assert p.R == 1 and p.rvs == {1}, (c, cus, p)
            if c.form[0] == "R":
                assert c.T <= 3
    assert form_batch("R2", 512, 512, 256) == 288 and form_batch("R2p", 512, 512, 256) == 283 and form_batch("R3", 512, 512, 256) == 544
    assert form_batch("R2", 512, 256, 256) == 352 and form_batch("R2", 128, 128, 256) == 1056
    fwd, bwd = collections.Counter(), collections.Counter()
    for c in CASES:
        assert c.T in (1, 2, 6, 19) or (c.form[0] == "R" and c.T == 3)
        assert not (c.bwd and not c.save) and not (c.fold and c.keep >= 1.0) and c.state in STATES
        fwd[(c.u1, c.u2, c.dt)] += 1
        bwd[(c.u1, c.u2, c.dt)] += int(c.bwd)
    every = [(a, b, dt) for a in UNITS for b in UNITS for dt in (F, BF)]
    assert set(fwd) == set(every) and all(bwd[k] >= 1 for k in every), [k for k in every if not bwd[k]]
    for dt in (F, BF):
        mine = [c for c in CASES if c.dt == dt]
        have = lambda p: any(p(c) for c in mine)      # noqa: E731
        for u in UNITS:                               # every U at least twice in either layer role
            assert sum(c.u1 == u and c.bwd for c in mine) >= 2 and sum(c.u2 == u and c.bwd for c in mine) >= 2
        assert {c.form for c in mine} >= set(FORMS) - {"R3"} and {c.form for c in mine if c.bwd} >= set(FORMS) - {"R3"}
        assert {c.T for c in mine if c.bwd} >= {1, 2, 6, 19}
        assert have(lambda c: c.T == 1 and not c.save and c.state == "both") and have(lambda c: c.T == 1 and c.bwd and c.state == "both")
        assert have(lambda c: c.keep == 1.0 and c.bwd) and have(lambda c: c.keep == 0.9 and c.fold) and have(lambda c: c.keep == 0.9 and c.bwd and not c.fold)
        assert have(lambda c: not c.save and c.keep == 0.9) and have(lambda c: not c.save and c.keep == 1.0)
        assert have(lambda c: c.hT and not c.yT) and have(lambda c: c.yT and not c.hT)
        assert have(lambda c: c.hT and c.yT and c.pad == 8) and have(lambda c: c.hT and c.yT and c.pad == 24) and have(lambda c: c.hT and c.yT and c.pad == 4)
        for st in ("none", "both", "l2", "c0"):
            assert have(lambda c: c.state == st and c.bwd), (dt, st)
        assert have(lambda c: c.bwd and c.db and c.pad > 0) and have(lambda c: c.bwd and not c.db)
        for nolocal in (False, True):
            assert have(lambda c: c.nolocal == nolocal and c.bwd) and have(lambda c: c.nolocal == nolocal and c.bwd and c.form in ("R2", "R2p"))
    assert any(c.form == "R3" and c.bwd for c in CASES) and any(c.state == "l1" for c in CASES)
    assert C_ABS <= 4 * 2.0 ** -10 and GATES_ABS <= 2 * 2.0 ** -10            # never above the row-parallel bounds of the same tensors


# ------------------------------------------------------------------------------------------------ operands, reference and checks (no device)
def torch_dtype(dt):
    return torch.float16 if dt == "fp16" else torch.bfloat16


def eps_of(dt):
    return 2.0 ** -10 if dt == "fp16" else 2.0 ** -7


def _np64(t):
    return t.double().cpu().numpy()


def make_operands(rng, T, B, u1, u2, dt, keep, fold, state):
    """The operands of one launch pair as CPU tensors, drawn as test_gpu_rowpar_kernels.py draws them: weights N(0, 0.06) up to K = 256 and
    N(0, 0.04) at K = 512, rounded to the 16-bit type; xproj1 ~ N(0, 1.2) f32 gate-minor; layer 2's bias N(0, 1) so that its pre-activations
    span the range layer 1's do; h0 = tanh(N(0, 0.7)) rounded, c0 ~ N(0, 0.7) f32; dh_ext ~ N(0, 0.02) f32.  `dh_in` is what the caller hands
    layer 2: dh_ext itself, or, at keep < 1 without `fold`, the already dropped dh_ext / keep * mask2 (f32 arithmetic)."""
    tdt = torch_dtype(dt)
    r16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt)            # noqa: E731
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))                    # noqa: E731
    sd = lambda k: 0.06 if k <= 256 else 0.04                                      # noqa: E731
    o = dict(T=T, B=B, u1=u1, u2=u2, dt=dt, keep=keep, fold=fold)
    o["wh_t1"] = r16(rng.normal(0, sd(u1), (4 * u1, u1)))
    o["wh_t2"] = r16(rng.normal(0, sd(u2), (4 * u2, u2)))
    o["wx_t2"] = r16(rng.normal(0, sd(u1), (4 * u2, u1)))                          # gate-interleaved rows, K = u1
    o["bias2"] = f32(rng.normal(0, 1.0, 4 * u2))
    o["xproj1"] = f32(rng.normal(0, 1.2, (T, B, u1, 4)))
    for l, u in ((1, u1), (2, u2)):
        o[f"mask{l}"] = (rng.random((T, B, u)) < keep).astype(np.uint8) if keep < 1.0 else None
        h0, c0 = r16(np.tanh(rng.normal(0, 0.7, (B, u)))), f32(rng.normal(0, 0.7, (B, u)))
        o[f"h0_{l}"] = h0 if state in ("both", f"l{l}") else None
        o[f"c0_{l}"] = c0 if state in ("both", f"l{l}", "c0") else None
    o["dh_ext"] = f32(rng.normal(0, 0.02, (T, B, u2)))
    o["dh_in"] = o["dh_ext"]
    if keep < 1.0 and not fold:
        o["dh_in"] = o["dh_ext"] / np.float32(keep) * torch.from_numpy(o["mask2"]).float()
    return o


def _opt64(t):
    return None if t is None else _np64(t)


C_ABS = 2.0 ** -16       # |c - c_ref|, absolute (f32 output): 4 x the largest measured error (2.65e-6), rounded up to a power of two (profiles/persist_kernel_tests.md)
GATES_ABS = 2.0 ** -19   # |gates - gates_ref|, absolute (f32 output), derived the same way (largest measured: 3.29e-7)
BOUNDS = dict(c=C_ABS, gates=GATES_ABS, h=2, y=3, dz=3, db=1)    # h, y in eps; dz in eps x max |dz_ref|; db in units of 1e-5 max(1, |ref|) + 1e-6


def forward_reference(o, out):
    """The float64 forward of both layers on the operands and on the stored 16-bit h / y of `out` (lstm2_float64.forward)."""
    T, B = o["T"], o["B"]
    view = lambda name, u: out[name][:T * B].view(T, B, u)                                      # noqa: E731
    h1, h2 = view("h1", o["u1"]), view("h2", o["u2"])
    out1 = view("y1", o["u1"]) if o["mask1"] is not None else h1
    return L2_64.forward(_np64(o["wh_t1"]), _np64(o["xproj1"]), _np64(h1), _np64(out1), _np64(o["wh_t2"]), _np64(o["wx_t2"]), _np64(o["bias2"]),
                         _np64(h2), (_opt64(o["h0_1"]), _opt64(o["c0_1"])), (_opt64(o["h0_2"]), _opt64(o["c0_2"])))


def check_forward(o, out):
    """o: make_operands; out: CPU tensors of one forward launch -- per layer l the guarded buffers c{l} [T B + 1, u] f32, h{l}, y{l} (under a mask)
    16-bit, gates{l} [T B + 1, 4u] f32 (saved), and hT{l} / yT{l} [u, ld] where asked for.  Asserts what must hold bit for bit (transposed copies,
    sentinels) and returns the measured errors against float64, keyed `<tensor><layer>`."""
    T, B, keep, eps = o["T"], o["B"], o["keep"], eps_of(o["dt"])
    N = T * B
    tdt = torch_dtype(o["dt"])
    r16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt).double().numpy()       # noqa: E731
    view = lambda name, u: out[name][:N].view(T, B, u)                                          # noqa: E731
    refs = forward_reference(o, out)
    errs = {}
    for l, ref in ((1, refs[0]), (2, refs[1])):
        u, mask = o[f"u{l}"], o[f"mask{l}"]
        h = view(f"h{l}", u)
        errs[f"c{l}"] = np.abs(_np64(view(f"c{l}", u)) - ref["c"]).max()
        errs[f"h{l}"] = np.abs(_np64(h) - ref["h"]).max() / eps                # every step, with or without a mask: this form always stores h
        outl = h
        if mask is not None:
            outl = view(f"y{l}", u)
            errs[f"y{l}"] = np.abs(_np64(outl) - r16(ref["h"]) / keep * mask).max() / eps
        else:
            assert f"y{l}" not in out
        if f"gates{l}" in out:
            errs[f"gates{l}"] = np.abs(_np64(out[f"gates{l}"][:N]).reshape(T, B, u, 4) - ref["g"]).max()
        for name in ("gates", "c", "h", "y"):
            if f"{name}{l}" in out:
                assert bool((out[f"{name}{l}"][N] == SENT).all()), f"guard row behind {name}{l}"
        if f"yT{l}" in out:           # y^T[unit][t B + row] = the layer's output
            yT = out[f"yT{l}"]
            assert torch.equal(yT[:, :N].reshape(u, T, B), outl.permute(2, 0, 1)), f"yT{l} is not the output, bit for bit"
            assert bool((yT[:, N:] == SENT).all()), f"padding columns of yT{l}"
        if f"hT{l}" in out:           # h^T[unit][(t + 1) B + row] = h[t]; column block 0 (h[-1]) is the caller's
            hT = out[f"hT{l}"]
            assert torch.equal(hT[:, B:N].reshape(u, T - 1, B), h[:T - 1].permute(2, 0, 1)), f"hT{l} is not h, bit for bit"
            assert bool((hT[:, :B] == SENT).all()), f"column block 0 of hT{l}"
            assert bool((hT[:, N:] == SENT).all()), f"padding columns of hT{l}"
    return errs


def check_backward(o, out):
    """out: the forward's saved tensors (gates{l}, c{l}) plus, per layer, dzT{l} [4u, ld] 16-bit (dz^T[column][t B + row]) and db{l} [4u] f32
    preloaded with DB0 (absent: no bias gradient).  dz against the float64 backward on the kernel's own saved tensors and stored dz; db against
    the float64 column sums of the stored dz over the rows < B; padding columns untouched."""
    T, B, keep, eps = o["T"], o["B"], o["keep"], eps_of(o["dt"])
    N = T * B
    dzk, sv = {}, {}
    for l in (1, 2):
        u = o[f"u{l}"]
        dzk[l] = _np64(out[f"dzT{l}"][:, :N].t()).reshape(T, B, 4 * u)
        sv[l] = (_np64(out[f"gates{l}"][:N]).reshape(T, B, u, 4), _np64(out[f"c{l}"][:N]).reshape(T, B, u))
    refs = L2_64.backward(_np64(o["wh_t1"]), sv[1][0], sv[1][1], dzk[1], o["mask1"], _np64(o["wh_t2"]), _np64(o["wx_t2"]), sv[2][0], sv[2][1], dzk[2],
                          _np64(o["dh_in"]), o["mask2"] if o["fold"] else None, keep, _opt64(o["c0_1"]), _opt64(o["c0_2"]))
    errs = {}
    for l, dz_ref in ((1, refs[0]), (2, refs[1])):
        scale = np.abs(dz_ref).max()
        assert scale > 1e-3, f"dz{l} too small to test f16"
        errs[f"dz{l}"] = np.abs(dzk[l] - dz_ref).max() / (eps * scale)
        assert bool((out[f"dzT{l}"][:, N:] == SENT).all()), f"padding columns of dzT{l}"
        if f"db{l}" in out:
            db_ref = dzk[l].sum((0, 1))
            errs[f"db{l}"] = np.abs(_np64(out[f"db{l}"]) - DB0 - db_ref).max() / (1e-5 * max(1.0, np.abs(db_ref).max()) + 1e-6)
    return errs


def assert_bounds(errs):
    for k, v in errs.items():
        assert v < BOUNDS[k[:-1]], f"bound of {k}: {v:.4g} >= {BOUNDS[k[:-1]]:.4g}"


def _report(tag, errs):
    print("\n[persist-kernels] " + json.dumps(dict(case=tag, errs={k: float(f"{float(v):.4g}") for k, v in errs.items()})))


def synthetic_outputs(o, pad):
    """What a flawless kernel would store: the float64 recurrence that feeds back its own 16-bit rounded hand-offs, rounded to the output types."""
    T, B, keep = o["T"], o["B"], o["keep"]
    N = T * B
    tdt = torch_dtype(o["dt"])
    t16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt)            # noqa: E731
    r16 = lambda a: t16(a).double().numpy()                                        # noqa: E731
    out, W, dzk = {}, {}, {}

    def guarded(a, cols, dtype):
        g = torch.full((N + 1, cols), SENT, dtype=dtype)
        g[:N] = torch.from_numpy(np.asarray(a, np.float32)).reshape(N, cols).to(dtype)
        return g

    X = _np64(o["xproj1"])
    for l in (1, 2):
        u, mask = o[f"u{l}"], o[f"mask{l}"]
        W[l] = _np64(o[f"wh_t{l}"])
        ref = L64.forward(W[l], X, lambda t, hv: r16(hv), h0=_opt64(o[f"h0_{l}"]), c0=_opt64(o[f"c0_{l}"]))
        out[f"gates{l}"], out[f"c{l}"], out[f"h{l}"] = guarded(ref["g"], 4 * u, torch.float32), guarded(ref["c"], u, torch.float32), guarded(ref["h"], u, tdt)
        res = r16(ref["h"])
        if mask is not None:
            res = r16(res / keep * mask)
            out[f"y{l}"] = guarded(res, u, tdt)
        for name, src, first in (("hT", r16(ref["h"])[:T - 1], B), ("yT", res, 0)):
            tr = torch.full((u, N + pad), SENT, dtype=tdt)
            tr[:, first:N] = t16(src).permute(2, 0, 1).reshape(u, -1)
            out[f"{name}{l}"] = tr
        if l == 1:
            X = L2_64.layer2_xproj(res, _np64(o["wx_t2"]), _np64(o["bias2"]))
    dh = _np64(o["dh_in"])
    for l in (2, 1):
        u = o[f"u{l}"]
        sv = (_np64(out[f"gates{l}"][:N]).reshape(T, B, u, 4), _np64(out[f"c{l}"][:N]).reshape(T, B, u))
        mask = o[f"mask{l}"] if (l == 1 or o["fold"]) else None
        dzk[l] = r16(L64.backward(W[l], sv[0], sv[1], dh, mask, keep, lambda t, dz: r16(dz), c0=_opt64(o[f"c0_{l}"])))
        tr = torch.full((4 * u, N + pad), SENT, dtype=tdt)
        tr[:, :N] = t16(dzk[l]).reshape(N, 4 * u).t()
        out[f"dzT{l}"] = tr
        out[f"db{l}"] = torch.from_numpy((DB0 + dzk[l].sum((0, 1))).astype(np.float32))
        dh = dzk[2] @ _np64(o["wx_t2"])
    return out


@pytest.mark.parametrize("dt", [F, BF])
def test_checker_rejects_small_defects(dt):
    """No device: check_forward / check_backward / assert_bounds -- the comparison the GPU cases run -- pass the float64 reference rounded to the
    output types (T = 3, B = 38: a second row tile of six rows; 64 and 32 units, keep 0.9, states, padded leading dimensions) and reject, each
    for its own reason: one element of h off by 4 ulp; two rows of the partial last tile swapped in h^T only; step T - 1's row B (the duplicate
    of row B - 1 a clamped offset computes) written into the guard row; db including that row; one padding column of dz^T overwritten."""
    T, B, u1, u2, pad = 3, 38, 64, 32, 8
    N = T * B
    o = make_operands(np.random.default_rng(7), T, B, u1, u2, dt, 0.9, True, "both")
    o["dh_ext"] *= 8
    o["dh_in"] = o["dh_ext"]          # few units: keep max |dz| above the 1e-3 the f16 cases ask for
    good = synthetic_outputs(o, pad)

    def passes(out):
        assert_bounds(check_forward(o, out))
        assert_bounds(check_backward(o, out))

    def variant(**changed):
        out = {k: v.clone() for k, v in good.items()}
        out.update(changed)
        return out

    passes(good)
    # ---- one element of h2 off by 4 ulp, away from the float64 value: a value in [0.5, 1) has ulp = eps / 2, so the error reaches the 2 eps bound ----
    # (taken from the last step: nothing is fed back from it, and h^T does not hold it -- only the bound can notice)
    ref2 = forward_reference(o, good)[1]["h"].reshape(N, u2)
    h = good["h2"].clone()
    mag = h[:N].double().abs()
    mag[:N - B] = 0
    idx = int(torch.nonzero(((mag >= 0.53) & (mag < 0.96)).reshape(-1))[0])
    r, col = divmod(idx, u2)
    away = 1 if abs(float(h[r, col])) >= abs(float(ref2[r, col])) else -1       # a larger magnitude is a larger bit pattern
    h.view(torch.int16)[r, col] += 4 * away
    assert abs(float(h[r, col]) - float(good["h2"][r, col])) == 4 * eps_of(dt) / 2
    with pytest.raises(AssertionError, match="bound of h2"):
        passes(variant(h2=h))
    # ---- two rows of the partial last tile (rows 32 .. 37) swapped in hT1 only ----
    hT = good["hT1"].clone()
    hT[:, [B + 33, B + 36]] = hT[:, [B + 36, B + 33]]
    with pytest.raises(AssertionError, match="hT1 is not h"):
        passes(variant(hT1=hT))
    # ---- step T - 1's row B into the guard row ----
    for name in ("h1", "c2", "gates1", "y2"):
        g = good[name].clone()
        g[N] = g[N - 1]
        with pytest.raises(AssertionError, match=f"guard row behind {name}"):
            passes(variant(**{name: g}))
    # ---- db including one row >= B ----
    for l in (1, 2):
        db = good[f"db{l}"] + good[f"dzT{l}"][:, N - 1].float()
        with pytest.raises(AssertionError, match=f"bound of db{l}"):
            passes(variant(**{f"db{l}": db}))
    # ---- one padding column of dz^T (and of h^T, y^T) overwritten ----
    for name in ("dzT1", "dzT2", "hT2", "yT1"):
        tr = good[name].clone()
        tr[:, N] = tr[:, N - 1]
        with pytest.raises(AssertionError, match=f"padding columns of {name}"):
            passes(variant(**{name: tr}))
    # ---- and a defect of the f32 outputs far below the 16-bit units: one cell state off by 2 C_ABS, one gate by 2 GATES_ABS ----
    c = good["c1"].clone()
    c[5, 3] += 2 * C_ABS
    with pytest.raises(AssertionError, match="bound of c1"):
        passes(variant(c1=c))
    g = good["gates2"].clone()
    g[7, 9] += 2 * GATES_ABS
    with pytest.raises(AssertionError, match="bound of gates2"):
        passes(variant(gates2=g))


# ------------------------------------------------------------------------------------------------ the device cases
@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def _set_nolocal(monkeypatch, nolocal):
    if nolocal:
        monkeypatch.setenv("MNN_PERSIST_NO_LOCAL", "1")          # the library reads its switches on every call
    else:
        monkeypatch.delenv("MNN_PERSIST_NO_LOCAL", raising=False)


def _poison_exchange(ws, T, B, u1, u2):
    """Fill the workspace's exchange area -- its last max(T nrt 64 (2 u1 + u2), T nrt 256 (u1 + u2)) bytes; in front of it: the sync words and
    the edge slabs each launch resets itself, and the sticky word -- with 0xFF bytes, a NaN in f16 and bf16, before a launch: what a step reads
    there must have been written by THIS launch, never be an earlier launch's identical values."""
    per = T * cdiv(B, 32)
    ws[ws.numel() - max(per * 64 * (2 * u1 + u2), per * 256 * (u1 + u2)):] = 0xFF


def _device_buffers(o, case, ld):
    """Sentinel-filled outputs of both launches on the device, keyed as check_forward / check_backward read them."""
    T, B = o["T"], o["B"]
    N = T * B
    tdt = torch_dtype(o["dt"])
    full = lambda shape, dtype, v=SENT: torch.full(shape, v, device=DEV, dtype=dtype)           # noqa: E731
    buf = {}
    for l in (1, 2):
        u = o[f"u{l}"]
        buf[f"c{l}"], buf[f"h{l}"] = full((N + 1, u), torch.float32), full((N + 1, u), tdt)
        if case.save:
            buf[f"gates{l}"] = full((N + 1, 4 * u), torch.float32)
        if o[f"mask{l}"] is not None:
            buf[f"y{l}"] = full((N + 1, u), tdt)
        for name, on in (("hT", case.hT), ("yT", case.yT)):
            if on:
                buf[f"{name}{l}"] = full((u, ld), tdt)
        if case.bwd:
            buf[f"dzT{l}"] = full((4 * u, ld), tdt)
            if case.db:
                buf[f"db{l}"] = full((4 * u,), torch.float32, DB0)
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_persist_kernel_vs_float64(ops, monkeypatch, case):
    """One form: every forward output of both layers against float64 (c, gates: the absolute f32 bounds; h 2 eps at every step, with or without a
    mask; y 3 eps of r16(h) / keep * mask; the final state is step T - 1 of c and h), y^T bit-equal to the layer's output and h^T to h with column
    block 0 untouched; the backward on the kernel's own saved tensors (dz 3 eps x max |dz_ref|, read from dz^T; db - 0.5 against the column sums
    of the stored dz, 1e-5); nothing written outside the outputs (guard rows, padding columns); the status word after every launch; a second
    forward + backward on the same workspace and buffers bit for bit (db aside: float atomics).  The exchange area is NaN-filled before every
    launch (_poison_exchange)."""
    _set_nolocal(monkeypatch, case.nolocal)
    u1, u2, T, keep = case.u1, case.u2, case.T, case.keep
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = form_batch(case.form, u1, u2, cus)
    p = plan(B, u1, u2, cus)
    assert p.nm <= cus and ops.lstm2_persist_ok(B, u1, u2)
    if case.form in ("R2", "R2p"):
        assert p.R == 2 and p.rvs == {1, 2}, (p, cus)
    elif case.form == "R3" or p.gmax >= 3:
        assert p.R == (3 if case.form == "R3" else 1), (p, cus)
    N, ld = T * B, T * B + case.pad
    o = make_operands(np.random.default_rng(2000 + CASES.index(case)), T, B, u1, u2, case.dt, keep, case.fold, case.state)
    buf = _device_buffers(o, case, ld)
    dev = lambda t: None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)       # noqa: E731
    d = {k: dev(v) for k, v in o.items() if isinstance(v, (torch.Tensor, np.ndarray)) or v is None}
    view = lambda name, l, cols: buf[f"{name}{l}"][:N].view(T, B, cols) if f"{name}{l}" in buf else None            # noqa: E731
    ws = ops.lstm2_persist_workspace(T, B, u1, u2, DEV)
    L1 = ops.lstm2_fwd_layer(d["xproj1"].view(T, B, 4 * u1), d["wh_t1"], d["h0_1"], d["c0_1"], view("gates", 1, 4 * u1), view("c", 1, u1),
                             view("h", 1, u1), buf.get("hT1"), view("y", 1, u1), d["mask1"], yT=buf.get("yT1"))
    L2 = ops.lstm2_fwd_layer(None, d["wh_t2"], d["h0_2"], d["c0_2"], view("gates", 2, 4 * u2), view("c", 2, u2), view("h", 2, u2), buf.get("hT2"),
                             view("y", 2, u2), d["mask2"], d["wx_t2"], d["bias2"], yT=buf.get("yT2"))

    def forward():
        _poison_exchange(ws, T, B, u1, u2)
        ops.lstm2_persist_fwd(T, B, L1, L2, keep, ws)
        torch.cuda.synchronize()
        ops.lstm2_persist_check(ws, B, u1, u2)

    forward()
    errs = check_forward(o, {k: v.cpu() for k, v in buf.items()})
    _report(case_id(case) + f" B{B} fwd", errs)
    assert_bounds(errs)
    if case.bwd:
        wss = [ops.lstm_seq_bwd_workspace(B, u, DEV) for u in (u1, u2)]
        wh_p1, wh_p2, wx_p2 = (d[k].t().contiguous() for k in ("wh_t1", "wh_t2", "wx_t2"))    # [k][gate-interleaved column]; a descriptor holds addresses
        E1 = ops.lstm2_bwd_layer(None, wh_p1, view("gates", 1, 4 * u1), view("c", 1, u1), d["c0_1"], None, wss[0], buf["dzT1"], buf.get("db1"), d["mask1"])
        E2 = ops.lstm2_bwd_layer(d["dh_in"], wh_p2, view("gates", 2, 4 * u2), view("c", 2, u2), d["c0_2"], None, wss[1], buf["dzT2"], buf.get("db2"),
                                 d["mask2"] if case.fold else None, wx_p2)

        def backward():
            _poison_exchange(ws, T, B, u1, u2)
            ops.lstm2_persist_bwd(T, B, E1, E2, keep, ws)
            torch.cuda.synchronize()
            ops.lstm2_persist_check(ws, B, u1, u2)

        saved = {k: v.clone() for k, v in buf.items() if k[:2] not in ("dz", "db")}
        backward()
        berrs = check_backward(o, {k: v.cpu() for k, v in buf.items()})
        _report(case_id(case) + f" B{B} bwd", berrs)
        assert_bounds(berrs)
        for k, v in saved.items():                    # the backward launch left the forward's outputs, guard rows and padding alone
            assert torch.equal(buf[k], v), k
    # ---- the same workspace and buffers again: every output bit for bit (db is summed with float atomics) ----
    first = {k: v.clone() for k, v in buf.items()}
    for l in (1, 2):
        if f"db{l}" in buf:
            buf[f"db{l}"].fill_(DB0)
    forward()
    if case.bwd:
        backward()
    for k in buf:
        if not k.startswith("db"):
            assert torch.equal(buf[k], first[k]), k
    if case.bwd:
        assert_bounds({k: v for k, v in check_backward(o, {k: v.cpu() for k, v in buf.items()}).items() if k.startswith("db")})


@pytest.mark.gpu
def test_persist_backward_refuses_an_external_gradient_for_layer_1(ops):
    """Layer 1's gradient comes from layer 2 inside the launch; a layer-1 descriptor that names a dh_ext would have it dropped without a word.
    The entry refuses it on the host: MnnError, nothing launched, dz^T and db as they were."""
    from multinn_amd._lib import MnnError
    T, B, u = 2, 6, 128
    N = T * B
    tdt = torch.bfloat16
    w = torch.zeros((u, 4 * u), device=DEV, dtype=tdt)
    dh, gates, c = torch.zeros((T, B, u), device=DEV), torch.zeros((T, B, 4 * u), device=DEV), torch.zeros((T, B, u), device=DEV)
    dzT = [torch.full((4 * u, N), SENT, device=DEV, dtype=tdt) for _ in range(2)]
    db = [torch.full((4 * u,), DB0, device=DEV) for _ in range(2)]
    ws = ops.lstm2_persist_workspace(T, B, u, u, DEV)
    wss = [ops.lstm_seq_bwd_workspace(B, u, DEV) for _ in range(2)]
    E1 = ops.lstm2_bwd_layer(dh, w, gates, c, None, None, wss[0], dzT[0], db[0])
    E2 = ops.lstm2_bwd_layer(dh, w, gates, c, None, None, wss[1], dzT[1], db[1], None, w)
    with pytest.raises(MnnError, match="layer 1"):
        ops.lstm2_persist_bwd(T, B, E1, E2, 1.0, ws)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in dzT) and all(bool((t == DB0).all()) for t in db)
    ops.lstm2_persist_check(ws, B, u, u)
