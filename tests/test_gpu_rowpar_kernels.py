"""Every kernel form of the row-parallel persistent recurrence (csrc/lstm_rowpar.hip), element by element against float64.

`rp_fwd_kernel` / `rp_bwd_kernel` instantiate four kernels 24 times forward (U in {128, 256, 512} x wave pair | single wave x 16-bit | f32
input projection x f16 | bf16) and 12 times backward.  Each case below calls ops.lstm_rowpar_fwd / ops.lstm_rowpar_bwd directly on descriptors
of ops.lstm2_fwd_layer / ops.lstm2_bwd_layer and compares every output with tests/lstm_float64.py on the kernel's own 16-bit operands (the
reference and the bounds of test_gpu_kernels.py::test_lstm_resident_recurrence_vs_float64 / ::test_lstm_cluster_recurrence_vs_float64, in
units of eps = 2^-10 for f16 and 2^-7 for bf16; measured errors: profiles/rowpar_kernel_tests.md).

A FORM is (B, MNN_ROWPAR_MAX_G, MNN_ROWPAR_NO_PAIR): the smallest batch that selects the kernel family and tile count --
    P1  pair, one row tile, one group          P2  pair, both pair slots of one workgroup      PG  pair, two row-tile groups
    S3  single wave, three tiles per workgroup S4  single wave, four tiles (U = 512: forward only, the backward holds three)
    S1  single wave, one tile
The descriptor options that change `behind` -- the run-time count of vector-memory operations behind a hand-off, which the flag's wait must
skip exactly -- are spread over the table: gates saved or not, h or y, h^T, y^T, a mask, dz^T K-blocked / plain / absent, the last step.
test_case_table_covers_every_instantiation_and_option (no device) proves the table's coverage from a restatement of rp_plan / rp_pair."""
import collections
import json

import numpy as np
import pytest
import torch

import lstm_float64 as L64

DEV = "cuda:0"
SENT = -768.0            # exactly representable in f16 / bf16 / f32 and outside the range of every output (|h|, |y|, gates <= 1.2, |c| <= T)

# form -> (B, MNN_ROWPAR_MAX_G, MNN_ROWPAR_NO_PAIR)
FORMS = {"P1": (32, None, False), "P2": (64, 1, False), "PG": (64, None, False), "S3": (96, 1, False), "S4": (128, 1, False), "S1": (32, None, True)}

Case = collections.namedtuple("Case", "form u dt xb T keep hT yT layout pad nolocal save bwd")


def C(form, u, dt, xb, T, keep, hT=True, yT=True, layout="kblock", pad=0, nolocal=False, save=True, bwd=True):
    """xb: 16-bit input projection (False: f32); layout: dz^T "kblock" | "plain" | None (dz row-major and db only); pad: extra columns of the
    leading dimension of h^T, y^T and the plain dz^T (a multiple of 8); save = False: the inference variant (no gates, no transposed copies)."""
    if not save:
        hT = yT = bwd = False
    return Case(form, u, dt, xb, T, keep, hT, yT, layout if bwd else None, pad, nolocal, save, bwd)


F, BF = "fp16", "bf16"
CASES = [
    # ---- wave pairs (lstm_rowpar_fwd2_kernel / lstm_rowpar_bwd2_kernel) ----
    C("P1", 128, F, True, 2, 1.0),
    C("P2", 128, BF, True, 6, 0.9, yT=False, layout="plain", pad=8),
    C("PG", 128, F, False, 19, 0.9, layout=None, pad=24),
    C("P1", 128, BF, False, 6, 1.0, hT=False, nolocal=True),
    C("P2", 256, F, True, 19, 0.9),
    C("PG", 256, BF, True, 6, 1.0, layout="plain", pad=8),
    C("P1", 256, F, False, 6, 0.9, hT=False, layout=None),
    C("P2", 256, BF, False, 2, 0.9, nolocal=True),
    C("PG", 512, F, True, 6, 0.9),
    C("P1", 512, BF, True, 19, 1.0, layout="plain", pad=16),
    C("P2", 512, F, False, 6, 1.0, yT=False),
    C("PG", 512, BF, False, 6, 0.9, layout=None, nolocal=True),
    C("P2", 512, F, True, 6, 0.9, save=False),
    C("PG", 128, BF, False, 6, 1.0, save=False),
    C("P1", 256, BF, True, 2, 1.0, save=False, nolocal=True),
    # ---- one wave per (row tile, unit tile) (lstm_rowpar_fwd_kernel / lstm_rowpar_bwd_kernel) ----
    C("S3", 128, F, True, 6, 0.9),
    C("S4", 128, BF, True, 19, 1.0, layout="plain", pad=8),
    C("S1", 128, F, False, 2, 0.9, yT=False, layout=None),
    C("S4", 128, BF, False, 6, 0.9, hT=False, nolocal=True),
    C("S4", 256, F, True, 6, 0.9),
    C("S3", 256, BF, True, 6, 1.0, hT=False, layout="plain", pad=24),
    C("S1", 256, F, False, 19, 0.9),
    C("S4", 256, BF, False, 2, 1.0, layout=None, nolocal=True),
    C("S3", 512, F, True, 19, 0.9),
    C("S3", 512, BF, True, 6, 1.0, yT=False, layout="plain", pad=8),
    C("S1", 512, F, False, 6, 0.9, layout=None),
    C("S3", 512, BF, False, 6, 0.9, nolocal=True),
    C("S4", 512, F, True, 6, 0.9, bwd=False),            # four tiles: the forward runs, the backward is refused before any launch
    C("S4", 512, BF, False, 2, 1.0, bwd=False),
    C("S3", 256, BF, True, 6, 1.0, save=False),
    C("S1", 128, F, False, 6, 0.9, save=False),
]


def case_id(c):
    opts = [c.form, f"u{c.u}", c.dt, "x16" if c.xb else "x32", f"T{c.T}", f"k{c.keep}"]
    opts += [] if c.save else ["nosave"]
    opts += [n for n, on in (("hT", c.hT), ("yT", c.yT)) if on] + ([f"dzT-{c.layout}"] if c.layout else []) + ([f"pad{c.pad}"] if c.pad else [])
    opts += (["nolocal"] if c.nolocal else []) + ([] if c.bwd or not c.save else ["fwdonly"])
    return "-".join(opts)


def tiles_per_workgroup(B, u, max_g, cus):
    """rp_plan: G = min(CUs / (U / 32), B / 32, MAX_G) row-tile groups, ceil((B / 32) / G) row tiles (= waves or wave pairs) per workgroup."""
    nrt = B // 32
    G = max(1, min(cus // (u // 32), nrt, max_g if max_g is not None else nrt))
    return -(-nrt // G)


def family(form, u, cus):
    """rp_pair: wave pairs when a workgroup owns at most two row tiles and MNN_ROWPAR_NO_PAIR is not set."""
    B, max_g, no_pair = FORMS[form]
    return "pair" if tiles_per_workgroup(B, u, max_g, cus) <= 2 and not no_pair else "single"


def test_case_table_covers_every_instantiation_and_option():
    """No device: the case table reaches all 24 forward instantiations at least once and all 12 backward instantiations at least twice, and
    inside each kernel family (pair, single) every descriptor option occurs: keep 0.9 and 1.0, no saved gates, h^T without y^T and the
    reverse, dz^T K-blocked / plain with a padded leading dimension / absent, MNN_PERSIST_NO_LOCAL, T = 2, 6 and 19 (past any 8- or
    16-deep ring; T = 1 never reaches these kernels from LstmStack)."""
    assert 24 <= len(CASES) <= 36 and len(set(CASES)) == len(CASES) and len({case_id(c) for c in CASES}) == len(CASES)
    for form, fam, tiles in (("P1", "pair", 1), ("P2", "pair", 2), ("PG", "pair", 1), ("S3", "single", 3), ("S4", "single", 4), ("S1", "single", 1)):
        for u in (128, 256, 512):
            for cus in (32, 64, 256, 304):        # PG needs two groups of U / 32 workgroups (>= 32 CUs); the other forms no particular count
                assert family(form, u, cus) == fam and tiles_per_workgroup(FORMS[form][0], u, FORMS[form][1], cus) == tiles, (form, u, cus)
    fwd, bwd = collections.Counter(), collections.Counter()
    for c in CASES:
        fam = family(c.form, c.u, 256)
        fwd[(c.u, fam, c.xb, c.dt)] += 1
        assert not (c.bwd and not c.save) and c.pad % 8 == 0 and c.T in (2, 6, 19)
        assert not (c.bwd and c.form == "S4" and c.u == 512)        # rp_plan(bwd): three waves per workgroup at U = 512
        if c.bwd:
            bwd[(c.u, fam, c.dt)] += 1
    every_fwd = [(u, fam, xb, dt) for u in (128, 256, 512) for fam in ("pair", "single") for xb in (True, False) for dt in (F, BF)]
    every_bwd = [(u, fam, dt) for u in (128, 256, 512) for fam in ("pair", "single") for dt in (F, BF)]
    assert all(fwd[k] >= 1 for k in every_fwd) and set(fwd) == set(every_fwd), [k for k in every_fwd if not fwd[k]]
    assert all(bwd[k] >= 2 for k in every_bwd) and set(bwd) == set(every_bwd), [k for k in every_bwd if bwd[k] < 2]
    assert any(c.form == "S4" and c.u == 512 and c.save and not c.bwd for c in CASES)          # the refused backward
    for fam in ("pair", "single"):
        mine = [c for c in CASES if family(c.form, c.u, 256) == fam]
        have = lambda p: any(p(c) for c in mine)      # noqa: E731
        assert {c.form for c in mine} == {f for f in FORMS if f[0] == fam[0].upper()}
        assert have(lambda c: c.keep == 0.9) and have(lambda c: c.keep == 1.0)
        assert have(lambda c: not c.save)
        assert have(lambda c: c.hT and not c.yT) and have(lambda c: c.yT and not c.hT) and have(lambda c: c.hT and c.yT and c.pad > 0)
        assert have(lambda c: c.bwd and c.layout == "kblock") and have(lambda c: c.bwd and c.layout == "plain" and c.pad > 0)
        assert have(lambda c: c.bwd and c.layout is None)
        assert have(lambda c: c.nolocal and c.bwd) and have(lambda c: not c.nolocal and c.bwd)
        assert {c.T for c in mine} == {2, 6, 19} and {c.T for c in mine if c.bwd} == {2, 6, 19}


@pytest.fixture(scope="module")
def ops():
    from multinn_amd import ops as o
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return o


def _set_form(monkeypatch, max_g, no_pair, nolocal):
    for name, val in (("MNN_ROWPAR_MAX_G", None if max_g is None else str(max_g)), ("MNN_ROWPAR_NO_PAIR", "1" if no_pair else None),
                      ("MNN_PERSIST_NO_LOCAL", "1" if nolocal else None)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)          # the library reads its switches on every call


def _guarded(rows, cols, dtype):
    """[rows + 1, cols] of the sentinel: the kernel gets the first `rows`, the last one is the guard row behind them."""
    return torch.full((rows + 1, cols), SENT, device=DEV, dtype=dtype)


def _poison_exchange(ws, T, B, u):
    """Fill the workspace's exchange slabs (its last T x B / 32 slabs of 4u x 32 16-bit values; in front of them: the sync words and the edge
    slabs each launch resets itself) with 0xFFFF, a NaN in f16 and bf16, before a launch: what a step reads there must have been written
    by THIS launch.  A consumer that loaded a slab before its producer's hand-off stores had landed -- a flag raised too early -- would
    carry NaN into every later output, in the first run and, where the stale bytes of an earlier launch would otherwise be the right
    values, in the repeated one.  In production the slabs hold the previous train step's values at that point, never zeros."""
    ws[ws.numel() - T * (B // 32) * (u // 4) * 1024:] = 0xFF


def _np64(t):
    return t.double().cpu().numpy()


def _report(tag, errs, bounds):
    print("\n[rowpar-kernels] " + json.dumps(dict(case=tag, errs={k: round(float(v), 4) for k, v in errs.items()}, bounds=bounds)))


FWD_BOUNDS = dict(c=4, h=2, y=3, gates=2, hT=2)         # in eps
BWD_BOUNDS = dict(dz=3, db=1)                           # dz: eps x max |dz_ref|; db: in units of 1e-5 max(1, |ref|) + 1e-6


def _check_backward(W, gates, c, dh, mask, keep, dzc_f, dzT, db, T, B, u, eps, layout, pad):
    """dz against the float64 backward on the kernel's own saved gates and c (feeding back the kernel's 16-bit dz), dz^T bit-equal to the
    row-major dz, db against the float64 column sums of the stored dz, guard row and padding untouched.  Returns the measured errors."""
    N = T * B
    dzc = dzc_f[:N].view(T, B, 4 * u)
    dzk = _np64(dzc)
    dz_ref = L64.backward(W, _np64(gates).reshape(T, B, u, 4), _np64(c), _np64(dh), mask, keep, lambda t, dz: dzk[t])
    scale = np.abs(dz_ref).max()
    errs = dict(dz=np.abs(dzk - dz_ref).max() / (eps * scale))
    flat = dzc_f[:N]
    db_ref = _np64(flat).sum(0)
    errs["db"] = np.abs(db.cpu().numpy() - db_ref).max() / (1e-5 * max(1.0, np.abs(db_ref).max()) + 1e-6)
    assert scale > 1e-3 and float(flat.float().abs().max()) > 0
    if layout == "kblock":
        assert torch.equal(dzT.permute(0, 2, 1).reshape(N, 4 * u), flat)
    elif layout == "plain":
        assert torch.equal(dzT[:, :N].t(), flat)
        assert dzT.shape[1] == N + pad and bool((dzT[:, N:] == SENT).all())
    assert bool((dzc_f[N] == SENT).all())                       # the guard row behind dz
    return errs


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rowpar_kernel_vs_float64(ops, monkeypatch, case):
    """One kernel form: forward h / y / c / gates / h^T / y^T against float64 (c 4 eps, h 2 eps, y 3 eps of r16(h) / keep * mask, gates 2 eps,
    y^T bit-equal to the output, h^T 2 eps with column block 0 untouched), backward on the kernel's own saved tensors (dz 3 eps x max |dz_ref|,
    dz^T bit-equal to dz, db 1e-5), no write outside the outputs (guard rows, padding columns, h under a mask), the status word after every
    launch, and a second forward + backward on the same workspace and buffers bit for bit (db aside: float atomics).  The exchange slabs are
    NaN-filled before every launch (_poison_exchange): nothing a step reads may come from an earlier launch."""
    from multinn_amd._lib import MnnError
    B, max_g, no_pair = FORMS[case.form]
    _set_form(monkeypatch, max_g, no_pair, case.nolocal)
    u, T, keep = case.u, case.T, case.keep
    N = T * B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if case.form == "PG":
        assert cus >= 32, "two row-tile groups of a 512-unit layer need 32 CUs"
    assert family(case.form, u, cus) == ("pair" if case.form[0] == "P" else "single")
    refused = case.form == "S4" and u == 512
    assert ops.lstm_rowpar_ok(B, u) == (not refused)
    tdt = torch.float16 if case.dt == "fp16" else torch.bfloat16
    eps = 2.0 ** -10 if case.dt == "fp16" else 2.0 ** -7
    rng = np.random.default_rng(1000 + CASES.index(case))
    r16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt)            # noqa: E731
    wh_t = r16(rng.normal(0, 0.06 if u <= 256 else 0.04, (4 * u, u)))              # [gate-interleaved row][k]
    xproj = torch.from_numpy(rng.normal(0, 1.2, (T, B, u, 4)).astype(np.float32))  # gate-minor; the f32 forms read these f32 values
    if case.xb:
        xproj = xproj.to(tdt)
    mask = (rng.random((T, B, u)) < keep).astype(np.uint8) if keep < 1.0 else None
    dh = torch.from_numpy(rng.normal(0, 0.02, (T, B, u)).astype(np.float32)).to(DEV)
    md = torch.from_numpy(mask).to(DEV) if mask is not None else None
    ld = N + case.pad
    buf = dict(c=_guarded(N, u, torch.float32), h=_guarded(N, u, tdt))
    if case.save:
        buf["gates"] = _guarded(N, 4 * u, tdt)
    if mask is not None:
        buf["y"] = _guarded(N, u, tdt)
    for name, on in (("hT", case.hT), ("yT", case.yT)):
        if on:
            buf[name] = torch.full((u, ld), SENT, device=DEV, dtype=tdt)
    view = lambda name, cols: buf[name][:N].view(T, B, cols) if name in buf else None      # noqa: E731
    gates, c, h, y = view("gates", 4 * u), view("c", u), view("h", u), view("y", u)
    ws = ops.lstm_rowpar_workspace(T, B, u, DEV)
    xd, wd = xproj.to(DEV).view(T, B, 4 * u), wh_t.to(DEV)
    L = ops.lstm2_fwd_layer(xd, wd, None, None, gates, c, h, buf.get("hT"), y, md, yT=buf.get("yT"), gates_dtype=tdt,
                            xproj_dtype=tdt if case.xb else torch.float32)

    def forward():
        _poison_exchange(ws, T, B, u)
        ops.lstm_rowpar_fwd(T, B, L, keep, ws)
        torch.cuda.synchronize()
        ops.lstm_rowpar_check(ws)

    forward()
    # ---- float64 forward on the same operands; the state fed back is the kernel's 16-bit h (under a mask only h[-1] leaves: r16 of the reference's) ----
    W = wh_t.double().numpy()
    hk = _np64(h)
    ref = L64.forward(W, xproj.double().numpy(), lambda t, hv: hk[t] if (mask is None or t + 1 == T) else r16(hv).double().numpy())
    errs = dict(c=np.abs(_np64(c) - ref["c"]).max() / eps)
    if mask is None:
        errs["h"] = np.abs(hk - ref["h"]).max() / eps
        out16 = h
    else:
        errs["h"] = np.abs(hk[-1] - ref["h"][-1]).max() / eps                     # only the final state leaves through h ...
        assert bool((h[:-1] == SENT).all())                                        # ... and the earlier steps are not written
        yref = r16(ref["h"]).double().numpy() / keep * mask
        errs["y"] = np.abs(_np64(y) - yref).max() / eps
        out16 = y
    if case.save:
        errs["gates"] = np.abs(_np64(gates).reshape(T, B, u, 4) - ref["g"]).max() / eps
    if case.yT:       # y^T[unit][t B + row] = the layer's output
        assert torch.equal(buf["yT"][:, :N].reshape(u, T, B), out16.permute(2, 0, 1))
    if case.hT:       # h^T[unit][(t + 1) B + row] = h[t]; column block 0 (h_{-1}) is the caller's
        hTv = buf["hT"][:, :N].reshape(u, T, B)
        hh = r16(ref["h"]).double().numpy()
        errs["hT"] = np.abs(_np64(hTv[:, 1:]) - np.transpose(hh, (2, 0, 1))[:, :-1]).max() / eps
        assert bool((hTv[:, 0] == SENT).all())
        if mask is None:
            assert torch.equal(hTv[:, 1:], h[:-1].permute(2, 0, 1))
    _report(case_id(case) + " fwd", errs, FWD_BOUNDS)
    for k, v in errs.items():
        assert v < FWD_BOUNDS[k], (k, v)
    for name in ("gates", "c", "h", "y"):
        if name in buf:
            assert bool((buf[name][N] == SENT).all()), name                       # the guard row behind each output
    for name in ("hT", "yT"):
        if name in buf:
            assert bool((buf[name][:, N:] == SENT).all()), name                   # padding columns [T B, ld)
    if not case.save:
        first = {k: v.clone() for k, v in buf.items()}
        forward()
        assert all(torch.equal(buf[k], first[k]) for k in buf)
        return
    # ---- backward on the kernel's own saved tensors ----
    wh_p = wh_t.t().contiguous().to(DEV)                                           # [k][gate-interleaved column]
    buf["dzc"] = _guarded(N, 4 * u, tdt)
    dzc = buf["dzc"][:N].view(T, B, 4 * u)
    if case.layout == "kblock" or not case.bwd:
        buf["dzT"] = torch.full((N // 32, 4 * u, 32), SENT, device=DEV, dtype=tdt)
    elif case.layout == "plain":
        buf["dzT"] = torch.full((4 * u, ld), SENT, device=DEV, dtype=tdt)
    db = torch.zeros(4 * u, device=DEV)
    E = ops.lstm2_bwd_layer(dh, wh_p, gates, c, None, dzc, ops.lstm_seq_bwd_workspace(B, u, DEV), buf.get("dzT"), db, md, gates_dtype=tdt)
    if not case.bwd:
        assert refused
        with pytest.raises(MnnError):
            ops.lstm_rowpar_bwd(T, B, E, keep, ws)                                 # refused on the host: nothing is launched, nothing written
        torch.cuda.synchronize()
        assert bool((buf["dzc"] == SENT).all()) and bool((buf["dzT"] == SENT).all()) and float(db.abs().max()) == 0.0
        return

    def backward():
        _poison_exchange(ws, T, B, u)
        ops.lstm_rowpar_bwd(T, B, E, keep, ws)
        torch.cuda.synchronize()
        ops.lstm_rowpar_check(ws)

    backward()
    berrs = _check_backward(W, gates, c, dh, mask, keep, buf["dzc"], buf.get("dzT"), db, T, B, u, eps, case.layout, case.pad)
    _report(case_id(case) + " bwd", berrs, BWD_BOUNDS)
    for k, v in berrs.items():
        assert v < BWD_BOUNDS[k], (k, v)
    # ---- the same workspace and buffers again: every output bit for bit (db is summed with float atomics) ----
    first = {k: v.clone() for k, v in buf.items()}
    db.zero_()
    forward()
    backward()
    for k in buf:
        assert torch.equal(buf[k], first[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_rowpar_single_wave_backward_on_cluster_forward_tensors(ops, monkeypatch, dt):
    """The fall-back of lstm_cluster_bwd: the saved tensors of ops.lstm_cluster_fwd (B = 768, U = 512, T = 4, keep 0.9) through
    ops.lstm_rowpar_bwd with three row tiles per workgroup (MNN_ROWPAR_MAX_G = 8) -- the single-wave backward a 512-unit layer takes at
    B = 1536 on a device whose clusters are not dealt onto single XCDs -- against the same float64 backward, on the shared workspace."""
    B, T, u, keep = 768, 4, 512, 0.9
    N = T * B
    _set_form(monkeypatch, None, False, False)
    tdt = torch.float16 if dt == "fp16" else torch.bfloat16
    eps = 2.0 ** -10 if dt == "fp16" else 2.0 ** -7
    rng = np.random.default_rng(77)
    r16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(tdt)            # noqa: E731
    wh_t = r16(rng.normal(0, 0.04, (4 * u, u)))
    xproj = r16(rng.normal(0, 1.2, (T, B, u, 4)))
    mask = (rng.random((T, B, u)) < keep).astype(np.uint8)
    dh = torch.from_numpy(rng.normal(0, 0.02, (T, B, u)).astype(np.float32)).to(DEV)
    md = torch.from_numpy(mask).to(DEV)
    gates_f, c_f, h_f, y_f = _guarded(N, 4 * u, tdt), _guarded(N, u, torch.float32), _guarded(N, u, tdt), _guarded(N, u, tdt)
    gates, c, h, y = gates_f[:N].view(T, B, 4 * u), c_f[:N].view(T, B, u), h_f[:N].view(T, B, u), y_f[:N].view(T, B, u)
    hT, yT = torch.zeros((u, N), device=DEV, dtype=tdt), torch.zeros((u, N), device=DEV, dtype=tdt)
    assert ops.lstm_cluster_ok(B, u)
    ws = ops.lstm_rowpar_workspace(T, B, u, DEV)
    L = ops.lstm2_fwd_layer(xproj.to(DEV).view(T, B, 4 * u), wh_t.to(DEV), None, None, gates, c, h, hT, y, md, yT=yT, gates_dtype=tdt, xproj_dtype=tdt)
    ops.lstm_cluster_fwd(T, B, L, keep, ws)
    torch.cuda.synchronize()
    ops.lstm_rowpar_check(ws)
    monkeypatch.setenv("MNN_ROWPAR_MAX_G", "8")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles_per_workgroup(B, u, 8, cus) == 3 and ops.lstm_rowpar_ok(B, u)
    wh_p = wh_t.t().contiguous().to(DEV)
    dzc_f = _guarded(N, 4 * u, tdt)
    dzT = torch.full((N // 32, 4 * u, 32), SENT, device=DEV, dtype=tdt)
    db = torch.zeros(4 * u, device=DEV)
    E = ops.lstm2_bwd_layer(dh, wh_p, gates, c, None, dzc_f[:N].view(T, B, 4 * u), ops.lstm_seq_bwd_workspace(B, u, DEV), dzT, db, md, gates_dtype=tdt)
    _poison_exchange(ws, T, B, u)
    ops.lstm_rowpar_bwd(T, B, E, keep, ws)
    torch.cuda.synchronize()
    ops.lstm_rowpar_check(ws)
    berrs = _check_backward(wh_t.double().numpy(), gates, c, dh, mask, keep, dzc_f, dzT, db, T, B, u, eps, "kblock", 0)
    _report(f"cluster-fwd-S3-u512-{dt}-B768-T4-k0.9 bwd", berrs, BWD_BOUNDS)
    for k, v in berrs.items():
        assert v < BWD_BOUNDS[k], (k, v)
    first = dzc_f.clone()
    db.zero_()
    _poison_exchange(ws, T, B, u)
    ops.lstm_rowpar_bwd(T, B, E, keep, ws)
    torch.cuda.synchronize()
    ops.lstm_rowpar_check(ws)
    assert torch.equal(dzc_f, first) and torch.equal(dzT.permute(0, 2, 1).reshape(N, 4 * u), dzc_f[:N])
    assert bool((gates_f[N] == SENT).all()) and bool((c_f[N] == SENT).all())       # the saved tensors' guard rows, after both kernels
