"""The grouped optimiser launches (csrc/opt_multi.hip: mnn_sumsq_multi, mnn_clip_adam_step_multi, mnn_step_increment_multi) against the
per-store launches they replace, bit for bit, and mnn_segments_copy -- the pack and the unpack of training.GradArena.  In-process, through
`ops`; every buffer a job touches lies between guard words."""
import ctypes as C
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, SENTINEL = 8, -777.25
BIG = 2048 * 256 + 5                    # more than 2048 workgroups of 256: the job's grid-stride loop wraps
SIZES = [1, 3, 4, 255, 256, 257, 1025, BIG]
MISALIGNED = 6                          # this job's four buffers are views offset by one float (n = 1025: five workgroups on the scalar path)
STEPS = [0, 5, 1000]
LR, B1, B2, EPS, GROW = 0.01, 0.9, 0.999, 1e-4, 200


def guarded(values, offset=0):
    """values inside a buffer of sentinels: (buffer, view); offset floats off the allocation's 16-byte grid."""
    n = values.numel()
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + n]
    view.copy_(values)
    return buf, view


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + view.numel():] == SENTINEL).all())


def make_state(njobs, seed=0, sizes=None, ls_all=False):
    """A list of jobs (ops' dicts, plus their guarded buffers under "bufs")."""
    gen = torch.Generator().manual_seed(seed)
    jobs = []
    for j in range(njobs):
        n = (sizes or SIZES)[j % len(sizes or SIZES)]
        off = 1 if (j == MISALIGNED or (sizes is not None and j == 0)) else 0
        vals = dict(theta=torch.randn(n, generator=gen), grad=torch.randn(n, generator=gen) * 1e-2, m=torch.randn(n, generator=gen) * 1e-2,
                    v=torch.rand(n, generator=gen) * 1e-4)
        job, bufs = {}, {}
        for k, t in vals.items():
            bufs[k], job[k] = guarded(t, off)
        job["step_dev"] = torch.tensor([STEPS[j % 3]], device=DEV, dtype=torch.int32)
        job["skipped"] = torch.zeros(1, device=DEV, dtype=torch.int32)
        if ls_all or j % 4 != 3:                        # every fourth job has no dynamic loss scale
            job["ls_dyn"] = torch.tensor([0.25, 4.0], device=DEV)
            job["ls_good"] = torch.tensor([GROW - 1 - j % 2], device=DEV, dtype=torch.int32)       # even jobs double their multiplier at this step
        else:
            job["ls_dyn"] = job["ls_good"] = None
        job["bufs"] = bufs
        jobs.append(job)
    return jobs


def true_sumsq(jobs):
    return sum(float((j["grad"].double() ** 2).sum()) for j in jobs)


def per_store_step(jobs, sumsq, clip, sgd):
    from multinn_amd import ops
    for j in jobs:
        ops.clip_adam_step(j["theta"], j["grad"], j["m"], j["v"], sumsq, clip, LR, B1, B2, EPS, 1, sgd, j["step_dev"], j["skipped"])
        ops.step_increment(j["step_dev"], sumsq, clip, j["ls_dyn"], j["ls_good"], GROW)


def grouped_step(jobs, sumsq, clip, sgd):
    from multinn_amd import ops
    ops.clip_adam_step_multi(jobs, sumsq, clip, LR, B1, B2, EPS, sgd)
    ops.step_increment_multi(jobs, sumsq, clip, GROW)


def assert_same(got, want):
    for j, (a, b) in enumerate(zip(got, want)):
        for k in ("theta", "grad", "m", "v"):
            assert torch.equal(a["bufs"][k], b["bufs"][k]), (j, k)
            assert guards_intact(a["bufs"][k], a[k]), (j, k)
        for k in ("step_dev", "skipped", "ls_dyn", "ls_good"):
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (j, k, a[k], b[k])


@pytest.mark.parametrize("binding", [True, False])
@pytest.mark.parametrize("sgd", [False, True])
@pytest.mark.parametrize("njobs", [1, 9, 16, 17])
def test_grouped_launches_equal_per_store_launches(njobs, sgd, binding):
    # one job: BIG off the 16-byte grid, so the scalar loop of all its 2048 workgroups wraps; more: BIG on the vector path (sgd: scalar, wraps)
    sizes = [BIG] if njobs == 1 else None
    a, b = make_state(njobs, 1, sizes), make_state(njobs, 1, sizes)
    gn = math.sqrt(true_sumsq(a))
    clip = gn * (0.5 if binding else 10.0)
    sumsq = torch.tensor([gn * gn], device=DEV)         # ONE word for both sides
    before = [j["theta"].clone() for j in a]
    grouped_step(a, sumsq, clip, sgd)
    per_store_step(b, sumsq, clip, sgd)
    torch.cuda.synchronize()
    assert_same(a, b)
    assert all(not torch.equal(j["theta"], t) for j, t in zip(a, before))              # and a step was taken
    assert [int(j["step_dev"]) for j in a] == [STEPS[i % 3] + 1 for i in range(njobs)]
    assert all(int(j["skipped"]) == 0 for j in a)


def test_sumsq_multi_accumulates_the_float64_sum():
    """rtol 1e-5: at most ~50 fused multiply-adds chain per lane at these sizes, then a tree and <= 256 atomics per job -- a few 1e-6."""
    from multinn_amd import ops
    jobs = make_state(17, 2)
    out = torch.tensor([3.5], device=DEV)
    ops.sumsq_multi(jobs, out)
    want = 3.5 + true_sumsq(jobs)
    assert abs(float(out) - want) <= 1e-5 * want, (float(out), want)
    for j in jobs:
        assert guards_intact(j["bufs"]["grad"], j["grad"])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_norm_skips_every_job(bad):
    from multinn_amd import ops
    a, b = make_state(9, 3, ls_all=True), make_state(9, 3, ls_all=True)
    for jobs in (a, b):
        jobs[4]["grad"][7] = bad
    sumsq = torch.zeros(1, device=DEV)
    ops.sumsq_multi(a, sumsq)
    assert not math.isfinite(float(sumsq))
    grouped_step(a, sumsq, 5.0, False)
    torch.cuda.synchronize()
    for j, (x, y) in enumerate(zip(a, b)):              # b: the untouched twin
        for k in ("theta", "m", "v"):
            assert torch.equal(x["bufs"][k], y["bufs"][k]), (j, k)
        assert int(x["skipped"]) == 1 and int(x["step_dev"]) == STEPS[j % 3]
        assert float(x["ls_dyn"][0]) == 0.125 and float(x["ls_dyn"][1]) == 8.0 and int(x["ls_good"]) == 0
    per_store_step(b, sumsq, 5.0, False)                # ... and the per-store launches leave the same
    for j, (x, y) in enumerate(zip(a, b)):
        for k in ("theta", "m", "v"):
            assert torch.equal(x["bufs"][k], y["bufs"][k]), (j, k)
        for k in ("step_dev", "skipped", "ls_dyn", "ls_good"):
            assert torch.equal(x[k], y[k]), (j, k)


def test_segments_copy_packs_and_unpacks_bit_for_bit():
    from multinn_amd import ops
    from multinn_amd.training import GradArena
    gen = torch.Generator().manual_seed(4)
    sizes = [1, 5, 1025, 4, 70001]
    bufs, grads = zip(*[guarded(torch.randn(n, generator=gen), 1 if i == 2 else 0) for i, n in enumerate(sizes)])      # segment 2 misaligned
    stores = [types.SimpleNamespace(grad=g) for g in grads]
    layout = GradArena(stores)
    assert all(o % 4 == 0 for o in layout.offsets) and layout.flat.numel() % 4 == 0
    abuf, arena = guarded(torch.zeros(layout.flat.numel()))
    want = [g.clone() for g in grads]
    ops.segments_copy([(g, arena[o:o + n], n) for g, o, n in zip(grads, layout.offsets, sizes)])
    gap = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    for o, n, w in zip(layout.offsets, sizes, want):
        assert torch.equal(arena[o:o + n], w)
        gap[o:o + n] = False
    assert int(gap.sum()) > 0 and bool((arena[gap] == 0).all())
    assert guards_intact(abuf, arena)
    for g in grads:
        g.fill_(1.0)
    ops.segments_copy([(arena[o:o + n], g, n) for g, o, n in zip(grads, layout.offsets, sizes)])
    for b, g, w in zip(bufs, grads, want):
        assert torch.equal(g, w) and guards_intact(b, g)
    # the same through GradArena's own buffer
    layout.pack()
    for g in grads:
        g.zero_()
    layout.unpack()
    assert all(torch.equal(g, w) for g, w in zip(grads, want))
    assert all(torch.equal(layout.segment(i), w) for i, w in enumerate(want))
    one = GradArena(stores[:1])
    assert one.single and one.flat is grads[0]


def test_captured_step_replays_read_counter_and_loss_scale_on_the_device():
    """Two jobs of one workgroup each in the reduction: the norm word is 0 + a + b in either order, so eager and replayed steps see the same
    word and must agree bit for bit -- step count (Adam's bias correction) and loss scale included."""
    from multinn_amd import ops
    from multinn_amd.common import graph_capture
    sizes = [1000, 257]
    a, b = make_state(2, 5, sizes, ls_all=True), make_state(2, 5, sizes, ls_all=True)
    clip = 0.5 * math.sqrt(true_sumsq(a))

    def step(jobs, word):
        tables = ops.opt_job_tables(jobs)               # validated and built once for the three launches (training.compute_gradients_multi)
        ops.fill(word, 0.0)
        ops.sumsq_multi(tables, word)
        grouped_step(tables, word, clip, False)

    wb = torch.empty(1, device=DEV)
    for _ in range(2):
        step(b, wb)
    wa = torch.empty(1, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        step(a, wa)
    assert int(a[0]["step_dev"]) == STEPS[0]                        # the capture executed nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert_same(a, b)
    assert [int(j["step_dev"]) for j in a] == [STEPS[0] + 2, STEPS[1] + 2]
    assert float(a[0]["ls_dyn"][0]) == 0.5 and float(a[1]["ls_dyn"][0]) == 0.5          # each doubled once, at its 200th good step


def test_argument_refusals():
    from multinn_amd import _lib
    t = torch.zeros(8, device=DEV)
    step = torch.zeros(1, device=DEV, dtype=torch.int32)
    word = torch.zeros(1, device=DEV)

    def table(count, **over):
        arr = (_lib.OptJob * max(count, 1))()
        for a in arr:
            a.theta = a.grad = a.m = a.v = t.data_ptr()
            a.n, a.step_dev = 8, step.data_ptr()
            for k, val in over.items():
                setattr(a, k, val)
        return arr

    def clip(count, arr):
        _lib.call("mnn_clip_adam_step_multi", None, count, arr, C.c_void_p(word.data_ptr()), 5.0, LR, B1, B2, EPS, 0)

    for count in (0, 17):
        with pytest.raises(_lib.MnnError, match="jobs"):
            clip(count, table(count))
        with pytest.raises(_lib.MnnError, match="jobs"):
            _lib.call("mnn_sumsq_multi", None, count, table(count), C.c_void_p(word.data_ptr()))
        with pytest.raises(_lib.MnnError, match="jobs"):
            _lib.call("mnn_step_increment_multi", None, count, table(count), C.c_void_p(word.data_ptr()), 5.0, GROW)
        with pytest.raises(_lib.MnnError, match="segments"):
            _lib.call("mnn_segments_copy", None, count, (_lib.CopySeg * max(count, 1))())
    with pytest.raises(_lib.MnnError, match="step_dev"):
        clip(2, table(2, step_dev=None))
    with pytest.raises(_lib.MnnError, match="step_dev"):
        _lib.call("mnn_step_increment_multi", None, 2, table(2, step_dev=None), C.c_void_p(word.data_ptr()), 5.0, GROW)
    with pytest.raises(_lib.MnnError, match="n > 0"):
        clip(2, table(2, n=0))
    with pytest.raises(_lib.MnnError, match="grow_after"):
        _lib.call("mnn_step_increment_multi", None, 1, table(1, ls_dyn=t.data_ptr(), ls_good=step.data_ptr()), C.c_void_p(word.data_ptr()), 5.0, 0)
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0 and int(step) == 0             # nothing was launched
