"""DeviceDataset on a CPU device (the windows by torch indexing) and the driver paths that take it: the same windows, in the same order, with
the same lengths as the NumPy path; the loss ring leaves the accumulator where per-step reads would have; every refusal."""
import math

import numpy as np
import pytest
import torch

from multinn_amd import DeviceDataset, driver
from multinn_amd.driver import LossAccumulator, LossRing, TrainingStats, iter_windows

S, T, P, M = 7, 11, 3, 2
LENGTHS = np.array([11, 0, 1, 4, 5, 9, 11])
BATCH, PIECE = 3, 4


@pytest.fixture(scope="module")
def X():
    return (np.random.default_rng(5).random((S, T, P, M)) < 0.3).astype(np.uint8)


@pytest.fixture(scope="module")
def ds(X):
    return DeviceDataset(X, LENGTHS, device="cpu")


def shuffled_ids():
    return np.random.default_rng(1).permutation(S)


def windows(ids):
    return [w for w in iter_windows(ids, LENGTHS, T, BATCH, PIECE) if w is not None]


def test_surface(X, ds):
    assert ds.shape == (S, T, P, M) and len(ds) == S and ds.nbytes == X.size and ds.device == torch.device("cpu")
    assert ds.lengths.dtype == np.int64 and ds.lengths.tolist() == LENGTHS.tolist()
    full = DeviceDataset(X.astype(bool), device="cpu")
    assert full.lengths.tolist() == [T] * S
    x, ln = full.window(np.arange(S), 0, T)
    assert x.dtype == torch.uint8 and np.array_equal(x.numpy(), X.reshape(S, T, P * M)) and ln.tolist() == [T] * S


def test_upload_in_slabs_of_a_strided_array(X):
    """A staging buffer smaller than the dataset (two songs per slab, then one song when a song is larger than it), from a view with strides."""
    big = np.zeros((S, T + 3, P, M + 1), np.uint8)
    big[:, 1:T + 1, :, :M] = X
    view = big[:, 1:T + 1, :, :M]
    assert not view.flags.c_contiguous
    for slab in (2 * T * P * M, 1):
        d = DeviceDataset(view, LENGTHS, device="cpu", slab_bytes=slab)
        assert np.array_equal(d.window(np.arange(S), 0, T)[0].numpy(), X.reshape(S, T, P * M))


def test_every_window_of_the_toy_set(X, ds):
    ids = shuffled_ids()
    ws = windows(ids)
    assert len(ws) == 7 and {len(w[0]) for w in ws} == {1, 2, 3} and {w[2] for w in ws} == {3, 4}
    for song_ids, j, max_len, len_batch in ws:
        x, ln = ds.window(song_ids, j, max_len)
        assert x.dtype == torch.uint8 and ln.dtype == torch.int32
        assert np.array_equal(x.numpy(), X[song_ids, j:j + max_len].reshape(len(song_ids), max_len, P * M))
        assert ln.tolist() == len_batch.tolist()
        for m in range(M):
            xt, lt = ds.window(song_ids, j, max_len, track=m, ids_dev=torch.from_numpy(song_ids.astype(np.int32)))
            assert np.array_equal(xt.numpy(), X[song_ids, j:j + max_len][..., m]) and lt.tolist() == len_batch.tolist()
    x, ln = ds.window(np.array([1, 3, 3, 6]), 3, 5)                       # lengths that clamp to 0, in between and to Tw; a repeated id
    assert ln.tolist() == [0, 1, 1, 5] and np.array_equal(x.numpy(), X[[1, 3, 3, 6], 3:8].reshape(4, 5, P * M))


def test_window_buffers_are_owned_and_reused(ds):
    a, la = ds.window(np.array([0, 6]), 0, 4)
    b, lb = ds.window(np.array([5, 2]), 4, 4)
    assert a.data_ptr() == b.data_ptr() and la.data_ptr() == lb.data_ptr()


# ---- the driver -------------------------------------------------------------------------------------------------------------------
SCRIPT = [1.5, float("nan"), 0.25, float("inf"), 2.0, float("-inf"), 0.125]        # one loss per window of the toy epoch


class StubGenerator:
    """Records what a step is fed; returns the scripted losses, as tensors except where `host` says a host number."""

    def __init__(self, host=()):
        self.fed, self.host = [], set(host)

    def train_step(self, xb, lb, optimizer, lr):
        k = len(self.fed)
        self.fed.append((xb.clone(), None if lb is None else lb.clone()))
        return SCRIPT[k] if k in self.host else torch.tensor(SCRIPT[k], dtype=torch.float32)

    def build_pianoroll(self, xb, lb, is_train, mode):
        assert (is_train, mode) == (False, "eval")
        self.fed.append((xb.clone(), None if lb is None else lb.clone()))
        self.metrics = {"batch/loss": torch.tensor(0.1 * len(self.fed) + float(xb.sum()), dtype=torch.float32)}


def same_batches(a, b):
    assert len(a) == len(b) > 0
    for (xa, la), (xb, lb) in zip(a, b):
        assert xa.dtype == xb.dtype == torch.uint8 and xa.shape == xb.shape and torch.equal(xa, xb)
        assert (la is None) == (lb is None)
        if la is not None:
            assert la.dtype == lb.dtype == torch.int32 and torch.equal(la, lb)


def run_epoch(X_or_ds, lengths, host=(), **kw):
    gen, acc, stats = StubGenerator(host), LossAccumulator(), TrainingStats()
    mean = driver.train_epoch(gen, X_or_ds, lengths, shuffled_ids(), BATCH, PIECE, None, acc, stats, lr=0.1, device="cpu", **kw)
    return gen, acc, stats, mean


@pytest.mark.parametrize("host", [(), (2, 3), tuple(range(7))])
def test_train_epoch_feeds_the_same_batches_and_accumulates_the_same(X, ds, host):
    g0, a0, s0, m0 = run_epoch(X, LENGTHS, host)
    g1, a1, s1, m1 = run_epoch(ds, LENGTHS, host)
    assert len(g0.fed) == len(SCRIPT)
    same_batches(g0.fed, g1.fed)
    assert any(l is None for _, l in g0.fed) and any(l is not None for _, l in g0.fed)       # full-length and ragged windows both occur
    assert s0.steps == s1.steps == 3
    assert (a0.finite_sum, a0.finite_n, a0.bad) == (a1.finite_sum, a1.finite_n, a1.bad)
    assert a1.bad == {"nan": 1, "+inf": 1, "-inf": 1} and a1.finite_n == 4 and m0 == m1 == a1.loss()
    g2, a2, _, _ = run_epoch(ds, None, host)                                                   # lengths: the dataset's own
    same_batches(g0.fed, g2.fed)
    assert (a0.finite_sum, a0.finite_n, a0.bad) == (a2.finite_sum, a2.finite_n, a2.bad)


def test_accumulation_order_is_step_order(ds):
    """finite_sum is a float sum, so the order counts: losses whose sum depends on it."""
    vals = [1e16, 1.0, -1e16, 1.0, 3.0, 1e-3, 7.0]
    exp = LossAccumulator()
    for v in vals:
        exp.update(float(torch.tensor(v, dtype=torch.float32)))
    for host in ((), (1, 4), (0, 2, 6)):
        acc = LossAccumulator()
        ring = LossRing(lambda v, _: acc.update(v), slots=3)
        for k, v in enumerate(vals):
            ring.put(float(np.float32(v)) if k in host else torch.tensor(v, dtype=torch.float32))
        ring.flush()
        assert (acc.finite_sum, acc.finite_n) == (exp.finite_sum, exp.finite_n)


@pytest.mark.parametrize("drain_every, drains", [(None, 1), (1, 7), (2, 4), (3, 3), (7, 1), (100, 1)])
def test_ring_drains_once_per_epoch_or_every_n_steps(ds, monkeypatch, drain_every, drains):
    sizes, real = [], LossRing.drain

    def spy(self):
        sizes.append(len(self._notes))
        real(self)
    monkeypatch.setattr(LossRing, "drain", spy)
    _, acc, _, _ = run_epoch(ds, LENGTHS, drain_every=drain_every)
    assert len(sizes) == drains == math.ceil(len(SCRIPT) / (drain_every or len(SCRIPT))) and sum(sizes) == len(SCRIPT)
    assert acc.finite_n + acc.num_bad() == len(SCRIPT)


def test_a_full_ring_drains(ds):
    got = []
    ring = LossRing(lambda v, note: got.append((v, note)), slots=2)
    for k in range(5):
        ring.put(torch.tensor(float(k)), note=k)
        assert len(got) == (k + 1) // 2 * 2
    ring.flush()
    ring.flush()
    assert got == [(float(k), k) for k in range(5)]


def test_drain_every_is_refused_off_the_dataset_path(X):
    with pytest.raises(ValueError, match="drain_every"):
        run_epoch(X, LENGTHS, drain_every=2)
    with pytest.raises(ValueError, match="drain_every"):
        driver.evaluate(StubGenerator(), X, LENGTHS, BATCH, PIECE, device="cpu", drain_every=2)
    with pytest.raises(ValueError, match="drain_every"):
        LossRing(lambda v, n: None, drain_every=0)


def test_lengths_beside_a_dataset_must_be_its_own(ds):
    with pytest.raises(ValueError, match="lengths"):
        run_epoch(ds, np.full(S, T))


def test_evaluate_sees_the_same_windows(X, ds):
    g0, g1, g2 = StubGenerator(), StubGenerator(), StubGenerator()
    v0 = driver.evaluate(g0, X, LENGTHS, BATCH, PIECE, device="cpu")
    v1 = driver.evaluate(g1, ds, LENGTHS, BATCH, PIECE)
    v2 = driver.evaluate(g2, ds, None, BATCH, PIECE, drain_every=2)
    same_batches(g0.fed, g1.fed)
    same_batches(g0.fed, g2.fed)
    assert len(g0.fed) == len(windows(np.arange(S))) and v0 == v1 == v2 and math.isfinite(v0)


class StubEncoder:
    num_layers = 2

    def __init__(self):
        self.fed = []

    def build(self, x, is_train, mode):
        self.fed.append((x.clone(), None))

    def train(self, _, lr, layer):
        return None, None, {"batch/loss": torch.tensor(float(self.fed[-1][0].sum()) + layer)}, None, None


@pytest.mark.parametrize("n_enc", [1, M])
def test_pretrain_encoders_sees_the_same_windows(X, ds, n_enc):
    cfg = {"batch_size": BATCH, "piece_size": 1, "learning_rate": 0.1, "epochs": 2}
    e0, e1 = [StubEncoder() for _ in range(n_enc)], [StubEncoder() for _ in range(n_enc)]
    h0 = driver.pretrain_encoders(e0, X, LENGTHS, cfg, beat_size=PIECE, device="cpu")
    h1 = driver.pretrain_encoders(e1, ds, LENGTHS, cfg, beat_size=PIECE)
    for a, b in zip(e0, e1):
        same_batches(a.fed, b.fed)
        assert a.fed[0][0].shape[2] == (P * M if n_enc == 1 else P)
    assert h0 == h1 and sorted(h0) == [(e, l) for e in range(n_enc) for l in range(2)]


def test_numpy_path_is_the_old_path(X, monkeypatch):
    """A NumPy X never meets the dataset code: its windows reach the generator through torch.from_numpy and every loss is read as it comes."""
    seen, real = [], torch.from_numpy

    def spy(a):
        seen.append(a)
        return real(a)
    monkeypatch.setattr(torch, "from_numpy", spy)
    monkeypatch.setattr(DeviceDataset, "window", lambda *a, **k: pytest.fail("a NumPy X was routed to the dataset"))
    monkeypatch.setattr(LossRing, "put", lambda *a, **k: pytest.fail("a NumPy X was routed to the loss ring"))
    gen, acc, _, _ = run_epoch(X, LENGTHS)
    ws = windows(shuffled_ids())
    xs = [a for a in seen if a.dtype == np.uint8]
    assert len(xs) == len(ws) and all(np.array_equal(a, X[w[0], w[1]:w[1] + w[2]]) for a, w in zip(xs, ws))
    assert all(torch.equal(x, real(a)) for (x, _), a in zip(gen.fed, xs))
    assert acc.finite_n == 4
    driver.evaluate(StubGenerator(), X, LENGTHS, BATCH, PIECE, device="cpu")
    driver.pretrain_encoders([StubEncoder()], X, LENGTHS, {"batch_size": BATCH, "piece_size": 1, "learning_rate": 0.1, "epochs": 1}, device="cpu")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad, match", [
    (lambda X: X[0], "rank"), (lambda X: X.reshape(S, T, P * M), "rank"), (lambda X: X.tolist(), "NumPy"),
    (lambda X: X.astype(np.float32), "uint8 or bool"), (lambda X: X.astype(np.int8), "uint8 or bool"), (lambda X: X[:0], "empty")])
def test_refuses_a_wrong_rank_or_dtype(X, bad, match):
    with pytest.raises(ValueError, match=match):
        DeviceDataset(bad(X), device="cpu")


@pytest.mark.parametrize("lengths", [LENGTHS[:-1], np.append(LENGTHS, 3), LENGTHS.astype(np.float64), LENGTHS.reshape(S, 1),
                                     np.where(LENGTHS == 0, -1, LENGTHS), np.where(LENGTHS == 11, 12, LENGTHS)])
def test_refuses_bad_lengths(X, lengths):
    with pytest.raises(ValueError, match="lengths"):
        DeviceDataset(X, lengths, device="cpu")


def test_refuses_a_dataset_beyond_its_share_of_free_memory(X, monkeypatch):
    """Before any upload: nothing but mem_get_info touches the device (there is none here)."""
    asked = []
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (asked.append(device), (2 * X.size - 2, 10 ** 12))[1])
    monkeypatch.setattr(torch, "empty", lambda *a, **k: pytest.fail("allocated before the refusal"))
    with pytest.raises(ValueError, match=rf"{X.size} bytes.*{2 * X.size - 2} bytes free"):
        DeviceDataset(X, LENGTHS, device="cuda:0")
    assert len(asked) == 1
    with pytest.raises(ValueError, match="max_fraction"):
        DeviceDataset(X, LENGTHS, device="cpu", max_fraction=0.0)
    with pytest.raises(ValueError, match="device"):
        DeviceDataset(X, LENGTHS, device="meta")


@pytest.mark.parametrize("ids", [[0, S], [-1, 2], [], [[0, 1]], [0.0, 1.0]])
def test_refuses_song_ids_out_of_range(ds, ids):
    with pytest.raises(ValueError, match="song_ids"):
        ds.window(np.array(ids), 0, 4)
    with pytest.raises(ValueError, match="song_ids"):
        ds.upload_ids(np.array(ids))


def test_refuses_a_window_outside_the_dataset(ds):
    for j, Tw in ((-1, 4), (0, 0), (8, 4), (0, T + 1)):
        with pytest.raises(ValueError, match="window"):
            ds.window(np.array([0, 1]), j, Tw)
    for track in (-1, M):
        with pytest.raises(ValueError, match="track"):
            ds.window(np.array([0, 1]), 0, 4, track=track)
    for ids_dev in (torch.tensor([0, 1]), torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([[0, 1]], dtype=torch.int32)):
        with pytest.raises(ValueError, match="ids_dev"):
            ds.window(np.array([0, 1]), 0, 4, ids_dev=ids_dev)
    with pytest.raises(ValueError, match="song_ids"):                      # the epoch's one upload checks its ids too
        driver.train_epoch(StubGenerator(), ds, None, np.array([0, S]), BATCH, PIECE, None, LossAccumulator(), TrainingStats())


def test_c_abi_refuses_bad_arguments_before_any_device_work(lib):
    """mnn_window_gather's host checks (no GPU here: a call that got past them would fail differently)."""
    ok = dict(X=1 << 20, S=4, T=10, D=6, ids=1 << 21, B=2, j=2, Tw=4, e0=0, es=1, Dout=6, lengths=1 << 22, out=1 << 23, out_len=1 << 24)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.mnn_window_gather(None, a["X"], a["S"], a["T"], a["D"], a["ids"], a["B"], a["j"], a["Tw"], a["e0"], a["es"], a["Dout"], a["lengths"], a["out"],
                                   a["out_len"])
        return rc, lib.mnn_last_error().decode()
    for name in ("S", "T", "D", "B", "Tw", "Dout"):
        for v in (0, -3):
            rc, msg = call(**{name: v})
            assert rc == -1 and "positive" in msg, (name, v, msg)
    for kw in (dict(j=-1), dict(j=7), dict(j=0, Tw=11)):
        rc, msg = call(**kw)
        assert rc == -1 and "window" in msg, (kw, msg)
    for kw in (dict(es=0), dict(e0=-1), dict(e0=1), dict(es=2, Dout=4), dict(es=3, e0=1, Dout=2, D=4), dict(Dout=7)):
        rc, msg = call(**kw)
        assert rc == -1 and "features" in msg, (kw, msg)
    for name in ("X", "ids", "out"):
        rc, msg = call(**{name: None})
        assert rc == -1 and "NULL" in msg, (name, msg)
    rc, msg = call(lengths=None)
    assert rc == -1 and "out_len needs lengths" in msg
