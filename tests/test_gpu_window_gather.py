"""mnn_window_gather (window.hip) against torch indexing, bit for bit, at the shapes where it can go wrong: every vector width and a
base that lowers it, partial and several chunks per row, more rows than one grid column, the strided track gather, clipped lengths, offsets
past 2^31 bytes -- and one epoch of driver.train_epoch on a DeviceDataset."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64


def random_bytes(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=g)


def gather(X, ids, j, Tw, lengths=None, track=None, tracks=1, skew=0):
    """ops.window_gather into a guarded buffer that starts `skew` bytes off a 16-byte boundary: (out, out_len); the guards must stay untouched."""
    from multinn_amd import ops
    B, Dout = ids.numel(), X.shape[2] // (tracks if track is not None else 1)
    n = B * Tw * Dout
    flat = torch.full((GUARD + skew + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    out = flat[GUARD + skew:GUARD + skew + n].view(B, Tw, Dout)
    assert out.data_ptr() % 16 == skew % 16
    ln_flat = torch.full((B + 2,), -77, dtype=torch.int32, device=DEV)
    ops.window_gather(X, ids, j, Tw, out, lengths=lengths, out_len=None if lengths is None else ln_flat[1:B + 1], track=track, tracks=tracks)
    assert bool((flat[:GUARD + skew] == 0xA5).all()) and bool((flat[GUARD + skew + n:] == 0xA5).all()), "wrote outside the window"
    assert ln_flat[0] == -77 and ln_flat[-1] == -77
    return out, ln_flat[1:B + 1]


@pytest.mark.parametrize("D", [1, 7, 12, 16, 440])                        # vector widths 1, 1, 4, 16, 8
def test_joint_window_every_width(D):
    S, T = 5, 9
    X = random_bytes((S, T, D), D)
    lengths = torch.tensor([T, 0, 1, 4, 6], dtype=torch.int32, device=DEV)
    for B in (1, 257):                                                    # 257 rows over 5 songs: repeated ids
        ids = torch.randint(0, S, (B,), generator=torch.Generator().manual_seed(B), dtype=torch.int32).to(DEV)
        for j, Tw in ((0, 1), (3, 1), (3, 4), (5, 4), (0, T), (T - 1, 1)):   # j = 0, odd, T - Tw; Tw = 1 (a row of D bytes: below 16) and T
            out, ln = gather(X, ids, j, Tw, lengths)
            assert torch.equal(out, X[ids.long(), j:j + Tw]), (B, j, Tw)
            assert torch.equal(ln, (lengths[ids.long()] - j).clamp(0, Tw)), (B, j, Tw)   # clamps to 0, to Tw, and in between
            assert {0, Tw} <= set(ln.tolist()) or B == 1
    out, _ = gather(X, ids, 2, 3)                                         # without lengths
    assert torch.equal(out, X[ids.long(), 2:5])


@pytest.mark.parametrize("D, T, j, Tw", [(1, 2500, 1, 2499), (16, 1030, 3, 1027), (440, 41, 1, 40), (12, 2051, 0, 2051)])
def test_rows_of_several_chunks(D, T, j, Tw):
    """A row longer than one workgroup's 1024 vectors, its last chunk partial."""
    S = 3
    X = random_bytes((S, T, D), T)
    ids = torch.tensor([2, 0, 2, 1], dtype=torch.int32, device=DEV)
    assert Tw * D // np.gcd(D, 16) > 1024 and (Tw * D // np.gcd(D, 16)) % 1024 != 0
    out, _ = gather(X, ids, j, Tw)
    assert torch.equal(out, X[ids.long(), j:j + Tw])


@pytest.mark.parametrize("skew_x, skew_out", [(0, 8), (8, 0), (4, 0), (0, 2), (1, 0), (0, 3), (4, 8)])
def test_a_base_off_16_bytes_lowers_the_vector_width(skew_x, skew_out):
    """D = 16 allows 16-byte vectors only if both bases do: a dataset or a window that starts elsewhere is copied with narrower ones."""
    S, T, D = 4, 7, 16
    flat = random_bytes((16 + S * T * D,), skew_x + 16 * skew_out)
    X = flat[skew_x:skew_x + S * T * D].view(S, T, D)
    assert X.data_ptr() % 16 == skew_x
    ids = torch.tensor([3, 1, 1, 0, 2], dtype=torch.int32, device=DEV)
    out, _ = gather(X, ids, 2, 5, skew=skew_out)
    assert torch.equal(out, X[ids.long(), 2:7])


def test_every_track_of_a_roll():
    S, T, P, M = 6, 9, 5, 3
    X = random_bytes((S, T, P * M), 9)
    lengths = torch.tensor([9, 0, 3, 5, 8, 1], dtype=torch.int32, device=DEV)
    for B in (1, 257):
        ids = torch.randint(0, S, (B,), generator=torch.Generator().manual_seed(B), dtype=torch.int32).to(DEV)
        for j, Tw in ((0, 1), (1, 4), (4, 5), (0, T)):
            for m in range(M):
                out, ln = gather(X, ids, j, Tw, lengths, track=m, tracks=M)
                assert torch.equal(out, X.view(S, T, P, M)[ids.long(), j:j + Tw, :, m]), (B, j, Tw, m)
                assert torch.equal(ln, (lengths[ids.long()] - j).clamp(0, Tw))


def test_offsets_past_2_31_bytes():
    """A dataset of 2.2e9 bytes: the last songs lie behind byte 2^31."""
    S, T, D = 2200, 1000, 1000
    assert (S - 2) * T * D > 2 ** 31
    X = torch.empty((S, T, D), dtype=torch.uint8, device=DEV)
    for s in (0, S - 2, S - 1):
        X[s] = random_bytes((T, D), s)
    ids = torch.tensor([S - 1, 0, S - 2, S - 1], dtype=torch.int32, device=DEV)
    lengths = torch.full((S,), T, dtype=torch.int32, device=DEV)
    lengths[S - 2] = 995
    for j, Tw in ((T - 3, 3), (991, 8), (0, 2)):
        out, ln = gather(X, ids, j, Tw, lengths)
        assert torch.equal(out, X[ids.long(), j:j + Tw])
        assert ln.tolist() == [Tw, Tw, max(0, min(995 - j, Tw)), Tw]
        out, _ = gather(X, ids, j, Tw, track=1, tracks=2)
        assert torch.equal(out, X.view(S, T, D // 2, 2)[ids.long(), j:j + Tw, :, 1])


def test_dataset_windows_on_the_device():
    """DeviceDataset on the ROCm device against its CPU twin (torch indexing), over every window of a small ragged epoch."""
    from multinn_amd import DeviceDataset
    from multinn_amd.driver import iter_windows
    R = np.random.default_rng(3)
    Xh = (R.random((13, 21, 5, 3)) < 0.3).astype(np.uint8)
    lengths = R.integers(0, 22, 13)
    a, b = DeviceDataset(Xh, lengths, device=DEV, slab_bytes=4 * 21 * 15), DeviceDataset(Xh, lengths, device="cpu")
    assert a.device == torch.device(DEV) and a.nbytes == Xh.size
    ids_dev = a.upload_ids(np.arange(13))
    for w in iter_windows(np.arange(13), lengths, 21, 4, 8):
        if w is None:
            continue
        for track in (None, 0, 2):
            xa, la = a.window(w[0], w[1], w[2], track=track)
            xb, lb = b.window(w[0], w[1], w[2], track=track)
            assert torch.equal(xa.cpu(), xb) and torch.equal(la.cpu(), lb) and la.tolist() == w[3].tolist()
    xa, _ = a.window(np.arange(4, 9), 2, 6, ids_dev=ids_dev[4:9])            # a slice of one upload
    assert torch.equal(xa.cpu(), b.window(np.arange(4, 9), 2, 6)[0])


def test_train_epoch_on_a_device_dataset(monkeypatch):
    """Two epochs of driver.train_epoch on a small RnnNade (eager first occurrences, then captured full-length and ragged replays): the step
    counter ends where the NumPy run's does, and the losses drained from the ring are, bit for bit, the loss tensors as each step returned
    them.  (Trajectories of two runs are not compared: the NADE backward's float atomics make even two NumPy runs differ in the last bits.)"""
    from multinn_amd import RnnNade, AdamOptimizer, DeviceDataset, driver
    from multinn_amd.driver import train_epoch, LossAccumulator, TrainingStats
    R = np.random.default_rng(5)
    X = (R.random((24, 12, 8, 2)) < .2).astype(np.uint8)
    lengths = np.full(24, 12)
    lengths[5] = 7                                               # one ragged song: its late window is a ragged step
    ids = np.arange(24)

    class Recording(LossAccumulator):
        def clear(self):
            super().clear()
            self.seen = []

        def update(self, loss):
            self.seen.append(float(loss))
            super().update(loss)

    def epochs(data, lens, wrap=lambda gen: None):
        gen = RnnNade(16, 16, [128, 128], keep_prob=0.9, precision="bf16", seed=2)
        gen._materialize(16)
        wrap(gen)
        opt, stats, accs = AdamOptimizer(0.01), TrainingStats(), []
        for _ in range(2):
            accs.append(Recording())
            train_epoch(gen, data, lens, ids, 8, 4, opt, accs[-1], stats, lr=0.01, device=DEV)
        gen.check()
        return gen, stats, accs

    g0, s0, a0 = epochs(X, lengths)
    returned = []

    def cloning(step):
        def wrapped(*a, **k):
            loss = step(*a, **k)
            returned.append(loss.clone())                        # the loss as the step returned it, before anything else runs
            return loss
        return wrapped

    def wrap_eager(gen):
        gen.train_step = cloning(gen.train_step)
    real_captured = driver._captured_step

    def captured(*a, **k):
        run = real_captured(*a, **k)
        return None if run is None else cloning(run)
    monkeypatch.setattr(driver, "_captured_step", captured)
    drains, real_drain = [], driver.LossRing.drain
    monkeypatch.setattr(driver.LossRing, "drain", lambda self: (drains.append(len(self._notes)), real_drain(self))[1])
    g1, s1, a1 = epochs(DeviceDataset(X, lengths, device=DEV), None, wrap_eager)
    n = len(a0[0].seen)
    assert n == 9 and [len(a.seen) for a in a0 + a1] == [n] * 4
    assert g1.store.step == g0.store.step == 2 * n and int(g1.store.step_dev) == int(g0.store.step_dev) and s1.steps == s0.steps == 6
    kinds = lambda g: sorted((k[0], k[-1]) for k in g._step_graphs)
    assert kinds(g1) == kinds(g0) and {k[-1] for k in g1._step_graphs} == {"full", "ragged"}     # the same windows were captured and replayed
    assert drains == [n, n]                                      # one read-back per epoch
    seen = a1[0].seen + a1[1].seen
    assert len(returned) == 2 * n and all(np.isfinite(seen))
    assert seen == [float(t) for t in returned]
