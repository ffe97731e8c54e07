"""Transposition augmentation on the host: data.transpose_rolls / pitch_extents / Transpose (what the NumPy path runs and the kernels are
compared against), the DeviceDataset on a CPU device, and the driver paths that take `augment=`: both inputs feed the step the same bytes,
nothing changes without it, validation is never transposed, the global np.random stream is left alone; every refusal."""
import numpy as np
import pytest
import torch

from multinn_amd import DeviceDataset, driver
from multinn_amd.data import Transpose, moving_bits, pitch_extents, transpose_rolls
from multinn_amd.driver import LossAccumulator, TrainingStats, iter_windows


def by_loops(x, shifts, moving):
    """The semantics, literally: out[b, t, p, m] = x[b, t, p - shifts[b], m] on a moving track where that pitch exists, else 0."""
    B, Tw, P, M = x.shape
    out = np.zeros_like(x)
    for b in range(B):
        for p in range(P):
            for m in range(M):
                q = p - int(shifts[b]) if m in moving else p
                if 0 <= q < P:
                    out[b, :, p, m] = x[b, :, q, m]
    return out


@pytest.fixture(scope="module")
def rolls():
    return np.random.default_rng(11).integers(0, 256, (2, 3, 7, 3), dtype=np.uint8)


@pytest.mark.parametrize("moving", [(0, 1, 2), (1,), (2, 0), ()])
def test_transpose_rolls_against_a_triple_loop(rolls, moving):
    for shifts in ([0, 0], [1, -1], [3, -6], [6, 2], [-2, 5]):
        got = transpose_rolls(rolls, np.array(shifts), moving)
        assert got.dtype == rolls.dtype and got.shape == rolls.shape and np.array_equal(got, by_loops(rolls, shifts, moving)), shifts
    assert not np.shares_memory(transpose_rolls(rolls, np.array([0, 0]), moving), rolls)


def test_shift_zero_and_all_tracks_fixed_are_the_identity(rolls):
    assert np.array_equal(transpose_rolls(rolls, np.array([0, 0]), (0, 1, 2)), rolls)
    assert np.array_equal(transpose_rolls(rolls, np.array([3, -2]), ()), rolls)


@pytest.mark.parametrize("s", [7, -7, 8, -100, 2 ** 31 - 1, -2 ** 31])
def test_a_shift_of_the_whole_axis_or_more_leaves_zeros_on_the_moving_tracks(rolls, s):
    got = transpose_rolls(rolls, np.array([s, 0], np.int64), (0, 2))
    assert not got[0][..., [0, 2]].any() and np.array_equal(got[0][..., 1], rolls[0][..., 1]) and np.array_equal(got[1], rolls[1])


def test_pitch_stride_scales_the_shift(rolls):
    x = np.random.default_rng(2).integers(0, 2, (2, 3, 12, 2), dtype=np.uint8)
    assert np.array_equal(transpose_rolls(x, np.array([1, -2]), (1,), pitch_stride=3), transpose_rolls(x, np.array([3, -6]), (1,)))


def test_transpose_rolls_refusals(rolls):
    for shifts in (np.array([1]), np.array([1.0, 2.0]), np.array([[1, 2]])):
        with pytest.raises(ValueError, match="shifts"):
            transpose_rolls(rolls, shifts, (1,))
    for moving in ((3,), (-1,), (1, 1)):
        with pytest.raises(ValueError, match="moving_tracks"):
            transpose_rolls(rolls, np.array([0, 0]), moving)
    with pytest.raises(ValueError, match="shape"):
        transpose_rolls(rolls[0], np.array([0, 0, 0]), (1,))


# ---- extents --------------------------------------------------------------------------------------------------------------------------
P_H, M_H, T_H = 6, 3, 5


def hand_made_songs():
    """(X [S, T, P, M], lengths, expected lo, expected hi) with track 0 fixed: a note at p = 0; at p = P - 1; at both ends; a note on the fixed
    track only; a note only behind the song's length; an empty song; a song of length 0; notes inside."""
    X = np.zeros((8, T_H, P_H, M_H), np.uint8)
    lengths = np.array([T_H, T_H, T_H, T_H, 2, T_H, 0, 4])
    X[0, 1, 0, 1] = 1
    X[1, 4, P_H - 1, 2] = 1
    X[2, 0, 0, 2] = X[2, 3, P_H - 1, 1] = 1
    X[3, 2, 3, 0] = 1
    X[4, 2, 3, 1] = X[4, 4, 0, 2] = 1
    X[6, 0, 2, 1] = 1
    X[7, 3, 2, 1] = X[7, 0, 4, 2] = 200
    X[7, 4, 5, 1] = X[7, 1, 0, 0] = 1
    return X, lengths, [0, P_H - 1, 0, P_H, P_H, P_H, P_H, 2], [0, P_H - 1, P_H - 1, -1, -1, -1, -1, 4]


def test_pitch_extents_on_hand_made_songs():
    X, lengths, lo_exp, hi_exp = hand_made_songs()
    lo, hi = pitch_extents(X, lengths, (1, 2))
    assert lo.dtype == hi.dtype == np.int64 and lo.tolist() == lo_exp and hi.tolist() == hi_exp
    lo, hi = pitch_extents(X, None, (1, 2))                      # every step counts: the notes behind the lengths are seen
    assert (lo[4], hi[4], lo[6], hi[6], lo[7], hi[7]) == (0, 3, 2, 2, 2, 5)
    lo, hi = pitch_extents(X, lengths, (0,))
    assert (lo[3], hi[3], lo[7], hi[7], lo[0], hi[0]) == (3, 3, 0, 0, P_H, -1)
    lo, hi = pitch_extents(X, lengths, ())
    assert lo.tolist() == [P_H] * 8 and hi.tolist() == [-1] * 8
    ds = DeviceDataset(X, lengths, device="cpu")
    for tracks in ((1, 2), (2, 1), (0,)):
        a, b = ds.extents(tracks), pitch_extents(X, lengths, tracks)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert ds.extents((1, 2))[0] is ds.extents((2, 1))[0]         # computed once per set of tracks


# ---- Transpose ------------------------------------------------------------------------------------------------------------------------
def test_no_note_is_lost_in_any_epoch():
    S, T, P, M, K = 6, 20, 12, 3, 5
    X = (np.random.default_rng(4).random((S, T, P, M)) < 0.06).astype(np.uint8)
    X[0] = 0                                                     # an empty song
    X[1, :, :2] = X[1, :, -3:] = 0                               # room below and above
    X[2, :, 1:] = 0                                              # notes at p = 0 only
    X[3:5, :, :3] = X[3:5, :, -4:] = 0                           # some room; song 5 as drawn (dense enough to reach both ends)
    aug = Transpose(K, fixed_tracks=(0,))
    moving = aug.bind(P, M)
    assert moving == (1, 2)
    ext = pitch_extents(X, None, moving)
    counts, drawn = X.sum(axis=(1, 2)), []
    for epoch in range(1, 11):
        sh = aug.shifts(ext, epoch)
        assert sh.dtype == np.int32 and sh.shape == (S,) and np.abs(sh).max() <= K
        out = transpose_rolls(X, sh, moving)
        assert np.array_equal(out.sum(axis=(1, 2)), counts), epoch
        assert np.array_equal(out[..., 0], X[..., 0])
        drawn.append(sh)
    drawn = np.array(drawn)
    assert (drawn[:, 2] >= 0).all() and (drawn[:, 2] > 0).any()     # clipped below, free above
    assert (drawn != 0).any(axis=0)[:5].all() and len({tuple(r) for r in drawn.tolist()}) > 5
    assert (drawn < 0).any() and (drawn > 0).any()


def test_shifts_depend_on_seed_epoch_and_song_alone():
    S, P = 9, 24
    ext = (np.full(S, 10), np.full(S, 13))
    a, b = Transpose(6, seed=3), Transpose(6, seed=3)
    assert np.array_equal(a.shifts(ext, 4, P), b.shifts(ext, 4, P))
    assert not np.array_equal(a.shifts(ext, 4, P), a.shifts(ext, 5, P))
    assert not np.array_equal(a.shifts(ext, 4, P), Transpose(6, seed=4).shifts(ext, 4, P))
    raw = np.random.Generator(np.random.PCG64([3, 4])).integers(-6, 7, size=S)
    assert np.array_equal(a.shifts(ext, 4, P), raw)               # nothing to clip here: the draw itself
    tight = (np.full(S, 2), np.full(S, 22))
    assert np.array_equal(a.shifts(tight, 4, P), np.clip(raw, -2, 1))
    empty = (np.full(S, P), np.full(S, -1))
    assert np.array_equal(a.shifts(empty, 4, P), raw)             # a song without a pitched note keeps its draw
    with pytest.raises(ValueError, match="pitch axis"):
        Transpose(6).shifts(ext, 1)


def test_the_global_stream_is_not_touched_by_a_draw():
    np.random.seed(77)
    before = np.random.get_state()[1].copy()
    Transpose(3).shifts((np.full(4, 5), np.full(4, 6)), 1, 12)
    assert np.array_equal(np.random.get_state()[1], before)


def test_pitch_stride_moves_whole_semitones_only():
    S, P, n = 40, 36, 3                                           # 12 semitones of 3 positions
    R = np.random.default_rng(8)
    lo = R.integers(0, 18, S)
    hi = lo + R.integers(0, 18, S)
    aug = Transpose(4, pitch_stride=n)
    aug.bind(P, 2)
    seen = set()
    for epoch in range(1, 6):
        sh = aug.shifts((lo, hi), epoch)
        assert (sh % n == 0).all() and (lo + sh >= 0).all() and (hi + sh <= P - 1).all() and np.abs(sh).max() <= 4 * n
        one = Transpose(4, pitch_stride=1).shifts((lo // n, hi // n), epoch, P // n)        # the same songs seen in semitones
        assert np.array_equal(sh, one * n)
        seen |= set(sh.tolist())
    assert len(seen) > 4


@pytest.mark.parametrize("kw, match", [
    (dict(max_shift=0), "max_shift"), (dict(max_shift=-1), "max_shift"), (dict(max_shift=2.0), "max_shift"), (dict(max_shift=True), "max_shift"),
    (dict(max_shift="3"), "max_shift"), (dict(max_shift=2, pitch_stride=0), "pitch_stride"), (dict(max_shift=2, pitch_stride=1.5), "pitch_stride"),
    (dict(max_shift=2, pitch_stride=True), "pitch_stride"), (dict(max_shift=2, fixed_tracks=(0, 0)), "fixed_tracks"),
    (dict(max_shift=2, fixed_tracks=(-1,)), "fixed_tracks"), (dict(max_shift=2, fixed_tracks=(0.0,)), "fixed_tracks"),
    (dict(max_shift=2, fixed_tracks=(True,)), "fixed_tracks")])
def test_transpose_refuses_at_construction(kw, match):
    with pytest.raises(ValueError, match=match):
        Transpose(**kw)


@pytest.mark.parametrize("kw, PM, match", [
    (dict(max_shift=12), (12, 3), "max_shift"), (dict(max_shift=4, pitch_stride=3), (12, 3), "max_shift"),
    (dict(max_shift=2, fixed_tracks=(3,)), (12, 3), "fixed_tracks"), (dict(max_shift=2), (12, 33), "32 tracks"),
    (dict(max_shift=1, pitch_stride=5), (12, 3), "pitch_stride")])
def test_transpose_refuses_rolls_it_does_not_fit(kw, PM, match):
    with pytest.raises(ValueError, match=match):
        Transpose(**kw).bind(*PM)
    X = np.zeros((2, 4) + PM, np.uint8)
    with pytest.raises(ValueError, match=match):                  # before any work: nothing is fed
        driver.train_epoch(Stub(), X, np.full(2, 4), np.arange(2), 2, 4, None, LossAccumulator(), TrainingStats(), device="cpu", augment=Transpose(**kw))


def test_boundary_arguments_are_accepted():
    assert Transpose(11).bind(12, 3) == (0, 1, 2)
    assert Transpose(3, pitch_stride=3).bind(12, 32) == tuple(range(32))
    assert Transpose(np.int64(2), fixed_tracks=[np.int32(1)]).bind(12, 3) == (0, 2)
    assert Transpose(2, fixed_tracks=(0, 1, 2)).bind(12, 3) == ()
    assert moving_bits((1, 4), 5) == 0b10010 and moving_bits((), 5) == 0


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
S, T, P, M = 7, 11, 6, 3
LENGTHS = np.array([11, 0, 1, 4, 5, 9, 11])
BATCH, PIECE = 3, 4


@pytest.fixture(scope="module")
def X():
    x = (np.random.default_rng(5).random((S, T, P, M)) < 0.25).astype(np.uint8)
    x[:, :, 0] = x[:, :, -2:] = 0                                 # room either way, so that shifts survive the clip
    return x


@pytest.fixture(scope="module")
def ds(X):
    return DeviceDataset(X, LENGTHS, device="cpu")


class Stub:
    """Records what a step is fed."""

    def __init__(self):
        self.fed = []

    def train_step(self, xb, lb, optimizer, lr):
        self.fed.append((xb.clone(), None if lb is None else lb.clone()))
        return torch.tensor(0.5 + len(self.fed), dtype=torch.float32)

    def build_pianoroll(self, xb, lb, is_train, mode):
        self.fed.append((xb.clone(), None if lb is None else lb.clone()))
        self.metrics = {"batch/loss": torch.tensor(float(xb.sum()), dtype=torch.float32)}


class StubEncoder:
    num_layers = 1

    def __init__(self):
        self.fed = []

    def build(self, x, is_train, mode):
        self.fed.append((x.clone(), None))

    def train(self, _, lr, layer):
        return None, None, {"batch/loss": torch.tensor(float(self.fed[-1][0].sum()))}, None, None


def same_batches(a, b):
    assert len(a) == len(b) > 0
    for (xa, la), (xb, lb) in zip(a, b):
        assert xa.dtype == xb.dtype == torch.uint8 and xa.shape == xb.shape and torch.equal(xa, xb)
        assert (la is None) == (lb is None)
        if la is not None:
            assert la.dtype == lb.dtype == torch.int32 and torch.equal(la, lb)


def ids_of_epoch():
    return np.random.default_rng(1).permutation(S)


def run_epoch(data, lengths, epoch=3, **kw):
    gen, acc, stats = Stub(), LossAccumulator(), TrainingStats()
    stats.epoch = epoch
    driver.train_epoch(gen, data, lengths, ids_of_epoch(), BATCH, PIECE, None, acc, stats, lr=0.1, device="cpu", **kw)
    return gen, acc


def expected_windows(X, aug, epoch):
    """The augmented epoch from its parts: the plain windows, each transposed by its songs' shifts of the epoch."""
    moving = aug.bind(P, M)
    sh = aug.shifts(pitch_extents(X, LENGTHS, moving), epoch)
    return sh, [transpose_rolls(X[w[0], w[1]:w[1] + w[2]], sh[w[0]], moving) for w in iter_windows(ids_of_epoch(), LENGTHS, T, BATCH, PIECE) if w is not None]


def test_train_epoch_feeds_the_same_transposed_bytes_from_both_inputs(X, ds):
    aug = Transpose(2, fixed_tracks=(0,), seed=9)
    g0, a0 = run_epoch(X, LENGTHS, augment=aug)
    g1, a1 = run_epoch(ds, LENGTHS, augment=aug)
    g2, _ = run_epoch(ds, None, augment=Transpose(2, fixed_tracks=(0,), seed=9), drain_every=2)
    same_batches(g0.fed, g1.fed)
    same_batches(g0.fed, g2.fed)
    assert (a0.finite_sum, a0.finite_n) == (a1.finite_sum, a1.finite_n)
    sh, exp = expected_windows(X, aug, 3)
    assert (sh != 0).sum() >= 3 and len(exp) == len(g0.fed)
    plain, _ = run_epoch(X, LENGTHS)
    changed = 0
    for (xb, _), e, (xp, _) in zip(g0.fed, exp, plain.fed):
        assert tuple(xb.shape[2:]) == (P, M) and np.array_equal(xb.numpy(), e)
        assert np.array_equal(xb.numpy()[..., 0], xp.numpy()[..., 0])                        # the fixed track stays
        assert np.array_equal(xb.numpy().sum(axis=(1, 2)), xp.numpy().sum(axis=(1, 2)))      # no note is lost
        changed += not torch.equal(xb, xp)
    assert changed >= 3
    g3, _ = run_epoch(ds, None, epoch=4, augment=aug)                                       # another epoch, other shifts
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(g1.fed, g3.fed))
    same_batches(g3.fed, run_epoch(X, LENGTHS, epoch=4, augment=aug)[0].fed)


def test_without_augment_both_feed_what_they_feed_today(X, ds, monkeypatch):
    calls = []
    real = DeviceDataset.window
    monkeypatch.setattr(DeviceDataset, "window", lambda self, *a, **k: (calls.append(sorted(k)), real(self, *a, **k))[1])
    monkeypatch.setattr(driver, "_Augment", lambda *a, **k: pytest.fail("no augmentation was asked for"))
    g0, _ = run_epoch(X, LENGTHS)
    g1, _ = run_epoch(ds, LENGTHS, augment=None)
    same_batches(g0.fed, g1.fed)
    ws = [w for w in iter_windows(ids_of_epoch(), LENGTHS, T, BATCH, PIECE) if w is not None]
    assert len(ws) == len(g0.fed) and all(np.array_equal(x.numpy(), X[w[0], w[1]:w[1] + w[2]]) for (x, _), w in zip(g0.fed, ws))
    assert calls == [["ids_dev"]] * len(ws)                       # the dataset is asked exactly as before


def test_the_epoch_uploads_ids_and_shifts_together(X, ds, monkeypatch):
    """One int32 upload per epoch: the windows' ids back to back, the shifts of the same rows behind them."""
    seen, real = [], torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: (seen.append(a), real(a))[1])
    aug = Transpose(2, fixed_tracks=(0,), seed=9)
    run_epoch(ds, None, augment=aug)
    up = [a for a in seen if a.dtype == np.int32 and a.ndim == 2]
    rows = np.concatenate([w[0] for w in iter_windows(ids_of_epoch(), LENGTHS, T, BATCH, PIECE) if w is not None])
    sh, _ = expected_windows(X, aug, 3)
    assert len(up) == 1 and np.array_equal(up[0], np.stack([rows, sh[rows]]))


def test_extents_of_a_numpy_array_are_computed_once(X, monkeypatch):
    from multinn_amd import data
    calls, real = [], data.pitch_extents
    monkeypatch.setattr(data, "pitch_extents", lambda *a: (calls.append(1), real(*a))[1])
    aug = Transpose(2, fixed_tracks=(0,), seed=9)
    g0, _ = run_epoch(X, LENGTHS, epoch=3, augment=aug)
    g1, _ = run_epoch(X, LENGTHS, epoch=4, augment=aug)
    assert len(calls) == 1 and any(not torch.equal(a[0], b[0]) for a, b in zip(g0.fed, g1.fed))
    run_epoch(X.copy(), LENGTHS, augment=aug)                     # another array: computed again
    assert len(calls) == 2


def test_an_augmented_epoch_leaves_the_global_stream_where_a_plain_one_does(X, ds):
    states = []
    for data, kw in ((X, {}), (X, dict(augment=Transpose(2, fixed_tracks=(0,)))), (ds, {}), (ds, dict(augment=Transpose(2, fixed_tracks=(0,))))):
        np.random.seed(3)
        ids = np.arange(S)
        np.random.shuffle(ids)
        stats = TrainingStats()
        stats.epoch = 3
        driver.train_epoch(Stub(), data, LENGTHS, ids, BATCH, PIECE, None, LossAccumulator(), stats, device="cpu", **kw)
        states.append((np.random.get_state()[1].copy(), np.random.get_state()[2], np.random.random()))
    for st in states[1:]:
        assert np.array_equal(st[0], states[0][0]) and st[1:] == states[0][1:]


def test_evaluate_feeds_untransposed_windows_and_takes_no_augment(X, ds):
    g0, g1 = Stub(), Stub()
    driver.evaluate(g0, X, LENGTHS, BATCH, PIECE, device="cpu")
    driver.evaluate(g1, ds, None, BATCH, PIECE)
    same_batches(g0.fed, g1.fed)
    ws = [w for w in iter_windows(np.arange(S), LENGTHS, T, BATCH, PIECE) if w is not None]
    assert all(np.array_equal(x.numpy(), X[w[0], w[1]:w[1] + w[2]]) for (x, _), w in zip(g0.fed, ws))
    with pytest.raises(TypeError):
        driver.evaluate(Stub(), X, LENGTHS, BATCH, PIECE, device="cpu", augment=Transpose(2))


@pytest.mark.parametrize("n_enc", [1, M])
def test_pretrain_encoders_sees_the_same_transposed_windows(X, ds, n_enc):
    cfg = {"batch_size": BATCH, "piece_size": 1, "learning_rate": 0.1, "epochs": 2}
    aug = Transpose(2, fixed_tracks=(M - 1,), seed=9)
    e0, e1, e2 = ([StubEncoder() for _ in range(n_enc)] for _ in range(3))
    h0 = driver.pretrain_encoders(e0, X, LENGTHS, cfg, beat_size=PIECE, device="cpu", augment=aug)
    h1 = driver.pretrain_encoders(e1, ds, LENGTHS, cfg, beat_size=PIECE, augment=aug)
    driver.pretrain_encoders(e2, X, LENGTHS, cfg, beat_size=PIECE, device="cpu")
    assert h0 == h1
    for i, (a, b, c) in enumerate(zip(e0, e1, e2)):
        same_batches(a.fed, b.fed)
        differs = any(not torch.equal(x[0], y[0]) for x, y in zip(a.fed, c.fed))
        assert differs == (n_enc == 1 or i != M - 1)                 # the fixed track's own encoder sees the plain windows
    moving = aug.bind(P, M)
    sh = aug.shifts(pitch_extents(X, LENGTHS, moving), 1)          # the loop's own epoch: the first one is epoch 1
    np.random.seed(1)                                              # encoder 0, layer 0, epoch 1: the first shuffle of the ids
    ids = np.arange(S)
    np.random.shuffle(ids)
    w = next(w for w in iter_windows(ids, LENGTHS, T, BATCH, PIECE) if w is not None)
    first = transpose_rolls(X[w[0], w[1]:w[1] + w[2]], sh[w[0]], moving)
    assert np.array_equal(e0[0].fed[0][0].numpy(), first.reshape(len(w[0]), w[2], -1) if n_enc == 1 else first[..., 0])


def test_the_cpu_dataset_window_takes_shifts(X, ds):
    ids = np.array([6, 0, 5, 6])
    sh = torch.tensor([1, -1, 0, 7], dtype=torch.int32)
    x, ln = ds.window(ids, 2, 5, shifts_dev=sh, moving=0b110)
    assert np.array_equal(x.numpy().reshape(4, 5, P, M), transpose_rolls(X[ids, 2:7], sh.numpy(), (1, 2))) and ln.tolist() == [5, 5, 5, 5]
    xt, _ = ds.window(ids, 2, 5, track=2, shifts_dev=sh, moving=0b110)
    assert np.array_equal(xt.numpy(), transpose_rolls(X[ids, 2:7], sh.numpy(), (1, 2))[..., 2])
    xf, _ = ds.window(ids, 2, 5, track=0, shifts_dev=sh, moving=0b110)
    assert np.array_equal(xf.numpy(), X[ids, 2:7][..., 0])
    for bad in (sh.long(), sh[:3], sh.view(1, 4), sh.numpy()):
        with pytest.raises(ValueError, match="shifts_dev"):
            ds.window(ids, 2, 5, shifts_dev=bad, moving=0b110)
    for moving in (None, 8, -1, True, (1, 2)):
        with pytest.raises(ValueError, match="moving"):
            ds.window(ids, 2, 5, shifts_dev=sh, moving=moving)
    with pytest.raises(ValueError, match="moving"):
        ds.window(ids, 2, 5, moving=0b110)


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
def run_fit(monkeypatch, X, training, **kw):
    calls = []
    monkeypatch.setattr(driver, "train_epoch", lambda *a, **k: calls.append(k))
    monkeypatch.setattr(driver, "evaluate", lambda *a, **k: (calls.append(("evaluate", k)), 1.0)[1])

    class G:
        def save(self, *a, **k):
            pass
    cfg = dict(batch_size=BATCH, piece_size=1, epochs=2, early_stopping=5, learning_rate=0.1, random_seed=41, **training)
    driver.fit(G(), None, X, LENGTHS, X, LENGTHS, cfg, {"save_checkpoint_epochs": 0}, {"model_dir": "unused", "model_last_dir": "unused"},
               save_best_only=True, log=lambda *_: None, **kw)
    return calls


def test_fit_builds_the_augmentation_from_the_config(X, monkeypatch):
    calls = run_fit(monkeypatch, X, {"transpose": {"max_shift": 1, "fixed_tracks": [0]}}, pitch_stride=3)
    train = [c for c in calls if not isinstance(c, tuple)]
    assert len(train) == 2 and train[0]["augment"] is train[1]["augment"]
    aug = train[0]["augment"]
    assert isinstance(aug, Transpose) and (aug.max_shift, aug.fixed_tracks, aug.seed, aug.pitch_stride) == (1, (0,), 41, 3)
    assert all(c == ("evaluate", {}) for c in calls if isinstance(c, tuple))                 # validation gets no augmentation
    assert run_fit(monkeypatch, X, {"transpose": {"max_shift": 1}})[0]["augment"].fixed_tracks == ()
    plain = run_fit(monkeypatch, X, {})
    assert [c for c in plain if not isinstance(c, tuple)] == [{}, {}]                        # an absent key: today's call, word for word
    for bad, match in (({"max_shift": 6}, "max_shift"), ({"fixed_tracks": [0]}, "mapping"), (3, "mapping"), ({"max_shift": 1, "seed": 2}, "mapping"),
                       ({"max_shift": 1, "fixed_tracks": [3]}, "fixed_tracks")):
        with pytest.raises(ValueError, match=match):
            run_fit(monkeypatch, X, {"transpose": bad})


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_before_any_device_work(lib):
    ok = dict(X=1 << 20, S=4, T=10, D=6, ids=1 << 21, B=2, j=2, Tw=4, e0=0, es=1, Dout=6, lengths=1 << 22, out=1 << 23, out_len=1 << 24,
              shifts=1 << 25, M=3, moving=6)

    def gather(**kw):
        a = dict(ok, **kw)
        rc = lib.mnn_window_gather_shift(None, a["X"], a["S"], a["T"], a["D"], a["ids"], a["B"], a["j"], a["Tw"], a["e0"], a["es"], a["Dout"], a["lengths"],
                                         a["out"], a["out_len"], a["shifts"], a["M"], a["moving"])
        return rc, lib.mnn_last_error().decode()
    for kw, word in ((dict(shifts=None), "shifts"), (dict(M=0), "tracks"), (dict(M=-2), "tracks"), (dict(M=33, D=66, Dout=66), "tracks"), (dict(M=4), "tracks"),
                     (dict(S=0), "positive"), (dict(j=7), "window"), (dict(es=2), "features"), (dict(out=None), "NULL"), (dict(lengths=None), "out_len needs lengths")):
        rc, msg = gather(**kw)
        assert rc == -1 and word in msg and "mnn_window_gather_shift" in msg, (kw, msg)

    def extent(**kw):
        a = dict(dict(X=1 << 20, S=4, T=10, D=6, M=3, moving=6, lengths=None, lo=1 << 21, hi=1 << 22), **kw)
        rc = lib.mnn_pitch_extent(None, a["X"], a["S"], a["T"], a["D"], a["M"], a["moving"], a["lengths"], a["lo"], a["hi"])
        return rc, lib.mnn_last_error().decode()
    for kw, word in ((dict(M=0), "tracks"), (dict(M=33, D=66), "tracks"), (dict(M=4), "tracks"), (dict(S=0), "positive"), (dict(T=0), "positive"),
                     (dict(X=None), "NULL"), (dict(lo=None), "NULL"), (dict(hi=None), "NULL")):
        rc, msg = extent(**kw)
        assert rc == -1 and word in msg and "mnn_pitch_extent" in msg, (kw, msg)
