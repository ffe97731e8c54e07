"""mnn_window_gather_shift and mnn_pitch_extent (window.hip) against their host statement (data.transpose_rolls / pitch_extents), byte for
byte: every vector case of the joint row and one track, interior and partial chunks, shifts up to the whole axis and to the ends of int32,
every kind of track mask, a skewed output, both gather forms -- and an augmented epoch of driver.train_epoch on a DeviceDataset."""
import numpy as np
import pytest
import torch

from multinn_amd.data import Transpose, pitch_extents, transpose_rolls
from test_transpose_cpu import hand_made_songs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
S, T, B, J = 4, 48, 6, 3
IDS = [2, 0, 2, 3, S + 1, 1]                                      # a repeated id and one outside the dataset
LENGTHS = [T, 20, 5, 0]
SHAPES = [(88, 5), (7, 3), (16, 4), (12, 1)]                      # joint-row vectors of 8, 1 and 16 bytes; one track
I32 = 2 ** 31


def shift_sets(P):
    return [0, 1, -1, P - 1, -(P - 1), P], [I32 - 1, -I32, -P - 3, 0, 2, -2]


def masks(M):
    return sorted({tuple(range(M)), (), tuple(sorted({min(1, M - 1), M - 1}))})


_DATA = {}


def dataset(P, M):
    """(X on the device u8 [S, T, P * M], the same on the host [S, T, P, M]): random bytes, made once per shape and left alone."""
    if (P, M) not in _DATA:
        Xh = np.random.default_rng(P * 37 + M).integers(0, 256, (S, T, P, M), dtype=np.uint8)
        _DATA[P, M] = (torch.from_numpy(Xh).to(DEV).view(S, T, P * M), Xh)
    return _DATA[P, M]


def expected(Xh, Tw, shifts, moving, track=None):
    """The plain window by indexing (a zero row for the id outside the dataset), transposed on the host."""
    w = np.zeros((B, Tw) + Xh.shape[2:], np.uint8)
    for b, i in enumerate(IDS):
        if 0 <= i < S:
            w[b] = Xh[i, J:J + Tw]
    out = transpose_rolls(w, np.array(shifts, np.int64), moving)
    return out.reshape(B, Tw, -1) if track is None else out[..., track]


def gather_shift(X, Tw, shifts, M, moving, track=None, skew=0, with_len=True):
    """ops.window_gather_shift into a guarded buffer that starts `skew` bytes off a 16-byte boundary; the guards must stay untouched."""
    from multinn_amd import ops
    Dout = X.shape[2] // (M if track is not None else 1)
    n = B * Tw * Dout
    flat = torch.full((GUARD + skew + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    out = flat[GUARD + skew:GUARD + skew + n].view(B, Tw, Dout)
    assert out.data_ptr() % 16 == skew % 16
    ln_flat = torch.full((B + 2,), -77, dtype=torch.int32, device=DEV)
    ids = torch.tensor(IDS, dtype=torch.int32, device=DEV)
    sh = torch.tensor(shifts, dtype=torch.int64).to(torch.int32).to(DEV)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV) if with_len else None
    ops.window_gather_shift(X, ids, J, Tw, out, sh, M, sum(1 << m for m in moving), lengths=lengths, out_len=ln_flat[1:B + 1] if with_len else None,
                            track=track)
    assert bool((flat[:GUARD + skew] == 0xA5).all()) and bool((flat[GUARD + skew + n:] == 0xA5).all()), "wrote outside the window"
    assert ln_flat[0] == -77 and ln_flat[-1] == -77
    return out, ln_flat[1:B + 1]


def plain(X, Tw, M, track=None):
    from multinn_amd import ops
    ids = torch.tensor(IDS, dtype=torch.int32, device=DEV)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    out = torch.empty((B, Tw, X.shape[2] // (M if track is not None else 1)), dtype=torch.uint8, device=DEV)
    ln = torch.empty(B, dtype=torch.int32, device=DEV)
    ops.window_gather(X, ids, J, Tw, out, lengths=lengths, out_len=ln, track=track, tracks=M)
    return out, ln


@pytest.mark.parametrize("Tw", [5, 41])
@pytest.mark.parametrize("P, M", SHAPES)
def test_joint_window_against_the_host(P, M, Tw):
    X, Xh = dataset(P, M)
    assert (Tw * P * M) % 256 != 0 and (Tw == 5 or Tw * P * M > 256)      # a partial last workgroup always; interior ones too at Tw = 41
    ln_exp = plain(X, Tw, M)[1]
    for shifts in shift_sets(P):
        for moving in masks(M):
            out, ln = gather_shift(X, Tw, shifts, M, moving)
            assert np.array_equal(out.cpu().numpy(), expected(Xh, Tw, shifts, moving)), (shifts, moving)
            assert torch.equal(ln, ln_exp) and ln.tolist() == [min(max(LENGTHS[i] - J, 0), Tw) if i < S else 0 for i in IDS]
    assert not gather_shift(X, Tw, shift_sets(P)[1], M, tuple(range(M)))[0][:3].any()     # |shift| >= P: zeros on every moving track


@pytest.mark.parametrize("P, M", SHAPES)
def test_an_output_one_byte_off_its_allocation(P, M):
    X, Xh = dataset(P, M)
    shifts, moving = shift_sets(P)[0], masks(M)[-1]
    for Tw in (5, 41):
        for skew in (1, 9):
            out, _ = gather_shift(X, Tw, shifts, M, moving, skew=skew)
            assert np.array_equal(out.cpu().numpy(), expected(Xh, Tw, shifts, moving)), (Tw, skew)
    out, _ = gather_shift(X, 5, shifts, M, moving, with_len=False)               # without lengths
    assert np.array_equal(out.cpu().numpy(), expected(Xh, 5, shifts, moving))


@pytest.mark.parametrize("Tw", [5, 41])
@pytest.mark.parametrize("P, M", SHAPES)
def test_single_track_of_a_moving_and_of_a_fixed_track(P, M, Tw):
    X, Xh = dataset(P, M)
    moving = (M - 1,)
    for shifts in shift_sets(P):
        for track in sorted({0, M - 1}):
            out, ln = gather_shift(X, Tw, shifts, M, moving, track=track, skew=1)
            assert np.array_equal(out.cpu().numpy(), expected(Xh, Tw, shifts, moving, track=track)), (shifts, track)
            assert torch.equal(ln, plain(X, Tw, M, track=track)[1])
            if track not in moving:                                              # a track that stays: the plain gather
                assert torch.equal(out, plain(X, Tw, M, track=track)[0])


@pytest.mark.parametrize("P, M", SHAPES)
def test_zero_shifts_and_no_moving_track_are_the_plain_gather(P, M):
    X, _ = dataset(P, M)
    for Tw in (5, 41):
        for track in (None, M - 1):
            ref, ln_ref = plain(X, Tw, M, track=track)
            for shifts, moving in (([0] * B, tuple(range(M))), (shift_sets(P)[0], ()), (shift_sets(P)[1], ())):
                out, ln = gather_shift(X, Tw, shifts, M, moving, track=track)
                assert torch.equal(out, ref) and torch.equal(ln, ln_ref), (Tw, track, shifts, moving)


def test_pitch_extent_against_the_host():
    from multinn_amd import ops
    Xh, lengths, lo_exp, hi_exp = hand_made_songs()
    Sx, Tx, Px, Mx = Xh.shape
    X = torch.from_numpy(Xh).to(DEV).view(Sx, Tx, Px * Mx)
    len_dev = torch.from_numpy(lengths.astype(np.int32)).to(DEV)
    lo, hi = ops.pitch_extent(X, Mx, 0b110, lengths=len_dev)
    assert lo.dtype == hi.dtype == torch.int32 and lo.tolist() == lo_exp and hi.tolist() == hi_exp
    for tracks, lens in (((1, 2), None), ((0,), lengths), ((), lengths), ((0, 1, 2), None)):
        lo, hi = ops.pitch_extent(X, Mx, sum(1 << m for m in tracks), lengths=None if lens is None else len_dev)
        e = pitch_extents(Xh, lens, tracks)
        assert np.array_equal(lo.cpu().numpy(), e[0]) and np.array_equal(hi.cpu().numpy(), e[1]), tracks
    R = np.random.default_rng(12)                                                # more features than one pass of the workgroup's lanes
    Xr = ((R.random((9, 33, 88, 5)) < 0.004) * R.integers(1, 256, (9, 33, 88, 5))).astype(np.uint8)
    Xr[4] = 0
    lens = R.integers(0, 34, 9)
    Xd = torch.from_numpy(Xr).to(DEV).view(9, 33, 440)
    for tracks in ((1, 2, 3, 4), (3,), (0, 4)):
        lo, hi = ops.pitch_extent(Xd, 5, sum(1 << m for m in tracks), lengths=torch.from_numpy(lens.astype(np.int32)).to(DEV))
        e = pitch_extents(Xr, lens, tracks)
        assert np.array_equal(lo.cpu().numpy(), e[0]) and np.array_equal(hi.cpu().numpy(), e[1]), tracks
        assert lo[4] == 88 and hi[4] == -1 and len(set(e[0].tolist())) > 3


def test_dataset_window_with_shifts_on_the_device():
    from multinn_amd import DeviceDataset
    R = np.random.default_rng(3)
    Xh = (R.random((13, 21, 10, 3)) < 0.3).astype(np.uint8)
    lengths = R.integers(0, 22, 13)
    a, b = DeviceDataset(Xh, lengths, device=DEV), DeviceDataset(Xh, lengths, device="cpu")
    for tracks in ((1, 2), (0,), (0, 1, 2)):
        ea, eb = a.extents(tracks), b.extents(tracks)
        assert ea[0].dtype == np.int64 and np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
    assert a.extents((2, 1))[0] is a.extents((1, 2))[0]
    ids = np.array([12, 0, 5, 5, 7])
    sh = torch.tensor([3, -2, 0, 10, -11], dtype=torch.int32)
    for j, Tw in ((0, 21), (4, 9)):
        for track in (None, 0, 2):
            xa, la = a.window(ids, j, Tw, track=track, shifts_dev=sh.to(DEV), moving=0b110)
            xb, lb = b.window(ids, j, Tw, track=track, shifts_dev=sh, moving=0b110)
            assert torch.equal(xa.cpu(), xb) and torch.equal(la.cpu(), lb), (j, Tw, track)
    assert not torch.equal(a.window(ids, 0, 21)[0].cpu(), b.window(ids, 0, 21, shifts_dev=sh, moving=0b110)[0])     # the shifts do something
    for bad in (sh, sh.to(DEV).long(), sh.to(DEV)[:4]):
        with pytest.raises(ValueError, match="shifts_dev"):
            a.window(ids, 0, 21, shifts_dev=bad, moving=0b110)


def test_wrapper_refusals():
    from multinn_amd import ops
    X = torch.zeros((2, 4, 66), dtype=torch.uint8, device=DEV)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    sh = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.empty((2, 3, 66), dtype=torch.uint8, device=DEV)
    ops.window_gather_shift(X, ids, 0, 3, out, sh, 3, 0b101)                     # the arguments the refusals below vary
    for tracks, moving in ((33, 1), (4, 1), (0, 0), (3, 8), (3, -1), (3, True)):
        with pytest.raises(ValueError, match="tracks|moving"):
            ops.window_gather_shift(X, ids, 0, 3, out, sh, tracks, moving)
    for tracks, moving in ((33, 1), (4, 1), (3, 8)):
        with pytest.raises(ValueError, match="tracks|moving"):
            ops.pitch_extent(X, tracks, moving)
    for bad in (sh.long(), sh.float(), torch.zeros(3, dtype=torch.int32, device=DEV), sh.view(2, 1), sh.cpu(), None, [0, 0]):
        with pytest.raises(ValueError, match="shifts"):
            ops.window_gather_shift(X, ids, 0, 3, out, bad, 3, 0b101)
    with pytest.raises(ValueError, match="track"):
        ops.window_gather_shift(X, ids, 0, 3, out, sh, 3, 0b101, track=3)
    with pytest.raises(ValueError, match="out"):
        ops.window_gather_shift(X, ids, 0, 3, out, sh, 3, 0b101, track=1)


def test_augmented_train_epoch_is_fed_identical_bytes():
    """One augmented epoch of driver.train_epoch on a tiny RnnNade, from the DeviceDataset and from the NumPy array: every step is fed the
    same bytes (train_step is wrapped to capture them, and no step is captured into a graph, so every window passes through it)."""
    from multinn_amd import RnnNade, AdamOptimizer, DeviceDataset, driver
    from multinn_amd.driver import train_epoch, LossAccumulator, TrainingStats
    R = np.random.default_rng(5)
    X = (R.random((8, 8, 12, 2)) < .2).astype(np.uint8)
    X[:, :, :2] = X[:, :, -2:] = 0
    aug = Transpose(3, fixed_tracks=(0,), seed=4)

    def epoch(data, lens):
        gen = RnnNade(24, 16, [32], keep_prob=0.9, precision="fp32", seed=2)
        gen._materialize(24)
        fed, step = [], gen.train_step

        def recording(xb, lb, *a, **k):
            fed.append((xb.clone(), None if lb is None else lb.clone()))
            return step(xb, lb, *a, **k)
        gen.train_step = recording
        stats = TrainingStats()
        stats.epoch = 2
        train_epoch(gen, data, lens, np.arange(8), 4, 8, AdamOptimizer(0.01), LossAccumulator(), stats, lr=0.01, device=DEV, augment=aug)
        gen.check()
        return fed

    with pytest.MonkeyPatch.context() as monkey:
        monkey.setattr(driver, "_captured_step", lambda *a, **k: None)          # every step eager
        f0 = epoch(X, np.full(8, 8))
        f1 = epoch(DeviceDataset(X, device=DEV), None)
    assert len(f0) == len(f1) == 2
    sh = aug.shifts(pitch_extents(X, None, (1,)), 2, 12)
    assert (sh != 0).sum() >= 4
    for k, ((xa, la), (xb, lb)) in enumerate(zip(f0, f1)):
        assert tuple(xa.shape) == tuple(xb.shape) == (4, 8, 12, 2) and torch.equal(xa, xb) and la is None and lb is None
        assert np.array_equal(xa.cpu().numpy(), transpose_rolls(X[4 * k:4 * k + 4], sh[4 * k:4 * k + 4], (1,)))
