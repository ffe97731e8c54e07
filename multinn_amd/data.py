"""utils/data.py:8-202 -- the on-disk formats either side of the hot path: the `.npy` dataset loader with the
`num_pixels` time-step reshape, intro selection for sampling, padding back to 128 MIDI pitches, and MIDI output.

Host-side NumPy only (no device work).  The reference writes MIDI through `pypianoroll` (absent here and not a dependency of this
package); `write_song` emits the same piano-rolls as a Standard MIDI File (format 1) with a small writer of its own: one tempo
track + one track per instrument, `beat_resolution` ticks per quarter note, a note per maximal run of non-zero cells of a pitch,
velocity = the run's first cell (the reference scales the binary roll by 100 and by a per-instrument gain, data.py:153-166).
"""
import os
import struct

import numpy as np


def pad_to_midi(songs, data_config):
    """data.py:8-35: `[batch, time_steps, step_span, tracks]` -> `[batch, steps, 128, tracks]` (zero rows below / above the range)."""
    lo, hi = data_config['pitch_range']['lowest'], data_config['pitch_range']['highest']
    songs = np.reshape(songs, (songs.shape[0], -1, hi - lo, songs.shape[-1]))
    return np.pad(songs, ((0, 0), (0, 0), (lo, 128 - hi), (0, 0)), 'constant', constant_values=0)


def load_data(data_config, step_size=1):
    """data.py:38-100: loads `<filename>.npy` `[songs, pixels, pitches, tracks]`, zero-pads the time axis to a multiple of
    `step_size` and folds `step_size` pixels into one model time step (`[songs, pixels/step, pitches*step, tracks]`); returns the
    (data, lengths) pairs of the train / validation / test split (test = the LAST num_test songs, as written)."""
    path = data_config['filename']
    n_tr, n_va, n_te = (data_config['split'][k] for k in ('num_train', 'num_valid', 'num_test'))
    if data_config['source'] != 'npy':
        raise ValueError('Not supported data format :(')
    songs = np.load(f'{path}.npy')[:n_tr + n_va + n_te]
    if len(songs.shape) != 4:
        raise ValueError("Dataset must have 4 dimensions.")
    if songs.shape[-1] != len(data_config['instruments']):
        raise ValueError(f"Dataset must have {len(data_config['instruments'])} tracks.")
    pad = (-songs.shape[1]) % step_size
    if pad:
        songs = np.pad(songs, ((0, 0), (0, pad), (0, 0), (0, 0)), 'constant', constant_values=0)
    songs = songs.reshape([songs.shape[0], songs.shape[1] // step_size, songs.shape[2] * step_size, songs.shape[3]])
    if data_config.get('sequence_lengths'):
        lengths = np.load(data_config['sequence_lengths'])[:n_tr + n_va + n_te]
    else:
        lengths = np.full(songs.shape[0], songs.shape[1])
    return ((songs[:n_tr], lengths[:n_tr]), (songs[n_tr:n_tr + n_va], lengths[n_tr:n_tr + n_va]), (songs[-n_te:], lengths[-n_te:]))


def prepare_sampling_inputs(X_train, X_valid, sampling_config, beat_size):
    """data.py:103-141: the intro excerpts (first `intro_beats` beats of the configured train / validation songs), the ids of the
    samples to save (`num_save` samples per intro: ids repeat with stride len(intro_songs)) and their labels t<i> / v<i>."""
    intro_steps = int(sampling_config['intro_beats'] * beat_size)
    ids = sampling_config['intro_ids']
    intro_songs = np.concatenate([X_train[ids['train']['start']:ids['train']['end'], :intro_steps, :],
                                  X_valid[ids['valid']['start']:ids['valid']['end'], :intro_steps, :]], axis=0)
    save_train = np.array(sampling_config['save_ids']['train'])
    save_valid = np.array(sampling_config['save_ids']['valid'])
    song_labels = [f't{i}' for i in save_train] + [f'v{i}' for i in save_valid]
    save_ids = np.concatenate([save_train, save_valid + (ids['train']['end'] - ids['train']['start'])], axis=0)
    nxt = save_ids
    for _ in range(1, sampling_config['num_save']):
        nxt = nxt + len(intro_songs)
        save_ids = np.concatenate([save_ids, nxt], axis=0)
    return intro_songs, save_ids, song_labels


# ---- transposition augmentation --------------------------------------------------------------------------------------
# The reference has no augmentation.  This is the host statement of what `mnn_window_gather_shift` / `mnn_pitch_extent` do on the device
# (device_data.DeviceDataset): the NumPy path of the driver runs it, and the kernels are tested against it.
def _moving_mask(moving_tracks, M):
    """bool [M]: True for the tracks that are transposed (`moving_tracks`: distinct integers in 0..M-1)."""
    tracks = [int(m) for m in moving_tracks]
    if len(set(tracks)) != len(tracks) or any(not 0 <= m < M for m in tracks):
        raise ValueError(f"moving_tracks must be distinct integers in 0..{M - 1}, got {list(moving_tracks)}")
    mask = np.zeros(M, bool)
    mask[tracks] = True
    return mask


def moving_bits(moving_tracks, M):
    """The tracks as the bit mask the kernels take (bit m: track m is transposed)."""
    return sum(1 << m for m in np.nonzero(_moving_mask(moving_tracks, M))[0].tolist())


def transpose_rolls(x, shifts, moving_tracks, pitch_stride=1):
    """x u8 [B, Tw, P, M] -> the same shape with row b's moving tracks shifted along the pitch axis by shifts[b] * pitch_stride positions:
    out[b, t, p, m] = x[b, t, p - shifts[b] * pitch_stride, m] where that position lies in 0..P-1, 0 elsewhere (nothing wraps around; a
    shift of P or more either way leaves zeros); the other tracks are x's.  shifts: B integers.  With the default pitch_stride = 1 they
    are positions of the pitch axis -- what `Transpose.shifts` returns and the kernel takes."""
    x = np.asarray(x)
    if x.ndim != 4:
        raise ValueError(f"transpose_rolls: x must be [B, Tw, P, M], got shape {x.shape}")
    B, _, P, M = x.shape
    shifts = np.asarray(shifts)
    if shifts.shape != (B,) or not np.issubdtype(shifts.dtype, np.integer):
        raise ValueError(f"transpose_rolls: shifts must be {B} integers (one per row), got {shifts.dtype} {shifts.shape}")
    mask = _moving_mask(moving_tracks, M)
    out = x.copy()
    if not mask.any():
        return out
    out[..., mask] = 0
    for b in range(B):
        s = int(shifts[b]) * int(pitch_stride)
        if abs(s) >= P:
            continue
        src, dst = (slice(0, P - s), slice(s, P)) if s >= 0 else (slice(-s, P), slice(0, P + s))
        out[b][:, dst, mask] = x[b][:, src, mask]          # out[b] is a view: one boolean index over the tracks, assigned in place
    return out


def pitch_extents(X, lengths, moving_tracks):
    """(lo, hi) int64 [S]: per song of X [S, T, P, M] the smallest and largest pitch position at which a moving track has a non-zero cell
    in a step t < lengths[song] (lengths None: every step); (P, -1) for a song without such a cell."""
    X = np.asarray(X)
    S, T, P, M = X.shape
    mask = _moving_mask(moving_tracks, M)
    lengths = np.full(S, T, np.int64) if lengths is None else np.asarray(lengths)
    lo, hi = np.full(S, P, np.int64), np.full(S, -1, np.int64)
    for s in range(S):
        used = np.nonzero(X[s, :max(int(lengths[s]), 0)][..., mask].any(axis=(0, 2)))[0]
        if used.size:
            lo[s], hi[s] = used[0], used[-1]
    return lo, hi


class Transpose:
    """Random transposition of the pitched tracks of a training window: every song is shifted by its own number of semitones, drawn anew
    each epoch from -max_shift..max_shift and clipped so that none of the song's notes leaves the pitch range.

    max_shift: K >= 1 semitones.  fixed_tracks: the tracks that stay where they are (the drums: track 0 in the LPD-5 order; there is no
    default guess -- with none given every track moves).  pitch_stride: positions of the pitch axis per semitone (`training.num_pixels`
    folds n time pixels into the pitch axis, position p * n + px: one semitone is then n positions).

    The shift is a function of (seed, epoch, song) alone -- not of the shuffle, the batch size, the window or the rank -- from a generator
    of its own: the global np.random stream that `fit` seeds and shuffles with is not touched.  Bound to a dataset's [P, M] at first use."""

    def __init__(self, max_shift, fixed_tracks=(), seed=23, pitch_stride=1):
        for name, v in (("max_shift", max_shift), ("pitch_stride", pitch_stride)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"Transpose: {name} must be a positive integer, got {v!r}")
        fixed = list(fixed_tracks)
        if any(isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 0 for m in fixed) or len(set(fixed)) != len(fixed):
            raise ValueError(f"Transpose: fixed_tracks must be distinct track numbers, got {fixed!r}")
        self.max_shift, self.fixed_tracks, self.seed, self.pitch_stride = int(max_shift), tuple(int(m) for m in fixed), int(seed), int(pitch_stride)
        self.P = None

    def bind(self, P, M):
        """Check this augmentation against rolls of P pitch positions and M tracks (ValueError where it does not fit, before any work is
        done with it), remember P for `shifts`, and return the moving tracks."""
        if M > 32:
            raise ValueError(f"Transpose: at most 32 tracks, got {M}")
        if any(m >= M for m in self.fixed_tracks):
            raise ValueError(f"Transpose: fixed_tracks {self.fixed_tracks} must lie in 0..{M - 1}")
        if P % self.pitch_stride != 0:
            raise ValueError(f"Transpose: pitch_stride = {self.pitch_stride} must divide the {P} positions of the pitch axis")
        if self.max_shift >= P // self.pitch_stride:
            raise ValueError(f"Transpose: max_shift = {self.max_shift} must be below the {P // self.pitch_stride} semitones of the pitch axis")
        self.P = int(P)
        return tuple(m for m in range(M) if m not in self.fixed_tracks)

    def shifts(self, extents, epoch, P=None):
        """int32 [S], in positions of the pitch axis (semitones * pitch_stride): the epoch's draw per song, clipped to what the song's
        extent (lo, hi) -- `pitch_extents` of the moving tracks -- leaves free below and above.  A song without a pitched note keeps its
        draw, which moves nothing.  P: the positions of the pitch axis (default: what `bind` was given)."""
        P = self.P if P is None else int(P)
        if P is None:
            raise ValueError("Transpose.shifts: the pitch axis is unknown (call bind(P, M) first, or pass P)")
        lo, hi = (np.asarray(a, np.int64) for a in extents)
        n = self.pitch_stride
        raw = np.random.Generator(np.random.PCG64([self.seed, int(epoch)])).integers(-self.max_shift, self.max_shift + 1, size=lo.shape[0])
        clipped = np.clip(raw, -(lo // n), (P - 1 - hi) // n)
        return (np.where(hi < 0, raw, clipped) * n).astype(np.int32)


# ---- Standard MIDI File writer ---------------------------------------------------------------------------------------
def _vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def _track_chunk(events):
    """events: (absolute tick, order, bytes); sorted by tick (note-offs before note-ons at the same tick)."""
    data, last = bytearray(), 0
    for tick, _, ev in sorted(events, key=lambda e: (e[0], e[1])):
        data += _vlq(tick - last) + ev
        last = tick
    data += b'\x00\xff\x2f\x00'
    return b'MTrk' + struct.pack('>I', len(data)) + bytes(data)


_GAIN = {'Piano': 0.8, 'Strings': 0.9, 'Bass': 1.2}           # data.py:158-164


def write_song(song, path, data_config):
    """data.py:144-181: `[time_steps, 128, tracks]` piano-roll -> MIDI file at `path`."""
    song = np.asarray(song, np.float64) * 100.
    names = data_config['instruments']
    res = int(data_config['beat_resolution'])
    tempo = int(round(60_000_000 / float(data_config['tempo'])))
    chunks = [_track_chunk([(0, 0, b'\xff\x51\x03' + struct.pack('>I', tempo)[1:])])]
    melodic = 0
    for i, name in enumerate(names):
        roll = np.take(song, i, axis=-1) * _GAIN.get(name.strip(), 1.0)
        drum = bool(data_config['is_drums'][i])
        if drum:
            ch = 9
        else:
            ch = melodic if melodic < 9 else melodic + 1
            melodic += 1
        ev = [(0, 0, b'\xff\x03' + _vlq(len(name.strip())) + name.strip().encode()),
              (0, 1, bytes([0xC0 | ch, int(data_config['programs'][i]) & 0x7F]))]
        on = roll > 0
        edge = np.diff(np.concatenate([np.zeros((1, roll.shape[1]), bool), on, np.zeros((1, roll.shape[1]), bool)]).astype(np.int8), axis=0)
        for pitch in np.nonzero(on.any(axis=0))[0]:
            starts, ends = np.nonzero(edge[:, pitch] > 0)[0], np.nonzero(edge[:, pitch] < 0)[0]
            for s, e in zip(starts, ends):
                vel = int(min(127, max(1, round(float(roll[s, pitch])))))
                ev.append((int(s), 3, bytes([0x90 | ch, int(pitch), vel])))
                ev.append((int(e), 2, bytes([0x80 | ch, int(pitch), 0])))
        chunks.append(_track_chunk(ev))
    with open(path, 'wb') as f:
        f.write(b'MThd' + struct.pack('>IHHH', 6, 1, len(chunks), res) + b''.join(chunks))


def save_music(music, num_intro, data_config, base_path, save_dir='outputs/', song_labels=None):
    """data.py:184-202: `[num_songs * num_intro, steps, 128, tracks]` -> `<base>_<label>_<j>.mid` for sample j of intro i."""
    os.makedirs(save_dir, exist_ok=True)
    for i in range(num_intro):
        for j in range(music.shape[0] // num_intro):
            label = f'song{i}' if song_labels is None else song_labels[i]
            write_song(music[i + j * num_intro], os.path.join(save_dir, f'{base_path}_{label}_{j}.mid'), data_config)
