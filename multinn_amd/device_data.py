"""A dataset that lives on the device: the `[songs, steps, pitches, tracks]` piano-rolls of utils/data.py:38-100 uploaded ONCE, and the windows
of train.py:164-173 cut out of them by one HIP kernel (`ops.window_gather`) instead of a NumPy fancy index + a pageable host-to-device copy
per step.  Opt-in: `driver.train_epoch` / `evaluate` / `pretrain_encoders` / `fit` take a `DeviceDataset` wherever they take the NumPy array,
and feed the step the same bytes in the same order.  A window may be transposed while it is cut (`data.Transpose` through the driver's
`augment=`: per-row pitch shifts of the moving tracks, `ops.window_gather_shift`), with `data.transpose_rolls` as the host statement of it.
"""
import numpy as np
import torch

from . import ops
from .data import moving_bits, pitch_extents, transpose_rolls


class DeviceDataset:
    """X: NumPy uint8 or bool `[S, T, P, M]`; lengths: None (every song has T steps) or S integers in 0..T.

    The upload goes through ONE reused staging buffer of at most `slab_bytes` (pinned for a ROCm device; a single song when a song is larger):
    a slab of songs is copied into it, sent, and waited for before the next one, so the host memory in flight is bounded by that buffer and no
    second full host copy of X is made, whatever X's strides.  `lengths` stays on the host as np.int64 (what `driver.iter_windows` reads) and
    goes to the device as int32.

    Refused with ValueError before anything is uploaded: an X of another rank or dtype; lengths of another count or outside 0..T; a dataset
    larger than `max_fraction` of the device memory that is free right now (`torch.cuda.mem_get_info`).  `max_fraction` is a policy, not a
    measurement: the rest is the model's, its workspaces' and the captured steps'.  A dataset that does not fit is not streamed.

    device "cuda[:n]": windows are cut by the HIP kernel.  device "cpu": the same windows by torch indexing (no kernel, no pinning) -- what
    the driver logic is tested with where there is no GPU, and what the kernel is compared against."""

    def __init__(self, X, lengths=None, device="cuda", max_fraction=0.5, slab_bytes=64 << 20):
        if not isinstance(X, np.ndarray) or X.ndim != 4:
            raise ValueError(f"DeviceDataset: X must be a NumPy array [songs, steps, pitches, tracks], got {type(X).__name__}"
                             + (f" of rank {X.ndim}" if isinstance(X, np.ndarray) else ""))
        if X.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"DeviceDataset: X must be uint8 or bool, got {X.dtype}")
        if 0 in X.shape:
            raise ValueError(f"DeviceDataset: X has an empty axis, shape {X.shape}")
        S, T, P, M = X.shape
        if lengths is None:
            lengths = np.full(S, T, np.int64)
        else:
            lengths = np.asarray(lengths)
            if lengths.shape != (S,) or not np.issubdtype(lengths.dtype, np.integer):
                raise ValueError(f"DeviceDataset: lengths must be {S} integers (one per song), got {lengths.dtype} {lengths.shape}")
            if lengths.min() < 0 or lengths.max() > T:
                raise ValueError(f"DeviceDataset: lengths must lie in 0..{T}, got {int(lengths.min())}..{int(lengths.max())}")
            lengths = lengths.astype(np.int64)
        device = torch.device(device)
        if device.type not in ("cuda", "cpu"):
            raise ValueError(f"DeviceDataset: device must be a ROCm device ('cuda[:n]') or 'cpu', got {device}")
        if not 0.0 < max_fraction <= 1.0:
            raise ValueError(f"DeviceDataset: max_fraction must lie in (0, 1], got {max_fraction}")
        nbytes = S * T * P * M
        if device.type == "cuda":
            free = torch.cuda.mem_get_info(device)[0]
            if nbytes > max_fraction * free:
                raise ValueError(f"DeviceDataset: the dataset is {nbytes} bytes, more than max_fraction = {max_fraction} of the {free} bytes free on "
                                 f"{device}: it is not streamed (train from the NumPy array, or raise max_fraction)")
        self._X = torch.empty((S, T, P * M), dtype=torch.uint8, device=device)
        self.shape, self.device, self.lengths = (S, T, P, M), self._X.device, lengths
        self._upload(X.view(np.uint8) if X.dtype == np.bool_ else X, max(int(slab_bytes), 1))
        self._len_dev = torch.from_numpy(lengths.astype(np.int32)).to(device)
        self._x_buf = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._len_buf = torch.empty(0, dtype=torch.int32, device=self.device)
        self._extents = {}

    def _upload(self, X, slab_bytes):
        S, T, P, M = self.shape
        per_slab = max(1, min(S, slab_bytes // (T * P * M)))
        stage = torch.empty((per_slab, T, P, M), dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        stage_np = stage.numpy()
        for s0 in range(0, S, per_slab):
            k = min(per_slab, S - s0)
            np.copyto(stage_np[:k], X[s0:s0 + k])
            self._X[s0:s0 + k].copy_(stage[:k].view(k, T, P * M), non_blocking=True)
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()        # the one staging buffer is refilled next

    def __len__(self):
        return self.shape[0]

    @property
    def nbytes(self):
        return self._X.numel()

    def upload_ids(self, song_ids):
        """Host song ids, range-checked, as int32 on the dataset's device (`window`'s ids_dev, or a tensor to slice it from)."""
        return torch.from_numpy(self.check_ids(song_ids).astype(np.int32)).to(self.device)

    def check_ids(self, song_ids):
        ids = np.asarray(song_ids)
        if ids.ndim != 1 or ids.size == 0 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"DeviceDataset: song_ids must be a non-empty 1-D integer array, got {ids.dtype} {ids.shape}")
        if ids.min() < 0 or ids.max() >= self.shape[0]:
            raise ValueError(f"DeviceDataset: song_ids must lie in 0..{self.shape[0] - 1}, got {int(ids.min())}..{int(ids.max())}")
        return ids

    def extents(self, moving_tracks):
        """Host (lo, hi) int64 [S]: `data.pitch_extents` of every song over its own length and the given tracks (what `data.Transpose`
        clips its shifts with).  Computed once per set of tracks -- on a ROCm device by `ops.pitch_extent` with one read-back -- and kept."""
        S, T, P, M = self.shape
        bits = moving_bits(moving_tracks, M)
        if bits not in self._extents:
            if self.device.type == "cuda":
                lo, hi = ops.pitch_extent(self._X, M, bits, lengths=self._len_dev)
                both = torch.stack([lo, hi]).cpu().numpy().astype(np.int64)
                self._extents[bits] = (both[0], both[1])
            else:
                self._extents[bits] = pitch_extents(self._X.numpy().reshape(S, T, P, M), self.lengths, moving_tracks)
        return self._extents[bits]

    def window(self, song_ids, j, Tw, track=None, ids_dev=None, shifts_dev=None, moving=None):
        """(x u8 [B, Tw, P*M] -- or [B, Tw, P], track `track` -- , len int32 [B]) = (X[song_ids, j:j+Tw], clamp(lengths[song_ids] - j, 0, Tw)) on the
        device, written into ONE pair of buffers the dataset owns, grows to the largest window asked for and REUSES for every window:
        consume (or clone) a window before asking for the next one (work already queued on the stream has consumed it).  song_ids: host
        integers, range-checked here; ids_dev: the same ids already on the device as int32 [B] (a slice of one upload per epoch), uploaded
        here when None.  shifts_dev (int32 [B] on the device, with moving = the bit mask of the transposed tracks): row b's moving tracks are
        shifted by shifts_dev[b] positions along the pitch axis, zeros moving in (`data.transpose_rolls`); None: the plain window."""
        S, T, P, M = self.shape
        ids = self.check_ids(song_ids)
        B, j, Tw = ids.size, int(j), int(Tw)
        if j < 0 or Tw < 1 or j + Tw > T:
            raise ValueError(f"DeviceDataset: the window j = {j}, Tw = {Tw} leaves the {T} steps of the dataset")
        if track is not None and not 0 <= int(track) < M:
            raise ValueError(f"DeviceDataset: track {track} of {M} tracks")
        track = None if track is None else int(track)
        if ids_dev is None:
            ids_dev = torch.from_numpy(ids.astype(np.int32)).to(self.device)
        elif ids_dev.dtype != torch.int32 or ids_dev.device != self._X.device or tuple(ids_dev.shape) != (B,) or not ids_dev.is_contiguous():
            raise ValueError(f"DeviceDataset: ids_dev must be the {B} song ids as contiguous int32 on {self._X.device}")
        if shifts_dev is None:
            if moving is not None:
                raise ValueError("DeviceDataset: moving comes with shifts_dev")
        else:
            if not isinstance(shifts_dev, torch.Tensor) or shifts_dev.dtype != torch.int32 or shifts_dev.device != self._X.device \
                    or tuple(shifts_dev.shape) != (B,) or not shifts_dev.is_contiguous():
                raise ValueError(f"DeviceDataset: shifts_dev must be the {B} rows' shifts as contiguous int32 on {self._X.device}")
            if M > 32 or isinstance(moving, bool) or not isinstance(moving, int) or not 0 <= moving < (1 << M):
                raise ValueError(f"DeviceDataset: moving must be a bit mask over the {M} tracks (at most 32), got {moving!r}")
        Dout = P * M if track is None else P
        if self._x_buf.numel() < B * Tw * Dout:
            self._x_buf = torch.empty(B * Tw * Dout, dtype=torch.uint8, device=self.device)
        if self._len_buf.numel() < B:
            self._len_buf = torch.empty(B, dtype=torch.int32, device=self.device)
        x, ln = self._x_buf[:B * Tw * Dout].view(B, Tw, Dout), self._len_buf[:B]
        if self.device.type == "cuda" and shifts_dev is not None:
            ops.window_gather_shift(self._X, ids_dev, j, Tw, x, shifts_dev, M, moving, lengths=self._len_dev, out_len=ln, track=track)
        elif self.device.type == "cuda":
            ops.window_gather(self._X, ids_dev, j, Tw, x, lengths=self._len_dev, out_len=ln, track=track, tracks=M)
        else:
            idx = ids_dev.long()
            w = self._X[idx, j:j + Tw]
            if shifts_dev is not None:
                tracks = [m for m in range(M) if moving >> m & 1]
                w = torch.from_numpy(transpose_rolls(w.numpy().reshape(B, Tw, P, M), shifts_dev.numpy(), tracks)).view(B, Tw, P * M)
            x.copy_(w if track is None else w.view(B, Tw, P, M)[..., track])
            ln.copy_((self._len_dev[idx] - j).clamp(0, Tw))
        return x, ln
