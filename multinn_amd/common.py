"""Host-side mirror of /root/reference/multinn/models/common: Model, RNN, NADE, RBM, DBN.

Same class names, constructor arguments and method names as the reference, with eager ROCm
tensors in place of TF1 symbolic tensors: a method that built graph ops in the reference runs
the corresponding HIP kernels here (through the C ABI in ``multinn_amd.ops``).

Parameters of a trainable module live in ONE flat float32 buffer (``ParamStore``) together with
its gradient and Adam slots; that flat gradient buffer is also the data-parallel all-reduce
buffer.
"""
import abc
import collections
import contextlib
import gc
import math
import os

import torch

from . import ops
from .switches import flag
from ._lib import MnnError, MnnUnsupported

STREAM_DROPOUT, STREAM_NADE, STREAM_RBM_H, STREAM_RBM_V, STREAM_DBN_ENC, STREAM_DBN_DEC = range(6)


def default_device():
    if not torch.cuda.is_available():
        raise MnnError("multinn_amd needs a ROCm device: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


# --------------------------------------------------------------------------------------------
@contextlib.contextmanager
def graph_capture(g, **kw):
    """`with torch.cuda.graph(g, **kw)` with the cyclic garbage collector switched off from before the capture begins until after it ends.  A
    collection that starts DURING a capture runs finalisers of whatever cyclic garbage is left (dead generators with their own graphs, streams,
    pools) in the middle of it -- one full GPU test run of round 6 died that way ("Fatal Python error: Aborted", "Garbage-collecting", inside a
    captured sampling scan).  Reference-counted frees are unaffected, and so is an explicit gc.collect() (torch.cuda.graph's, when it is
    configured to collect as the capture begins)."""
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, **kw):
            yield
    finally:
        if was:
            gc.enable()


def _warm_up(fn, n=1):
    """fn() n times on a side stream, then the current stream waits for it: whatever a capture needs (parameters, workspaces, persistent-kernel
    attributes) exists before it, and none of the warm-up's work is pending on the stream about to be captured."""
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(int(n)):
            fn()
    cur.wait_stream(side)


def capture_train_step(feed, step, warmup, models, stores, split=False, fwd_bwd=None, opt=None, error_mode="global", reduce=None):
    """The captured optimiser step of every graphed_* train entry: `warmup` eager step()s on a side stream, then hipGraph(s) of the step.
    Returns run(*a, **kw) -> loss: feed(*a, **kw) copies new inputs into the static ones, then the replay.  One rank: ONE graph of step()
    (capture_error_mode=error_mode).  split (data parallel): a graph of fwd_bwd() -> loss and one of opt() (clip + Adam, no all-reduce) in its
    pool (run.opt_graph); each replay all-reduces the flat gradients eagerly between them, so nothing of RCCL is captured (thread_local: the
    process group's watchdog thread may touch the runtime while this thread captures).  The 16-bit packed weights of `models` are marked
    stale before the capture (the graph packs them itself, whatever ran before) and after it (the packed copies live in the graph's pool).
    reduce (split only, optional): the eager work of a replay between the two graphs, in place of the all-reduce of every store's gradient
    -- a mode with several stores exchanges them in ONE collective of its gradient arena.
    stores() (asked after the warm-up, which may create some): the ParamStores whose host mirror store.step follows the device counter.
    run holds no model: one cached on its model (driver._captured_step) would make it cyclic garbage (graph_capture)."""
    from .training import allreduce_flat, setup_cabi_comm
    if split:
        setup_cabi_comm()               # MULTINN_COMM=capi: the communicator exists before anything is captured
    _warm_up(step, warmup)
    for m in models:
        m._packed_step = -1
    graph, opt_graph = torch.cuda.CUDAGraph(), None
    with graph_capture(graph, capture_error_mode="thread_local" if split else error_mode):
        loss = fwd_bwd() if split else step()
    if split:
        opt_graph = torch.cuda.CUDAGraph()
        with graph_capture(opt_graph, pool=graph.pool(), capture_error_mode="thread_local"):
            opt()
    for m in models:
        m._packed_step = -1
    mirror = list(stores())
    for st in mirror:
        st.step -= 1                    # the capture executed nothing (host mirror of store.step_dev)

    def run(*a, **kw):
        feed(*a, **kw)
        graph.replay()
        if opt_graph is not None:
            if reduce is not None:
                reduce()
            else:
                for st in mirror:
                    allreduce_flat(st.grad)
            opt_graph.replay()
        for st in mirror:
            st.step += 1
        return loss
    run.graph, run.opt_graph = graph, opt_graph
    return run


class ScanGraphs:
    """hipGraph cache for whole sampling scans (rnn_estimator.py:271-323, multinn_feedback.py:120-218).

    A scan is `num_steps` x {sample, LSTM step, Dense}: a dozen small launches per generated step, ~0.5 ms of host time
    against ~0.1 ms of device time when launched eagerly.  The whole scan -- intro pass, weight packing and every
    step, each with its own RNG counter baked into its node -- is captured once per (shape, num_steps, seed) and
    replayed; inputs are copied into the captured buffer, the result is a copy of the captured output.  A conditioned scan takes its codes
    (given_codes) as a second static input, copied in the same way: the caller's key records only whether there are any.
    MULTINN_GENERATE_GRAPH=0 keeps the eager loop."""

    def __init__(self, max_entries=4):
        self._cache = collections.OrderedDict()
        self._max = max_entries
        self._stats = {}                 # key -> the particle statistics arrays its captured scan writes (dropped with the entry)

    @staticmethod
    def enabled(x):
        return x.is_cuda and flag("MULTINN_GENERATE_GRAPH") and not torch.cuda.is_current_stream_capturing()

    def run(self, key, x, scan, warm, after_capture, extra=None, lengths=None):
        """scan(static_x) -> output tensor (captured); warm(static_x): a short eager run that creates parameters and
        workspaces before the capture; after_capture(): drop host-side caches that now point into the graph's pool.
        extra (optional, e.g. the codes of a conditioned scan): a second input, then scan(static_x, static_extra) and
        warm(static_x, static_extra).  lengths (optional, the prompt lengths of a ragged scan: int32 [B] on the device): a third input,
        handed on as the keyword `lengths` of scan and warm."""
        ent = self._cache.get(key)
        if ent is None:
            static_x = x.clone()
            static_e = None if extra is None else extra.clone()
            static_l = None if lengths is None else lengths.clone()
            args = (static_x,) if extra is None else (static_x, static_e)
            kw = {} if lengths is None else dict(lengths=static_l)
            _warm_up(lambda: warm(*args, **kw))
            g = torch.cuda.CUDAGraph()
            with graph_capture(g, capture_error_mode="thread_local"):
                out = scan(*args, **kw)
            after_capture()
            ent = (g, static_x, out, static_e, static_l)
            self._cache[key] = ent
            while len(self._cache) > self._max:
                self._cache.popitem(last=False)
        else:
            self._cache.move_to_end(key)
        g, static_x, out, static_e, static_l = ent
        static_x.copy_(x)
        if static_e is not None:
            static_e.copy_(extra)
        if static_l is not None:
            static_l.copy_(lengths)
        g.replay()
        return out.clone()

    @staticmethod
    def generate(owner, key, x, num_steps, given, temperature, scan, stale, max_notes=None, redraws=0, particles=0, stats_shape=None, lengths=None):
        """The one capture wrapper of a `generate`: scan(x, num_steps, given, temperature) eagerly where graphs are off, else one replay of
        the scan captured under key + ("given",) + temperature_key (a new given of the same shape replays the same graph; the temperature
        is baked into the captured launches, nothing at 1.0: the scan captured without it) from the cache kept on `owner`.  max_notes (a
        normalised polyphony cap; None: the call, the key and the captured scan without one): a fifth argument of scan, and max_notes_key;
        redraws (normalised, sampling_redraws; 0: nothing changes): a sixth argument of scan, and redraws_key; particles (normalised,
        sampling_particles; 0: nothing changes): the keyword `particles` of scan, and particles_key; with them stats_shape = (num_steps,
        tracks, B): the owner's `_particle_live` becomes the statistics arrays this scan writes -- new ones for an eager call, the graph
        entry's for a captured one (created before the capture, dropped with the entry).  lengths (normalised prompt lengths on the
        device, int32 [B]; None: nothing changes): the keyword `lengths` of scan, the key gains ("lengths",) and nothing else -- they are
        a third static input, so other lengths of the same shape replay the same graph.  stale(): mark
        the owner's packed weight copies stale -- before the capture (the graph packs them itself: a replay always sees the current
        weights) and after it (the packed copies then live in the graph's pool).  The warm-up is the scan's first min(num_steps, 2) steps."""
        cap = () if max_notes is None else ((max_notes,) if not redraws else (max_notes, redraws))
        kw = dict(particles=particles) if particles else {}
        if not ScanGraphs.enabled(x):
            if particles and stats_shape is not None:
                owner._particle_live = new_particle_cells(*stats_shape, x.device)
            if lengths is not None:
                kw["lengths"] = lengths
            return scan(x, num_steps, given, temperature, *cap, **kw)
        if getattr(owner, "_scan_graphs", None) is None:
            owner._scan_graphs = ScanGraphs()
        if given is not None:
            key = key + ("given",)
        key = key + temperature_key(temperature) + max_notes_key(max_notes) + redraws_key(redraws) + particles_key(particles)
        if lengths is not None:
            key = key + ("lengths",)
        if particles and stats_shape is not None:
            graphs = owner._scan_graphs
            graphs._stats = {k: v for k, v in graphs._stats.items() if k in graphs._cache}
            if key not in graphs._stats:
                graphs._cache.pop(key, None)         # (never both: an entry without its arrays is captured again)
                graphs._stats[key] = new_particle_cells(*stats_shape, x.device)
            owner._particle_live = graphs._stats[key]

        def captured(sx, sg=None, **lk):
            stale()
            return scan(sx, num_steps, sg, temperature, *cap, **kw, **lk)

        def warm(sx, sg=None, **lk):
            n = min(int(num_steps), 2)
            return scan(sx, n, None if sg is None else sg[:, :n].contiguous(), temperature, *cap, **kw, **lk)

        if lengths is not None:
            return owner._scan_graphs.run(key, x, captured, warm, stale, extra=given, lengths=lengths)
        return owner._scan_graphs.run(key, x, captured, warm, stale, extra=given)


# --------------------------------------------------------------------------------------------
# The Philox position of a sampling step's draws: (stream, global row, sub-counter, element) with seed and row0 naming the stream and the
# first row, and the sub-counter "the generated step" (times max(k, 1) for a Gibbs chain).  step: the generated step, a host number; base
# (optional): a one-word step cell on the device that the kernels add to it (a session's captured chunk).  Every sample_single takes one
# (`at`) and reads its position from nothing else.
DrawAt = collections.namedtuple("DrawAt", ("seed", "row0", "step", "base"), defaults=(None,))


# --------------------------------------------------------------------------------------------
# Conditional generation. A visible of a sampling scan is given a code: 0 or 1 clamps it to that value (it is not drawn; its value is fed
# forward exactly like a draw), 255 leaves it free (ops.nade_sample / generate_scan: `given`).
GIVEN_FREE = 255


def check_given(given, batch, num_steps, *tail):
    """The one shape check of a scan's codes, on the host: u8 [batch, num_steps, *tail] (tail: a generator's num_output, or the feedback
    scan's P, M), ValueError otherwise."""
    want = [int(batch), int(num_steps)] + [int(n) for n in tail]
    if not torch.is_tensor(given) or given.dtype != torch.uint8 or list(given.shape) != want:
        got = f"{given.dtype} {tuple(given.shape)}" if torch.is_tensor(given) else type(given).__name__
        raise ValueError(f"given must be u8 {want}, got {got}")


def _check_mask(given_shape, given_mask):
    if given_mask.dtype != torch.bool:
        raise ValueError(f"given_mask must be bool, got {given_mask.dtype}")
    try:
        ok = torch.broadcast_shapes(tuple(given_mask.shape), tuple(given_shape)) == tuple(given_shape)
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError(f"given_mask of shape {tuple(given_mask.shape)} does not broadcast to {tuple(given_shape)} ([M], [P, M] or [B, steps, P, M])")


def given_codes(given, given_mask=None, shape=None):
    """(given, given_mask) -> the scan's tri-state codes, u8 [B, num_steps, P, M] on given's device (no value is read back to the host).
    given: u8 [B, num_steps, P, M], any nonzero value is a note on; given_mask: bool broadcastable to it ([M]: whole tracks, [P, M]: pitch
    ranges, the full shape: any cells), None = every cell is given.  shape (optional): the shape the caller expects.  Cells under the mask
    get 0 / 1, the others GIVEN_FREE.  `.reshape(B, steps, P * M)` is both the joint order p M + m and the MultiNADE order i tracks + m."""
    if given.dtype != torch.uint8 or given.dim() != 4:
        raise ValueError(f"given must be u8 [B, num_steps, P, M], got {given.dtype} {tuple(given.shape)}")
    if shape is not None and tuple(given.shape) != tuple(shape):
        raise ValueError(f"given has shape {tuple(given.shape)}, expected {tuple(shape)}")
    on = (given != 0).to(torch.uint8)
    if given_mask is None:
        return on.contiguous()
    _check_mask(given.shape, given_mask)
    free = torch.full((), GIVEN_FREE, dtype=torch.uint8, device=given.device)
    return torch.where(given_mask.to(given.device), on, free).contiguous()


def given_tracks(given_mask, shape):
    """Host summary of a mask over [B, num_steps, P, M]: (whole, some) -- per track, whether every cell / any cell of it is given."""
    M = shape[-1]
    if given_mask is None:
        return [True] * M, [True] * M
    _check_mask(shape, given_mask)
    m = given_mask.detach().to("cpu")
    per = m.reshape(-1, M) if m.dim() > 0 and m.shape[-1] == M else m.reshape(-1, 1).expand(-1, M)     # (broadcast axes repeat what they hold)
    return [bool(v) for v in per.all(0)], [bool(v) for v in per.any(0)]


def given_mask_tracks(given_mask, shape, tracks=1):
    """The mask of a conditional NLL over a batch of `shape` = [B, T, F] or [B, T, P, M], seen by a model of `tracks` tracks over the
    flattened features (feature f is track f % tracks: the joint order p M + m, the MultiNADE / MultiRBM order i tracks + m; one track: the
    whole step).  Host checks only (ValueError for a mask that is not bool or does not broadcast to `shape`) ->
    (mask4, shape4, whole, some): the mask as it broadcasts to shape4 = [B, T, F / tracks, tracks], and given_tracks of it."""
    shape = tuple(int(n) for n in shape)
    if not torch.is_tensor(given_mask):
        raise ValueError("given_mask must be a bool tensor")
    if len(shape) not in (3, 4):
        raise ValueError(f"x must be [B, T, F] or [B, T, P, M], got {shape}")
    _check_mask(shape, given_mask)
    F = shape[2] * (shape[3] if len(shape) == 4 else 1)
    if F % tracks:
        raise ValueError(f"{F} features do not split into {tracks} tracks")
    shape4 = (shape[0], shape[1], F // tracks, tracks)
    mask4 = given_mask if shape == shape4 else given_mask.expand(shape).reshape(shape4)
    whole, some = given_tracks(mask4, shape4)
    return mask4, shape4, whole, some


# --------------------------------------------------------------------------------------------
# Sampling temperature.  A NADE generator draws visible i as u < sigmoid(logit_i / T) (its nll / probabilities stay the model's own); an RBM
# generator runs the Gibbs chain of exp(-E / T), every conditional sigmoid(z / T).  T is one number or one per track.
MAX_TEMPERATURE_TRACKS = 8


def sampling_temperature(temperature, num_tracks=None, allow_none=True, allow_sequence=True, what="temperature"):
    """The one normalisation of a `temperature` argument, on the host, before any device work.  Returns None (threshold decoding, p >= 0.5:
    NADE generators only -- allow_none), a float, or a tuple of num_tracks floats.  Accepted: a positive finite number; a sequence of
    num_tracks of them (at most MAX_TEMPERATURE_TRACKS; not where allow_sequence is False -- the hidden units of a joint RBM belong to no
    track); None.  A sequence of equal values IS the scalar, so 1.0 and (1.0, ..., 1.0) are both the float 1.0: the kernels, bits and
    captured scans of a call without the argument.  Anything else raises ValueError."""
    import math
    import numbers
    if temperature is None:
        if not allow_none:
            raise ValueError(f"{what}=None (threshold decoding) exists for NADE generators only: an RBM has no threshold mode")
        return None

    def one(t):
        if isinstance(t, bool) or not isinstance(t, numbers.Real) or not math.isfinite(t) or not t > 0:
            raise ValueError(f"{what} must be a positive finite number, got {t!r}")
        return float(t)

    if torch.is_tensor(temperature):
        temperature = temperature.detach().to("cpu").tolist()
    if isinstance(temperature, numbers.Real):
        return one(temperature)
    try:
        seq = list(temperature)
    except TypeError:
        raise ValueError(f"{what} must be a positive finite number or a sequence of them, got {temperature!r}") from None
    if not allow_sequence:
        raise ValueError(f"{what} per track does not exist here (a joint RBM's hidden units belong to no track): pass one number")
    if len(seq) > MAX_TEMPERATURE_TRACKS:
        raise ValueError(f"{what}: at most {MAX_TEMPERATURE_TRACKS} tracks, got {len(seq)} values")
    if num_tracks is None or len(seq) != int(num_tracks):
        raise ValueError(f"{what}: a sequence needs one value per track ({num_tracks}), got {len(seq)}")
    seq = tuple(one(t) for t in seq)
    return seq[0] if all(t == seq[0] for t in seq) else seq


def temperature_key(temperature):
    """What a scan-graph key gains from a (normalised) temperature: nothing at 1.0 -- the key, and the captured scan, of a call without one."""
    return () if temperature == 1.0 else (("temperature", temperature),)


# --------------------------------------------------------------------------------------------
# Polyphony cap.  A NADE generator emits at most K ones per track and generated step: the scan counts the ones of a track, given ones as well
# as drawn ones, and a free visible of a track that has reached its cap is a settled 0 (ops.nade_sample: `max_notes`).  K is one number or
# one per track (None: that track has no cap).  An RBM generator has none: a Gibbs chain has no visible order in which to stop.
def sampling_max_notes(max_notes, num_tracks=None, num_dims=None, collapse=True, what="max_notes"):
    """The one normalisation of a `max_notes` argument, on the host, before any device work.  Returns None (no cap), an int >= 0, or a tuple
    of num_tracks entries, each an int >= 0 or None.  Accepted: None; an integer >= 0; a sequence of num_tracks entries (at most
    MAX_TEMPERATURE_TRACKS), each an integer >= 0 or None.  num_dims (the visibles of a track, where known): a cap >= num_dims can never be
    reached and is None.  A sequence of equal entries IS the scalar (collapse=False: where a sequence counts by visible index inside ONE
    NADE and a scalar counts the whole of it, the sequence stays), and all-None is None: the kernels, bits and captured scans of a call
    without the argument.  Anything else -- a bool, a float, a negative number, a wrong length -- raises ValueError."""
    import numbers
    if max_notes is None:
        return None

    def one(k):
        if k is None:
            return None
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 0:
            raise ValueError(f"{what} must be an integer >= 0 (or None: no cap), got {k!r}")
        return None if num_dims is not None and int(k) >= int(num_dims) else int(k)

    if torch.is_tensor(max_notes):
        max_notes = max_notes.detach().to("cpu").tolist()
    if isinstance(max_notes, numbers.Real):
        return one(max_notes)
    try:
        seq = list(max_notes)
    except TypeError:
        raise ValueError(f"{what} must be an integer >= 0, None, or a sequence of them, got {max_notes!r}") from None
    if len(seq) > MAX_TEMPERATURE_TRACKS:
        raise ValueError(f"{what}: at most {MAX_TEMPERATURE_TRACKS} tracks, got {len(seq)} values")
    if num_tracks is None or len(seq) != int(num_tracks):
        raise ValueError(f"{what}: a sequence needs one value per track ({num_tracks}), got {len(seq)}")
    seq = tuple(one(k) for k in seq)
    if all(k is None for k in seq):
        return None
    return seq[0] if collapse and all(k == seq[0] for k in seq) else seq


def max_notes_key(max_notes):
    """What a scan-graph key gains from a (normalised) cap: nothing at None -- the key, and the captured scan, of a call without one."""
    return () if max_notes is None else (("max_notes", max_notes),)


# --------------------------------------------------------------------------------------------
# The cap by rejection.  With `redraws=R` a row whose step would emit a 1 past a cap is thrown away and drawn again, at most R times, before
# the truncating scan of `max_notes` serves it (ops.nade_sample: `redraws`): an accepted row is an exact draw from the step distribution
# restricted to the caps.  R stands beside max_notes wherever that is accepted and means nothing without it.
MAX_REDRAWS = 255


def sampling_redraws(redraws, max_notes, temperature, what="redraws"):
    """The one normalisation of a `redraws` argument, on the host, before any device work: an integer 0..MAX_REDRAWS.  max_notes: the
    NORMALISED cap of the call -- None: nothing can be violated, and the result is 0 (the kernels, bits and captured scans of a call
    without the argument).  A bool, a non-integer, a value out of range, or redraws > 0 under threshold decoding (temperature None: a
    redraw would emit the same vector again) raise ValueError."""
    import numbers
    if isinstance(redraws, bool) or not isinstance(redraws, numbers.Integral) or not 0 <= redraws <= MAX_REDRAWS:
        raise ValueError(f"{what} must be an integer 0..{MAX_REDRAWS}, got {redraws!r}")
    if redraws > 0 and temperature is None:
        raise ValueError(f"{what} > 0 needs a temperature: threshold decoding (temperature=None) would emit the same vector again")
    return 0 if max_notes is None else int(redraws)


def redraws_key(redraws):
    """What a scan-graph key gains from (normalised) redraws: nothing at 0 -- the key, and the captured scan, of a call without them."""
    return (("redraws", redraws),) if redraws else ()


def redraw_cell(owner, device):
    """A generator's static statistics cell, int32[2] on the device: (scans redrawn at least once, fallback scans) of its last generate call or
    session chunk.  Created once per owner and device (before any capture: the warm-up of a captured scan runs first)."""
    cell = getattr(owner, "_redraw_stats", None)
    if cell is None or cell.device != torch.device(device):
        cell = owner._redraw_stats = torch.zeros(2, dtype=torch.int32, device=device)
    return cell


def redraw_counts(owner):
    """(redrawn, fallback) of the owner's last generate call or session chunk, as ints (scans: row x track x step); synchronises.  (0, 0)
    where that call ran without redraws: the cell was not written, and is not read."""
    if not getattr(owner, "_redraw_live", False):
        return 0, 0
    n = owner._redraw_stats.cpu()
    return int(n[0]), int(n[1])


# --------------------------------------------------------------------------------------------
# Ragged prompts.  With `lengths` row b of an intro x [B, Ti, ...] is the prompt x[b, :lengths[b]]: the intro pass stops that row's LSTM state
# at its own length (ops.lstm_step_det: lengths, t) and generated step j of the row is the step at absolute time lengths[b] + j.  Row b of
# the call is then, bit for bit, the one-row call on x[b:b+1, :lengths[b]] with row0 + b (DESIGN.md section 4 "Ragged prompts").
def prompt_lengths(lengths, B, Ti, what="lengths"):
    """The one normalisation of a generation call's prompt lengths, on the host, before any device work: None (the entries, kernels, bits,
    graph key and captured scan of a call without the argument) or a tuple of B ints in 1..Ti that are not all Ti.  Accepted: a sequence of
    ints, an integer NumPy array or an integer CPU tensor of B entries; None and "every entry equals Ti" are None.  ValueError: bools,
    non-integers, a wrong count, a value outside 1..Ti -- and a tensor on a device, which could only be checked by synchronising.
    B = Ti = None (a mode whose x is not built yet): only what needs neither is checked, and the tuple is returned."""
    import numbers
    import numpy as np
    if lengths is None:
        return None
    if B is None or Ti is None:
        B = Ti = None
    else:
        B, Ti = int(B), int(Ti)
    if torch.is_tensor(lengths):
        if lengths.device.type != "cpu":
            raise ValueError(f"{what} must live on the host (a sequence, a NumPy array or a CPU tensor): checking a tensor on {lengths.device} "
                             "would synchronise")
        if lengths.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64) or lengths.dim() != 1:
            raise ValueError(f"{what} must be integers, one per row, got a {lengths.dtype} tensor of shape {tuple(lengths.shape)}")
        vals = lengths.tolist()
    elif isinstance(lengths, np.ndarray):
        if lengths.dtype.kind not in "iu" or lengths.ndim != 1:
            raise ValueError(f"{what} must be integers, one per row, got a {lengths.dtype} array of shape {lengths.shape}")
        vals = lengths.tolist()
    elif isinstance(lengths, (list, tuple)):
        vals = list(lengths)
        if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in vals):
            raise ValueError(f"{what} must be integers, one per row, got {lengths!r}")
        vals = [int(v) for v in vals]
    else:
        raise ValueError(f"{what} must be None, a sequence of ints, an integer NumPy array or an integer CPU tensor, got {type(lengths).__name__}")
    if B is None:
        if any(v < 1 for v in vals):
            raise ValueError(f"{what} must be >= 1, got {vals}")
        return tuple(vals)
    if len(vals) != B:
        raise ValueError(f"{what} must have one entry per row ({B}), got {len(vals)}")
    if any(not 1 <= v <= Ti for v in vals):
        raise ValueError(f"{what} must lie in 1..{Ti} (the intro's steps), got {vals}")
    return None if all(v == Ti for v in vals) else tuple(vals)


def prompt_lengths_device(lengths, device):
    """Normalised prompt lengths (a tuple) as the int32 [B] array the kernels read, on `device`."""
    return torch.tensor(lengths, dtype=torch.int32).to(device)


def last_prompt_rows(x, lengths_dev):
    """x[b, lengths[b] - 1] of every row, gathered on the device: the last row of each prompt (a Gibbs chain's start)."""
    return x[torch.arange(x.shape[0], device=x.device), lengths_dev.long() - 1]


def refuse_prompt_lengths(lengths, who, why):
    """The paths without a ragged form: any lengths (None excepted) raise MnnUnsupported, before any device work."""
    if lengths is not None:
        raise MnnUnsupported(f"{who}: prompt lengths are not supported here ({why})")


# --------------------------------------------------------------------------------------------
# Importance resampling.  With `particles=C` a partly given NADE step runs C clamped scans and emits one of them, picked with probability
# proportional to the probability it gives the step's given cells (ops.nade_sample_sir): an approximate draw from p(free | given, past),
# exact as C grows.  None, 0 and 1 are the call without the argument.
MAX_PARTICLES = 1024


def sampling_particles(particles, temperature=1.0, max_notes=None, given=True, what="particles"):
    """The one normalisation of a `particles` argument, on the host, before any device work: 0 (the kernels, bits and captured scans of a call
    without the argument) or an integer 2..MAX_PARTICLES.  None, 0 and 1 are 0, and so is any value where nothing is given (given False /
    None).  A bool, a non-integer or a value outside 0..MAX_PARTICLES raise ValueError, as do particles > 1 under threshold decoding
    (temperature None draws nothing); particles > 1 with a (normalised) max_notes raise MnnUnsupported: a cap changes the proposal."""
    import numbers
    if particles is None:
        return 0
    if isinstance(particles, bool) or not isinstance(particles, numbers.Integral) or not 0 <= particles <= MAX_PARTICLES:
        raise ValueError(f"{what} must be None or an integer 0..{MAX_PARTICLES}, got {particles!r}")
    if particles <= 1 or given is None or given is False:
        return 0
    if temperature is None:
        raise ValueError(f"{what} > 1 needs a temperature: threshold decoding (temperature=None) draws nothing to resample")
    if max_notes is not None:
        raise MnnUnsupported(f"{what} > 1 with max_notes is not supported: a polyphony cap changes the proposal the weights belong to")
    return int(particles)


def particles_key(particles):
    """What a scan-graph key gains from (normalised) particles: nothing at 0 -- the key, and the captured scan, of a call without them."""
    return (("particles", particles),) if particles else ()


def refuse_particles(particles, who):
    """The paths without a particle form (the feedback modes' grouped multi-job sample launch): particles > 1 raise MnnUnsupported, after the
    argument's own checks."""
    if sampling_particles(particles):
        raise MnnUnsupported(f"{who}: particles > 1 are not supported here (the grouped multi-job sample launch has no particle form)")


def new_particle_cells(num_steps, tracks, B, device):
    """The statistics arrays of a scan of num_steps steps: (ess f32, pick int32), both [num_steps, tracks, B] on the device, WRITTEN by the
    kernels.  Who keeps them: an eager call only its owner's `_particle_live` until the next call; a captured scan its graph entry, whose
    replays write to their addresses (ScanGraphs.generate, session.GeneratorSession) -- they go when the entry leaves its bounded cache."""
    shape = (int(num_steps), int(tracks), int(B))
    return torch.zeros(shape, device=device), torch.zeros(shape, dtype=torch.int32, device=device)


def particle_cells(owner, num_steps, tracks, B, device):
    """What a scan of num_steps steps writes its statistics to: the owner's live arrays where they are this scan's (the caller of the scan
    set them), else arrays of its own that nobody reads (the short warm-up run in front of a capture)."""
    live = getattr(owner, "_particle_live", None)
    if live is not None and tuple(live[0].shape) == (int(num_steps), int(tracks), int(B)) and live[0].device == torch.device(device):
        return live
    return new_particle_cells(num_steps, tracks, B, device)


def particle_stats(owner, which):
    """The ess (which = 0) or the picks (1) of the owner's last generate call or session chunk as [B, num_steps, tracks]; synchronises.  None
    where that call ran without particles: nothing was written, and nothing is read."""
    live = getattr(owner, "_particle_live", None)
    return None if live is None else live[which].permute(2, 0, 1).contiguous().cpu()


# --------------------------------------------------------------------------------------------
class ParamStore:
    """Flat f32 parameter / gradient / Adam-slot buffers with named views."""

    def __init__(self, device=None):
        self.device = device
        self._specs = []          # (name, shape, init_fn)
        self.theta = self.grad = self.m = self.v = None
        self.views, self.gviews = {}, {}
        self.step = 0

    def declare(self, name, shape, init):
        assert self.theta is None, "declare() after materialize()"
        self._specs.append((name, tuple(shape), init))

    def materialize(self):
        if self.theta is not None:
            return
        dev = self.device or default_device()
        n = sum(math.prod(s) for _, s, _ in self._specs)
        self.theta = torch.zeros(n, device=dev)
        self.grad = torch.zeros(n, device=dev)
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        self.step_dev = torch.zeros(1, device=dev, dtype=torch.int32)     # device copy of `step` (read by kernels under hipGraph replay)
        # optimiser steps the device skipped because the gradient norm was not finite (mnn_clip_adam_step; f16 loss-scale overflow)
        self.skipped = torch.zeros(1, device=dev, dtype=torch.int32)
        # the dynamic part of the f16 loss scale, [m, 1 / m] (+ applied steps since its last change): a skipped step halves m, LS_GROW_AFTER
        # applied steps in a row double it back up to 1 (mnn_step_increment); the backward passes of precision "fp16" multiply their gradient
        # seed by m and the finished gradient by 1 / m, both read on the device
        self.ls_dyn = torch.ones(2, device=dev)
        self.ls_good = torch.zeros(1, device=dev, dtype=torch.int32)
        off = 0
        for name, shape, init in self._specs:
            k = math.prod(shape)
            self.views[name] = self.theta[off:off + k].view(shape)
            self.gviews[name] = self.grad[off:off + k].view(shape)
            if init is not None:
                self.views[name].copy_(init(shape).to(dev))
            off += k

    def __getitem__(self, name):
        return self.views[name]

    def offset(self, name):
        """First word of variable `name` in the flat buffers (declaration order)."""
        off = 0
        for n, shape, _ in self._specs:
            if n == name:
                return off
            off += math.prod(shape)
        raise KeyError(name)

    def names(self):
        return [n for n, _, _ in self._specs]

    LS_GROW_AFTER = 200

    def check(self, tolerate_overflow=False):
        """Raise FloatingPointError if an optimiser step has been skipped on the device since the last check (non-finite gradient norm:
        the f16 backward pass overflowed, or a NaN reached the gradient).  Synchronises; clears the counter.
        tolerate_overflow (a training loop in precision "fp16"): skipped steps are what the dynamic loss scale feeds on -- warn, and raise only
        when the scale has been halved down to its floor without finding a finite gradient (that is a NaN, not an overflow)."""
        if self.theta is None:
            return
        n = int(self.skipped.item())
        if n:
            self.skipped.zero_()
            self.step = int(self.step_dev.item())       # the host mirror counts attempts; the device counter only APPLIED steps
            m = float(self.ls_dyn[0]) if getattr(self, "ls_dyn", None) is not None else 1.0
            if tolerate_overflow and m > 2.0 ** -19:
                import warnings
                warnings.warn(f"{n} optimiser step(s) skipped (non-finite gradient norm: f16 overflow); the loss scale multiplier is now {m:g}")
                return
            raise FloatingPointError(f"{n} optimiser step(s) skipped: the gradient norm was not finite (f16 loss-scale overflow or NaN "
                                     f"gradient; dynamic loss-scale multiplier {m:g}); lower LstmStack.loss_scale_rows or use precision='bf16'")

    def state_dict(self):
        return dict(theta=self.theta.cpu(), m=self.m.cpu(), v=self.v.cpu(), step=int(self.step_dev.item()), names=self.names(),
                    shapes=[s for _, s, _ in self._specs], ls_dyn=self.ls_dyn.cpu(), ls_good=int(self.ls_good.item()))

    def load_state_dict(self, sd):
        if list(sd["names"]) != self.names() or [tuple(s) for s in sd["shapes"]] != [s for _, s, _ in self._specs]:
            raise ValueError("checkpoint does not match the model's variables")
        self.theta.copy_(sd["theta"]); self.m.copy_(sd["m"]); self.v.copy_(sd["v"])
        self.step = int(sd["step"])
        self.step_dev.fill_(self.step)
        if "ls_dyn" in sd:                               # (checkpoints of earlier builds: the dynamic loss scale restarts at 1)
            self.ls_dyn.copy_(sd["ls_dyn"])
            self.ls_good.fill_(int(sd.get("ls_good", 0)))


def glorot_uniform(gen, fan_in, fan_out):
    """tf.contrib.layers.xavier_initializer() / glorot_uniform (rbm.py:36, rnn_nade.py:56)."""
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return lambda shape: (torch.rand(shape, generator=gen) * 2 - 1) * lim


def truncated_normal(gen, std):
    """tf.truncated_normal_initializer(stddev) (nade.py:49-50): resample beyond two sigma."""
    def f(shape):
        x = torch.randn(shape, generator=gen)
        bad = x.abs() > 2
        while bool(bad.any()):
            x[bad] = torch.randn(int(bad.sum()), generator=gen)
            bad = x.abs() > 2
        return x * std
    return f


def zeros_init(shape):
    return torch.zeros(shape)


# --------------------------------------------------------------------------------------------
class Model(abc.ABC):
    """models/common/model.py:9-234."""

    # store.step the 16-bit packed copies were made at; -1 = stale.  Every "stale" mark also starts a new pack epoch: the f32 repacks of the
    # deterministic sampling steps (LstmStack.det_job) are redone once per epoch -- i.e. once per scan, inside its captured graph
    @property
    def _packed_step(self):
        return self.__dict__.get("_packed_step_v", -1)

    @_packed_step.setter
    def _packed_step(self, v):
        self.__dict__["_packed_step_v"] = v
        if v == -1:
            self.__dict__["_pack_epoch"] = self.__dict__.get("_pack_epoch", 0) + 1

    def __init__(self, name="model"):
        self._name = name
        self._is_built = False
        self._variables = {}
        self._trainable_variables = []
        self._placeholders = {}
        self._metrics, self._metrics_upd = None, None
        self._summaries = {"weights": None, "metrics": None, "gradients": None}
        self.store = None

    name = property(lambda self: self._name)
    is_built = property(lambda self: self._is_built)
    variables = property(lambda self: self._variables)
    trainable_variables = property(lambda self: self._trainable_variables)
    placeholders = property(lambda self: self._placeholders)
    metrics = property(lambda self: self._metrics)
    metrics_upd = property(lambda self: self._metrics_upd)
    summaries = property(lambda self: self._summaries)

    @property
    def weight_summary(self):
        """model.py:104-107 (TensorBoard histograms) -> per-variable (mean, std) on the host."""
        return {k: (float(v.mean()), float(v.std())) for k, v in self._flat_named().items()}

    def _flat_named(self):
        return dict(self.store.views) if self.store is not None else {}

    def build(self, x=None, y=None, lengths=None, is_train=None, mode="eval"):
        if mode not in ("train", "eval", "generate"):        # model.py:146-149
            raise ValueError("`mode` must be one of: 'train', 'eval', 'generate'.")

    @abc.abstractmethod
    def build_metrics(self, targets, predictions, cond_probs=None, log_probs=None):
        ...

    def save(self, sess=None, ckpt_dir=None, global_step=None, write_meta_graph=False):
        """model.py:180-207.  torch.save of the flat state (optimizer slots included, R12)."""
        os.makedirs(ckpt_dir, exist_ok=True)
        path = os.path.join(ckpt_dir, f"{self.name}.pt")
        torch.save(self.store.state_dict(), path)
        return path

    def load(self, sess=None, ckpt_dir=None):
        """model.py:209-234: returns False when no checkpoint exists."""
        path = os.path.join(ckpt_dir, f"{self.name}.pt")
        if not os.path.exists(path):
            return False
        self.store.load_state_dict(torch.load(path))
        return True


# --------------------------------------------------------------------------------------------
class RNN(Model):
    """models/common/rnn.py: MultiRNNCell of DropoutWrapper(CudnnCompatibleLSTMCell)."""

    def __init__(self, num_units=128, keep_prob=1.0, attn_length=0, learn_zero_state=False, name="rnn"):
        super().__init__(name=name)
        if isinstance(num_units, int):
            num_units = [num_units]
        if attn_length:
            raise NotImplementedError("attn_length (the AttentionCellWrapper of rnn.py:127-129) is not built: no caller of the reference sets it")
        for u in num_units:
            if u % 32:
                raise ValueError("LSTM units must be a multiple of 32 (gate-interleaved MFMA layout)")
        self._num_units = list(num_units)
        self._keep_prob = keep_prob
        self._learn_zero_state = bool(learn_zero_state)
        self._tanh_c0 = {}
        self._is_train = False

    learn_zero_state = property(lambda self: self._learn_zero_state)
    num_units = property(lambda self: self._num_units)
    num_layers = property(lambda self: len(self._num_units))
    keep_prob = property(lambda self: self._keep_prob)

    def declare(self, store, n_in, gen, prefix="rnn"):
        """Kernel [in+u, 4u] glorot-uniform, bias zeros (LSTMBlockCell defaults).  learn_zero_state: per layer a trainable c0 [1, u],
        zeros, behind ALL cell kernels / biases (rnn.py:139-143, 214-217) -- zeros_init draws nothing, so every other weight is the one a
        model without the flag gets from the same seed."""
        self.n_in = n_in
        self.prefix = prefix
        for l, u in enumerate(self._num_units):
            store.declare(f"{prefix}/cell_{l}/kernel", (n_in + u, 4 * u), glorot_uniform(gen, n_in + u, 4 * u))
            store.declare(f"{prefix}/cell_{l}/bias", (4 * u,), zeros_init)
            n_in = u
        if self._learn_zero_state:
            for l, u in enumerate(self._num_units):
                store.declare(f"{prefix}/cell_{l}/c0", (1, u), zeros_init)
        self.store = store

    def layer_inputs(self):
        return [self.n_in] + self._num_units[:-1]

    def build_cell(self, is_train):
        self._is_train = bool(is_train) if is_train is not None else True
        self._is_built = True

    def effective_keep_prob(self):
        return self._keep_prob if self._is_train else 1.0      # rnn.py:117-120

    def build_metrics(self, targets, predictions, cond_probs=None, log_probs=None):
        return [], [], None

    def zero_state(self, batch_size, dtype=torch.float32):
        """rnn.py:155-176: tuple of (c, h) per layer.  learn_zero_state: (c0, tanh(c0)) tiled over the batch, computed on the device from the
        CURRENT value of the variables (no host read: a captured step follows c0 as the optimiser moves it)."""
        dev = self.store.theta.device
        if self._learn_zero_state:
            out = []
            for l, u in enumerate(self._num_units):
                c0 = self.store[f"{self.prefix}/cell_{l}/c0"]
                th = torch.tanh(c0)
                self._tanh_c0[l] = th                   # kept for zero_state_grad of the same step (the tanh' factor)
                out.append((c0.expand(batch_size, u).contiguous(), th.to(dtype).expand(batch_size, u).contiguous()))
            return tuple(out)
        return tuple((torch.zeros((batch_size, u), device=dev), torch.zeros((batch_size, u), device=dev, dtype=dtype))
                     for u in self._num_units)

    def zero_state_grad(self, dstate):
        """Chain rule of zero_state: dstate [(dc0, dh0) f32 [B, u]] per layer (LstmStack.backward(need_dstate=True)) ->
        g(c0_l) += sum_b dc0_l[b] + (1 - tanh(c0_l)^2) * sum_b dh0_l[b], added into the store's gradient view (every row of a window is valid
        at t = 0; loss scale, grad_scale and row weights are already in dstate)."""
        for l, ds in enumerate(dstate):
            if ds is None:                              # (a layer that ran without a state: LstmStack.backward)
                continue
            dc0, dh0 = ds
            g = self.store.gviews[f"{self.prefix}/cell_{l}/c0"].view(-1)
            ops.bias_grad(dc0, g, accumulate=True)
            sh = torch.empty_like(g)
            ops.bias_grad(dh0, sh)
            th = self._tanh_c0.pop(l, None)             # tanh(c0) of this step's zero_state
            th = torch.tanh(self.store[f"{self.prefix}/cell_{l}/c0"]).view(-1) if th is None else th.view(-1)
            g.addcmul_(sh, 1.0 - th * th)

    def __call__(self, inputs, state, *args, **kwargs):
        if not self._is_built:
            raise RuntimeError("RNN cell is not built yet, build it with `cell.build_cell()` before calling")
        raise NotImplementedError("single-step calls go through RnnEstimator.single_step")


# --------------------------------------------------------------------------------------------
class NADE(Model):
    """models/common/nade.py.  w_enc/w_dec are stored [D, Hn] (reference [D,1,Hn] / [D,Hn,1])."""

    def __init__(self, num_dims, num_hidden=128, internal_bias=False, name="nade"):
        super().__init__(name=name)
        if internal_bias:
            raise NotImplementedError("a standalone NADE with internal biases is not built: RnnNade / RnnMultiNADE(internal_bias=True) fold "
                                      "them into the Dense bias (generators.py), which is the only place the reference uses them (rnn_nade.py:245-251)")
        if num_hidden > 256:
            raise ValueError("NADE hidden units > 256 are not supported by the HIP scan kernels")
        self._num_dims, self._num_hidden, self._internal_bias = num_dims, num_hidden, internal_bias
        self._is_built = True

    num_dims = property(lambda self: self._num_dims)
    num_hidden = property(lambda self: self._num_hidden)
    internal_bias = property(lambda self: self._internal_bias)

    def declare(self, store, gen, prefix="nade"):
        std = 1.0 / math.sqrt(self._num_dims)
        store.declare(f"{prefix}/w_enc", (self._num_dims, self._num_hidden), truncated_normal(gen, std))
        store.declare(f"{prefix}/w_dec", (self._num_dims, self._num_hidden), truncated_normal(gen, std))
        self.store, self.prefix = store, prefix

    _w_enc_t = _w_dec_t = None      # set when the weights are views of a generator's stacked store

    @property
    def w_enc(self):
        return self._w_enc_t if self._w_enc_t is not None else self.store[f"{self.prefix}/w_enc"]

    @property
    def w_dec(self):
        return self._w_dec_t if self._w_dec_t is not None else self.store[f"{self.prefix}/w_dec"]

    def build_metrics(self, targets, predictions, cond_probs=None, log_probs=None):
        from .metrics import base_metrics
        return base_metrics(log_probs, targets, predictions, log_probs)

    def log_prob(self, x, b_enc=None, b_dec=None):
        """nade.py:155-229.  x u8/float [N,D]; returns (nll [N], cond_p [N,D])."""
        if b_enc is None or b_dec is None:
            raise ValueError("Bias values should be provided when `internal_bias` is `False`")
        N = x.shape[0]
        if b_enc.shape[0] == 1 != N:
            b_enc = b_enc.expand(N, -1)
        if b_dec.shape[0] == 1 != N:
            b_dec = b_dec.expand(N, -1)
        bias = torch.cat([b_enc, b_dec], 1).contiguous()
        nll = torch.empty(N, device=bias.device)
        cp = torch.empty((N, self._num_dims), device=bias.device)
        ops.nade_logprob_fwd(x.to(torch.uint8).contiguous(), bias, self.w_enc, self.w_dec, 1, self._num_dims, self._num_hidden,
                             None, nll, cp)
        return nll, cp

    def sample(self, b_enc=None, b_dec=None, n=None, temperature=None, seed=0, row0=0, sub=0):
        """nade.py:231-308.  Returns (samples u8 [N,D], nll [N])."""
        if b_enc is None or b_dec is None:
            raise ValueError("Bias values should be provided when `internal_bias` is `False`")
        N = n or b_enc.shape[0]
        bias = torch.cat([b_enc.expand(N, -1), b_dec.expand(N, -1)], 1).contiguous()
        out = torch.empty((N, self._num_dims), device=bias.device, dtype=torch.uint8)
        nll = torch.empty(N, device=bias.device)
        ops.nade_sample(bias, self.w_enc, self.w_dec, 1, self._num_dims, self._num_hidden, temperature, seed, row0, sub, out, nll=nll)
        return out, nll


# --------------------------------------------------------------------------------------------
def ais_ladder(num_betas, device):
    """The default AIS ladder: num_betas uniformly spaced values from 0 to 1 (f32; the end points exact).  Untuned: pass betas= to override."""
    if num_betas < 2:
        raise ValueError("the AIS ladder needs at least two values (0 and 1)")
    return (torch.arange(num_betas, dtype=torch.float64) / (num_betas - 1)).to(torch.float32).to(device)


class RBM(Model):
    """models/common/rbm.py."""

    def __init__(self, num_dims, num_hidden=128, k=10, name="rbm"):
        super().__init__(name=name)
        self._num_dims, self._num_hidden, self._k = num_dims, num_hidden, k
        self._is_built = True
        self.seed = 0

    num_dims = property(lambda self: self._num_dims)
    num_hidden = property(lambda self: self._num_hidden)
    k = property(lambda self: self._k)

    def declare(self, store, gen, prefix="rbm"):
        store.declare(f"{prefix}/W", (self._num_dims, self._num_hidden), glorot_uniform(gen, self._num_dims, self._num_hidden))
        store.declare(f"{prefix}/bv", (1, self._num_dims), zeros_init)      # rbm.py:62: [W, bv, bh]
        store.declare(f"{prefix}/bh", (1, self._num_hidden), zeros_init)
        self.store, self.prefix = store, prefix

    W = property(lambda self: self.store[f"{self.prefix}/W"])
    bh = property(lambda self: self.store[f"{self.prefix}/bh"])
    bv = property(lambda self: self.store[f"{self.prefix}/bv"])

    def build_metrics(self, targets, predictions, cond_probs=None, log_probs=None):
        """rbm.py:96-146 with per-row free energy (R4); mean([N,N]) == mean_n, so the scalars match."""
        from .metrics import base_metrics
        cost, free_energy = self.free_energy_cost(targets, predictions)
        if log_probs is None and cond_probs is not None:
            from .encoders import reconstruction_cost
            log_probs = reconstruction_cost(targets, cond_probs)   # tf.losses.log_loss summed over the visibles
        else:
            raise ValueError("Incorrect arguments. Either `cond_probs`, or `log_probs` should be provided on `rbm.build_metrics()` function call")
        metrics, upd, summ = base_metrics(cost, targets, predictions, log_probs)
        metrics["free_energy"] = free_energy.mean()
        return metrics, upd, summ

    def forward(self, v, bh=None, seed=None, row0=0, sub=0, stream=STREAM_RBM_H):
        """rbm.py:148-167 -> (p_h f32 [N,Hn], h u8 [N,Hn])."""
        bh = bh if bh is not None else self.bh
        N = v.shape[0]
        p = torch.empty((N, self._num_hidden), device=v.device)
        h = torch.empty((N, self._num_hidden), device=v.device, dtype=torch.uint8)
        vv = v if v.dtype in (torch.uint8, torch.float32) else v.float()
        ops.rbm_hidden(vv.contiguous(), self.W, bh, stream, self.seed if seed is None else seed, row0, sub, p, h)
        return p, h

    def reconstruct(self, h, bv=None, seed=None, row0=0, sub=0, stream=STREAM_RBM_V):
        """rbm.py:169-190 -> (p_v f32 [N,D], v u8 [N,D])."""
        bv = bv if bv is not None else self.bv
        N = h.shape[0]
        p = torch.empty((N, self._num_dims), device=h.device)
        v = torch.empty((N, self._num_dims), device=h.device, dtype=torch.uint8)
        hh = h if h.dtype in (torch.uint8, torch.float32) else h.float()
        ops.rbm_visible(hh.contiguous(), self.W, bv, stream, self.seed if seed is None else seed, row0, sub, p, v)
        return p, v

    def sample(self, v, bh=None, bv=None, k=None, seed=None, row0=0, row_ids=None, sub0=0, given=None, temperature=1.0, sub_base=None):
        """rbm.py:192-231; k=None -> self.k (R1).  Returns (p_v, v_sample u8).  given (optional): codes u8 [N, D] (ops.rbm_gibbs) -- the
        clamped chain: v_sample equals the code at every clamped visible, the free ones are sampled conditioned on all of them.
        temperature: the chain of exp(-E / T); p_v is then the tempered probability.  sub_base: ops.rbm_gibbs's (a session's step cell)."""
        temperature = sampling_temperature(temperature, allow_none=False, allow_sequence=False)
        k = self._k if k is None else k
        bh = bh if bh is not None else self.bh
        bv = bv if bv is not None else self.bv
        N, D = v.shape
        p_v = torch.empty((N, D), device=v.device)
        v_s = torch.empty((N, D), device=v.device, dtype=torch.uint8)
        ops.rbm_gibbs(v.to(torch.uint8).contiguous(), self.W, bh, bv, k, self.seed if seed is None else seed, row0, row_ids, sub0, p_v, v_s,
                      given=given, temperature=temperature, sub_base=sub_base)
        return p_v, v_s

    def log_partition(self, bh=None, bv=None, num_chains=64, num_betas=1000, betas=None, seed=None, row0=0, row_ids=None, stats=None, given=None):
        """log Z of each bias row by annealed importance sampling (ops.rbm_ais; DESIGN.md section 4 "AIS estimator") -> log Z^ f32 [N].
        bh / bv: [N or 1, Hn] / [N or 1, D] rows (default: this RBM's own biases).  betas: the ladder (0 = b_0 <= ... <= b_{L-1} = 1);
        default ais_ladder(num_betas), uniform -- nobody has tuned or measured it.  Z^ is unbiased for Z, so log Z^ is biased LOW.
        stats (optional f32 [N, 2]) receives (effective sample size, standard error of log Z^).
        given (optional): codes u8 [N, D] (ops.rbm_ais; 0 / 1 clamp, 255 free) -> log Z^_c of the clamped RBM (DESIGN.md section 4 "Clamped
        AIS"): free_energy(v) + log Z^_c = -log p(v_free | v_clamped) for a v that agrees with the codes."""
        bh = bh if bh is not None else self.bh
        bv = bv if bv is not None else self.bv
        dev = self.W.device
        betas = ais_ladder(num_betas, dev) if betas is None else torch.as_tensor(betas, dtype=torch.float32).to(dev).contiguous()
        return ops.rbm_ais(self.W, bh, bv, betas, num_chains, self.seed if seed is None else seed, row0, row_ids, stats=stats, given=given)

    def log_partition_reverse(self, v, bh=None, bv=None, num_chains=64, num_betas=1000, betas=None, seed=None, row0=0, row_ids=None, stats=None,
                              given=None):
        """log Z of each bias row by REVERSE annealed importance sampling from the row's data vector v [N, D] (ops.rbm_raise; DESIGN.md
        section 4 "Reverse AIS") -> log Z^_rev f32 [N].  Arguments as log_partition, the same ladder.  1 / Z^_rev is unbiased for the annealing
        model's likelihood ratio of v, so log Z^_rev is biased the other way from log_partition's: HIGH in expectation over data drawn from
        the model.  With a long enough ladder the two bracket log Z and their gap says whether it was long enough; for an arbitrary v on a
        short ladder log Z^_rev can fall below the truth -- it is not a bound per row.  given (optional): codes as log_partition takes them --
        the reverse estimate of the clamped log Z^_c, with the same two statements about its bias and no more."""
        bh = bh if bh is not None else self.bh
        bv = bv if bv is not None else self.bv
        dev = self.W.device
        betas = ais_ladder(num_betas, dev) if betas is None else torch.as_tensor(betas, dtype=torch.float32).to(dev).contiguous()
        return ops.rbm_raise_given(self.W, bh, bv, v.to(torch.uint8).contiguous(), given, betas, num_chains, self.seed if seed is None else seed,
                                   row0, row_ids, stats=stats)

    def free_energy(self, v, bh=None, bv=None):
        bh = bh if bh is not None else self.bh
        bv = bv if bv is not None else self.bv
        F = torch.empty(v.shape[0], device=v.device)
        return ops.rbm_free_energy(v.to(torch.uint8).contiguous(), self.W, bh, bv, F)

    def free_energy_cost(self, v, v_sample, bh=None, bv=None):
        """rbm.py:233-263 (per row): returns (cost [N], free_energy [N])."""
        Fv = self.free_energy(v, bh, bv)
        return Fv - self.free_energy(v_sample, bh, bv), Fv

    def visible_bias_init_ops(self, v):
        """rbm.py:286-297: returns the (not yet executed) init ops -- call each to assign bv = log(1e-6 + p/(1-p)), p the mean
        activation of every visible unit over the batch (over ALL ranks' batches under data parallelism)."""
        from .training import dp_active
        import torch.distributed as dist

        def assign_bv():
            N, D = v.shape
            vf = torch.empty((N, D), device=v.device)
            ops.convert2d(v if v.dtype in (torch.uint8, torch.float32) else v.float(), vf)
            stat = torch.zeros(D + 1, device=v.device)         # [column sums | row count]: one buffer, one all-reduce
            ops.bias_grad(vf, stat[:D], accumulate=True)
            n_tot = float(N)
            if dp_active():
                ops.fill(stat[D:], float(N))
                dist.all_reduce(stat)
                n_tot = float(stat[D])
            ops.rbm_visible_bias_init(stat[:D], n_tot, self.bv.view(-1))
        return [assign_bv]

    def _flat_delta(self):
        """[W | bv | bh] are consecutive in the store (declare()): their flat slice and a delta buffer of the same layout."""
        W, bh = self.W, self.bh
        off = W.storage_offset() - self.store.theta.storage_offset()
        n = self._num_dims * self._num_hidden + self._num_dims + self._num_hidden
        assert bh.storage_offset() - W.storage_offset() == self._num_dims * self._num_hidden + self._num_dims
        return self.store.theta[off:off + n]

    def _cd_update(self, v, lr, seed=None, row0=0, sub0=0):
        """rbm.py:299-335: returns (update_ops, [dW, dbv, dbh]) and applies the deltas (assign_add).  Under data parallelism the flat
        delta [dW | dbv | dbh] is summed over the ranks (ONE all-reduce) and N is the global row count, so every rank
        applies the full-batch update."""
        from .training import dp_active
        import torch.distributed as dist
        seed = self.seed if seed is None else seed
        N = v.shape[0]
        D, Hn = self._num_dims, self._num_hidden
        vu = v.to(torch.uint8).contiguous()
        p_v_s, v_s = self.sample(vu, self.bh, self.bv, self._k, seed, row0, None, sub0)
        _, h = self.forward(vu, None, seed, row0, sub0 + self._k)
        p_h_s, _ = self.forward(v_s, None, seed, row0, sub0 + self._k + 1)
        n_tot = N
        if dp_active():
            cnt = torch.full((1,), float(N), device=v.device)
            dist.all_reduce(cnt)
            n_tot = float(cnt)
        lrn = lr / n_tot
        # outer-product sums on MFMA: [D,N] x [N,Hn]
        Np = ops.round_up(N, 4)
        def t_(x, rows):
            return ops.transpose(x, torch.zeros((rows, Np), device=v.device))
        vT, hT = t_(vu, D), t_(h, Hn)
        pvT, phT = t_(p_v_s, D), t_(p_h_s, Hn)
        delta = torch.zeros(D * Hn + D + Hn, device=v.device)
        dW, dbv, dbh = delta[:D * Hn].view(D, Hn), delta[D * Hn:D * Hn + D].view(1, D), delta[D * Hn + D:].view(1, Hn)
        neg = torch.empty((D, Hn), device=v.device)
        ops.gemm_tn(vT, hT, dW)
        ops.gemm_tn(pvT, phT, neg)
        ops.axpby(lrn, dW.view(-1), -lrn, neg.view(-1), dW.view(-1))
        ops.rbm_cd_bias_delta(vu, p_v_s, h, p_h_s, lrn, dbv.view(-1), dbh.view(-1))
        if dp_active():
            dist.all_reduce(delta)
        theta = self._flat_delta()
        ops.axpby(1.0, theta, 1.0, delta, theta)            # assign_add of W, bv, bh (rbm.py:329-333)
        return [], [dW, dbv, dbh]

    def train(self, v, lr, **kw):
        """rbm.py:265-284."""
        init_ops = self.visible_bias_init_ops(v)
        update_ops, gradients = self._cd_update(v, lr, **kw)
        return init_ops, update_ops, gradients


# --------------------------------------------------------------------------------------------
class DBN(Model):
    """models/common/dbn.py: stacked RBMs; forward feeds SAMPLED codes upward (dbn.py:136-157)."""

    def __init__(self, num_dims, num_hidden, k=10, name="dbn", seed=23, device=None):
        super().__init__(name=name)
        if isinstance(num_hidden, int):
            num_hidden = [num_hidden]
        self._num_dims, self._num_hidden = num_dims, list(num_hidden)
        gen = torch.Generator().manual_seed(seed)
        self.store = ParamStore(device)
        self._rbms = []
        n_in = num_dims
        for i, nh in enumerate(self._num_hidden):
            r = RBM(n_in, nh, k=k, name=f"{name}/rbm_{i}")
            r.declare(self.store, gen, prefix=f"{name}/rbm_{i}")
            self._rbms.append(r)
            n_in = nh
        self.store.materialize()
        self._is_built = True

    num_dims = property(lambda self: self._num_dims)
    num_hidden = property(lambda self: self._num_hidden)
    num_layers = property(lambda self: len(self._num_hidden))
    rbms = property(lambda self: self._rbms)
    rbm_layers = property(lambda self: self._rbms)          # the reference's name (dbn.py:60)

    def build_metrics(self, targets, predictions, cond_probs=None, log_probs=None):
        return self._rbms[0].build_metrics(targets, predictions, cond_probs, log_probs)

    def forward(self, x, seed=0, row0=0, sub=0):
        """dbn.py:136-157 -> (p_h of the top layer, sampled h u8)."""
        h, p = x, None
        for i, r in enumerate(self._rbms):
            p, h = r.forward(h, None, seed, row0, (sub << 4) | i, STREAM_DBN_ENC)
        return p, h

    def reconstruct(self, h, seed=0, row0=0, sub=0):
        """dbn.py:159-180 -> (p_v of the bottom layer, sampled v u8)."""
        v, p = h, None
        for i in range(len(self._rbms) - 1, -1, -1):
            p, v = self._rbms[i].reconstruct(v, None, seed, row0, (sub << 4) | i, STREAM_DBN_DEC)
        return p, v
