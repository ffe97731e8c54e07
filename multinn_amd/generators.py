"""Host-side mirror of /root/reference/multinn/models/generators: Generator, RnnEstimator,
RnnNade, RnnMultiNADE, RnnRBM -- same constructor arguments, method names and return arity.

Eager semantics: ``build(x, y, lengths, is_train, mode)`` RUNS the forward pass (the reference
builds graph ops that a later ``sess.run`` executes), ``train(optimizer, lr)`` runs the backward
pass, the data-parallel all-reduce and the clipped optimiser step.  All compute goes through
the C ABI (multinn_amd.ops); internal tensors are time-major ([T,B,...], row n = t*B + b) and
rows past ``lengths`` are masked by a zero row weight instead of being gathered away
(utils/sequences.py:6-37 defines only the ORDER of the API-level flat outputs, reproduced by
``flat_index``).
"""
import abc
import collections
import contextlib
import functools
import math
import numbers

import weakref

import torch

from . import ops
from .switches import flag, value
from .common import Model, RNN, NADE, RBM, ParamStore, ScanGraphs, DrawAt, check_given, given_codes, given_mask_tracks, sampling_temperature, sampling_max_notes, sampling_redraws, sampling_particles, prompt_lengths, prompt_lengths_device, last_prompt_rows, particle_cells, particle_stats, redraw_cell, redraw_counts, glorot_uniform, zeros_init, default_device, capture_train_step
from .training import compute_gradients, world, dp_active, AdamOptimizer
from ._lib import MnnUnsupported
from .lstm_stack import LstmStack, _SINGLE, drive, drive_group, _det_f32, det_steps

_RnnEstimatorStateTuple = collections.namedtuple("RnnEstimatorStateTuple", ("b_enc", "b_dec", "rnn_state"))


class RnnEstimatorStateTuple(_RnnEstimatorStateTuple):
    """rnn_estimator.py:12-36.  `dense` (not in the reference) keeps the [b_enc | b_dec] matrix the biases are
    views of, so the sampling kernel can take it without a copy."""
    dense = None

    @property
    def dtype(self):
        return self.b_enc.dtype


def _compute_dtype(precision):
    if precision in ("bf16", torch.bfloat16):
        return torch.bfloat16
    if precision in ("fp16", "f16", torch.float16):
        return torch.float16
    if precision in ("fp32", "f32", torch.float32):
        return torch.float32
    raise ValueError("precision must be 'fp16', 'bf16' or 'fp32'")


def flat_index(lengths, B, T, device):
    """Time-major row ids (t*B+b) of the valid rows in the reference's flat order: b-major,
    then t (utils/sequences.py:30-31)."""
    t = torch.arange(T, device=device)[None, :].expand(B, T)
    b = torch.arange(B, device=device)[:, None].expand(B, T)
    if lengths is None:
        return (t * B + b).reshape(-1)
    m = t < lengths.to(device)[:, None]
    return (t * B + b)[m]


class NllEstimate:
    """Negative log-likelihood of a built batch, per valid row in API order (b-major, then t; like RnnRBM.cost).
    nll [n] f32; log_z / free_energy [n] (AIS estimators; None where the NLL is exact); mean: mean NLL per valid row; stderr: standard error
    of `mean` (0 when exact; AIS: sqrt(sum of the rows' squared standard errors) / n, the rows' chains being independent); ess: the smallest
    effective sample size over the rows (inf when exact).  An AIS estimate (method="ais") is biased LOW (E[Z^] = Z, so E[log Z^] <= log Z):
    optimistic, and its own ESS / stderr cannot show chains that never reached a mode.  A reverse-AIS estimate (method="raise": the same
    ladder run downwards from the data row, DESIGN.md section 4 "Reverse AIS") is biased the other way -- HIGH in expectation over data
    drawn from the model: conservative.  Reported together (method="both": an NllBracket) the two bracket the NLL when the ladder is long
    enough, and their gap says when it is not; for an arbitrary row on a short ladder the reverse estimate can fall below the truth, so the
    bracket is not a bound per row."""

    def __init__(self, nll, log_z=None, free_energy=None, row_stderr=None, row_ess=None):
        self.nll, self.log_z, self.free_energy = nll, log_z, free_energy
        self.row_stderr, self.row_ess = row_stderr, row_ess
        n = max(int(nll.numel()), 1)
        self.mean = float(nll.double().sum()) / n
        self.stderr = 0.0 if row_stderr is None else float(row_stderr.double().pow(2).sum().sqrt()) / n
        self.ess = math.inf if row_ess is None or row_ess.numel() == 0 else float(row_ess.min())

    @staticmethod
    def total(parts):
        """The joint NLL of several models of the same rows (a mode's generators): row NLLs, log Z^ and free energies add, squared standard
        errors add, the smallest ESS is kept."""
        if len(parts) == 1:
            return parts[0]
        nll = sum(p.nll for p in parts)
        ai = [p for p in parts if p.log_z is not None]
        log_z = sum(p.log_z for p in ai) if ai else None
        fe = sum(p.free_energy for p in ai) if ai else None
        se = torch.stack([p.row_stderr for p in ai]).pow(2).sum(0).sqrt() if ai else None
        ess = torch.stack([p.row_ess for p in ai]).min(0).values if ai else None
        return NllEstimate(nll, log_z, fe, se, ess)


class NllBracket:
    """estimate_nll(method="both"): lower = the AIS estimate (optimistic), upper = the reverse-AIS estimate (conservative), each the
    NllEstimate its single-method call returns for the same seed.  gap = upper.mean - lower.mean: what the ladder's length leaves open (near 0,
    within gap_stderr, when it is long enough; see NllEstimate for what the bracket does not promise).  gap_stderr: the two standard errors
    in quadrature (the two sets of chains share no uniform).  Exact generators (NADE): lower is upper, gap 0.0."""

    def __init__(self, lower, upper):
        self.lower, self.upper = lower, upper
        self.gap = upper.mean - lower.mean
        self.gap_stderr = math.sqrt(lower.stderr ** 2 + upper.stderr ** 2)

    @staticmethod
    def total(parts):
        """The joint bracket of several models of the same rows: NllEstimate.total on each side (one estimate where every part is exact)."""
        lower = NllEstimate.total([p.lower for p in parts])
        return NllBracket(lower, lower if all(p.lower is p.upper for p in parts) else NllEstimate.total([p.upper for p in parts]))


NLL_METHODS = {"ais": ("ais",), "raise": ("raise",), "both": ("ais", "raise")}       # method -> the estimators it runs, lower side first


def nll_sides(method):
    """The estimators of an estimate_nll method; ValueError for anything else (raised before any device work)."""
    if method not in NLL_METHODS:
        raise ValueError(f"method must be 'ais', 'raise' or 'both', got {method!r}")
    return NLL_METHODS[method]


def nll_result(method, sides):
    """What estimate_nll returns for the per-side estimates: the estimate itself, or the bracket of the two."""
    return NllBracket(*sides) if method == "both" else sides[0]


def total_nll(method, parts):
    """The joint result of several models of the same rows (a mode's generators), each part a result of `method`."""
    return NllBracket.total(parts) if method == "both" else NllEstimate.total(parts)


def rbm_nll_side(side, rbm, v, F, bh, bv, num_chains, num_betas, betas, seed, ids, given=None):
    """One RBM's NLL rows F + log Z^ with log Z^ from AIS (side "ais": RBM.log_partition) or reverse AIS from the rows' targets v (side
    "raise": RBM.log_partition_reverse), chains keyed by the row ids.  given (optional): the rows' codes u8 [n, D] (targets at the given
    cells, 255 at the free ones) -> the CONDITIONAL NLL rows -log p(v_free | v_given) = F(v) + log Z^_c (the clamped estimators)."""
    stats = torch.empty((bh.shape[0], 2), device=bh.device)
    kw = {} if given is None else dict(given=given)
    if side == "ais":
        log_z = rbm.log_partition(bh, bv, num_chains, num_betas, betas, seed, row_ids=ids, stats=stats, **kw)
    else:
        log_z = rbm.log_partition_reverse(v, bh, bv, num_chains, num_betas, betas, seed, row_ids=ids, stats=stats, **kw)
    return NllEstimate(F + log_z, log_z, F, stats[:, 1], stats[:, 0])


def given_nll_result(method, n, device):
    """estimate_nll of n rows whose every cell is given: -log p(nothing | everything) = 0, exactly -- one exact estimate (no log Z^, stderr
    0) on both sides, as an exact generator's."""
    est = NllEstimate(torch.zeros(n, device=device))
    return nll_result(method, (est, est))


NADE_MASK_REFUSAL = ("the conditional NLL of a NADE under a mask that leaves it partly given is not implemented: a NADE factorises over its "
                     "visibles in their order (the joint NADE's are ordered p M + m, all tracks of a pitch side by side), so "
                     "-log p(free | given) is not a sum of its conditionals -- it needs the sum over the free visibles ordered before a "
                     "given one.  A mask under which every NADE is wholly given or wholly free is exact")


NLL_PARTIAL = ("refuse", "importance")


def nll_partial(partial, num_chains=None):
    """estimate_nll's `partial`: what a NADE does under a mask that leaves it partly given -- "refuse" (MnnUnsupported, NADE_MASK_REFUSAL) or
    "importance" (the importance estimator of DESIGN.md section 4, num_chains particles per row).  ValueError for anything else, and for
    fewer than one particle where they would be drawn (num_chains given); raised before any device work."""
    if partial not in NLL_PARTIAL:
        raise ValueError(f"partial must be 'refuse' or 'importance', got {partial!r}")
    if partial == "importance" and num_chains is not None and (isinstance(num_chains, bool) or not isinstance(num_chains, int) or num_chains < 1):
        raise ValueError(f"partial='importance' draws num_chains particles per row: an integer >= 1, got {num_chains!r}")
    return partial


def nade_is_side(side, bias, w_enc, w_dec, tracks, D, Hn, codes, tgt, rows, part, num_chains, seed, ids):
    """The importance estimates of one side for the partly given tracks `part` of a (Multi)NADE: one launch over all tracks (codes u8 [tracks,
    n, D], all 255 on the tracks that are not in `part`: nothing is scanned there), particles keyed by the row ids like an RBM's chains.
    side "ais": the lower side; "raise": the upper side, particle 0's free cells the targets tgt.  rows[m]: the exact NLL(x) rows of track m.
    -> {m: NllEstimate(rows[m] + log p^(x_G), log_z = log p^(x_G), free_energy = rows[m], row standard errors, row ESS)}."""
    stats = torch.empty((tracks, bias.shape[0], 2), device=bias.device)
    log_pg = ops.nade_given_is(bias, w_enc, w_dec, tracks, D, Hn, codes, num_chains, seed, row_ids=ids, data=tgt if side == "raise" else None, stats=stats)
    return {m: NllEstimate(rows[m] + log_pg[m], log_pg[m], rows[m], stats[m, :, 1], stats[m, :, 0]) for m in part}


def refuse_host_model(device, what):
    """MnnUnsupported (an MnnError and a NotImplementedError) for a model that does not live on a ROCm device: raised before any device work."""
    if device is not None and torch.device(device).type != "cuda":
        raise MnnUnsupported(f"{what} runs in HIP kernels: this model lives on {device}, not a ROCm device")


def shifted_sequences(x):
    """x [B, T, F] (or [B, T, P, M]: feature p * M + m) -> (inputs, targets): one all-zero step in front, inputs = x[:, :-1] (multinn_joint.py:83-89)."""
    if x.dim() == 4:
        x = x.reshape(x.shape[0], x.shape[1], -1)
    if x.dim() != 3:
        raise ValueError(f"x must be [B, T, F] or [B, T, P, M], got {tuple(x.shape)}")
    x = x if x.dtype == torch.uint8 else (x != 0).to(torch.uint8)
    inputs = torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1)
    return inputs.contiguous(), x.contiguous()


# ------------------------------------------------------------------------------------------------
class Generator(Model):
    """models/generators/generator.py:9-205."""

    def __init__(self, num_dims, num_hidden, num_hidden_rnn, keep_prob=1.0, internal_bias=False, name="generator", track_name="all"):
        super().__init__(name=name)
        self._track_name = track_name
        self._num_dims = num_dims
        self._num_hidden = [num_hidden] if isinstance(num_hidden, int) else list(num_hidden)
        self._num_hidden_rnn = [num_hidden_rnn] if isinstance(num_hidden_rnn, int) else list(num_hidden_rnn)
        self._keep_prob, self._internal_bias = keep_prob, internal_bias
        self._lengths = self._inputs = None

    num_dims = property(lambda self: self._num_dims)
    num_hidden = property(lambda self: self._num_hidden)
    num_hidden_rnn = property(lambda self: self._num_hidden_rnn)
    track_name = property(lambda self: self._track_name)
    keep_prob = property(lambda self: self._keep_prob)
    internal_bias = property(lambda self: self._internal_bias)

    def build(self, x=None, y=None, lengths=None, is_train=None, mode="eval"):
        super().build(mode=mode)
        self._inputs, self._lengths = x, lengths

    @abc.abstractmethod
    def zero_state(self, batch_size):
        ...

    def forward(self):
        return self._outputs

    @abc.abstractmethod
    def generate(self, x, num_steps, given=None, temperature=1.0, max_notes=None, redraws=0, particles=None, lengths=None):
        ...

    def pretrain(self, optimizer, lr, run_optimizer=True):
        return [], [], self.metrics, self.metrics_upd, self.summaries

    def train(self, optimizer, lr, run_optimizer=True):
        """generator.py:176-205: backward of metrics['batch/loss'] + clipped optimiser step."""
        self.backward()                     # leaves self._dx (f32 [T,B,n_in], time-major) when self.need_dx is set by the mode
        summaries = dict(self.summaries)
        if run_optimizer:
            self._grad_sumsq = compute_gradients(optimizer, self.store, self.clip_norm, lr)
            self._packed_step = -1          # weights changed: re-pack before the next forward
        return [], [], self.metrics, self.metrics_upd, summaries


class RnnEstimator(Generator):
    """models/generators/rnn_estimator.py:39-323."""

    def __init__(self, num_dims, num_hidden, num_hidden_rnn, keep_prob=1.0, internal_bias=True, name="rnn-rbm", track_name="all",
                 num_inputs=None, precision="bf16", seed=23, device=None, clip_norm=5.0, learn_zero_state=False):
        super().__init__(num_dims, num_hidden, num_hidden_rnn, keep_prob, internal_bias, name, track_name)
        self.learn_zero_state = bool(learn_zero_state)  # rnn.py:139-143: every window / intro pass starts from a trained (c0, tanh c0) instead of zeros
        self.dtype = _compute_dtype(precision)
        self.seed, self.clip_norm = seed, clip_norm
        self.row0 = 0                     # global index of this rank's first sequence (data parallel)
        # weight of this generator's loss in the optimised objective: a mode that trains M per-track generators on the MEAN track loss
        # with one global-norm clip over all of them (multinn_jamming.py:235-241) sets 1/M; the generator's own metrics stay unscaled
        self.grad_scale = 1.0
        self.need_dx = False              # a feedback mode sets it: backward() then also leaves d loss / d inputs in self._dx (f32 [T,B,n_in])
        self._dx = None
        self.store = ParamStore(device)
        self._gen = torch.Generator().manual_seed(seed)
        self._num_inputs = num_inputs
        self._packed_step = -1
        self._init_rnn()
        self._init_estimator()

    # -- construction ---------------------------------------------------------------------------
    def _init_rnn(self):
        self._rnn = RNN(num_units=self.num_hidden_rnn, keep_prob=self.keep_prob, learn_zero_state=self.learn_zero_state)

    @abc.abstractmethod
    def _init_estimator(self):
        ...

    def _materialize(self, num_inputs):
        if self.store.theta is not None:
            return
        self._num_inputs = self._num_inputs or num_inputs
        self._declare(self._num_inputs)
        self.store.materialize()
        self._stack = LstmStack(self._rnn, self.store, self.dtype)
        self._stack.owner = weakref.ref(self)            # (weak: a cycle would leave dead generators -- and their captured graphs -- to the garbage
                                                         #  collector, which may then run in the middle of another capture and abort the process)
        self._trainable_variables = [self.store[n] for n in self.store.names()]
        self._variables = dict(self.store.views)

    def _get_rnn_zero_state(self, batch_size):
        return self._rnn.zero_state(batch_size, self.dtype)

    def _state0(self, B, dtype=None):
        """Initial LSTM state of a window / an intro pass: None (the kernels' zero state) or, with learn_zero_state, [(c0, tanh c0)] tiled over
        the B rows -- formed on the device at every call, so a captured step follows c0 as the optimiser moves it."""
        if not self.learn_zero_state:
            return None
        return list(self._rnn.zero_state(B, self.dtype if dtype is None else dtype))

    def _lstm_backward_co(self, dy, cx):
        """The stack's backward of a built window (cx: the build's context) -- and, with learn_zero_state, the chain rule of zero_state into
        the c0 gradients, in front of _unscale like every other gradient."""
        T, B = cx["T"], cx["B"]
        need = self.learn_zero_state
        r = yield from self._stack.backward_co(dy.view(T, B, -1), cx["lstm"], cx["kp"], self.seed, self.row0, need_dx=self.need_dx,
                                               step_dev=self.store.step_dev, need_dstate=need)
        if need:
            r, dstate = r
            self._rnn.zero_state_grad(dstate)
        return r

    def _ensure_packed(self):
        if self._packed_step != self.store.step or self._stack.packed is None:
            self._stack.pack()
            self._pack_estimator()
            self._packed_step = self.store.step

    # -- layout helpers -------------------------------------------------------------------------
    def _to_time_major_inputs(self, x):
        """x [B,T,Din] (u8/float) -> [T,B,ld0] compute dtype, zero padded."""
        B, T, Din = x.shape
        out = torch.zeros((T, B, self._stack.ld0), device=x.device, dtype=self.dtype)
        out[:, :, :Din] = x.transpose(0, 1).to(self.dtype)
        return out

    # set by a caller that captures ragged steps (the mode classes' graphed_train_step): row weights, valid-row count and f16 loss scale of a
    # ragged window are then derived on the device, without a host read
    ragged_on_device = False
    _ls_dev = None

    def lengths_fed(self):
        """New lengths were copied into the static lengths of a captured ragged step.  A replay runs none of the build's Python, so the
        API-order row index cached by `_idx()` (derived from the lengths of the replay before) is dropped here: the per-row properties
        (log_probs, cond_probs, free_energy, cost, _outputs, ...) of the next replay index its rows by ITS lengths."""
        self._flat_idx = None

    def _idx(self):
        """Positions of the API-order rows (b-major, then t: sequences.py:30-31) in the arrays the kernels wrote: time-major rows, or -- for a
        compacted ragged window -- compact rows (through the window's inverse permutation)."""
        if self._flat_idx is None:
            fi = flat_index(self._lengths, self._ctx["B"], self._ctx["T"], self._loss.device)
            cp = self._ctx.get("compact")
            self._flat_idx = cp["inv"].long()[fi] if cp is not None else fi
        return self._flat_idx

    def _row_ids(self, B, T, device):
        """Global ids (int64, t * 65536 + row0 + b) of the time-major rows of a [B, T] window: they key the Gibbs / AIS uniforms of a row, so
        the draws do not depend on the data-parallel split."""
        return (torch.arange(T, device=device)[:, None] * 65536 + (self.row0 + torch.arange(B, device=device))[None, :]).reshape(-1)

    def _row_weight(self, lengths, B, T, device):
        """1/N_valid on valid rows (N_valid summed over ALL ranks), 0 on padding.  Leaves the host copy of N_valid in self._n_valid (the
        f16 loss scale is derived from it)."""
        if lengths is None:
            # full-length batches: every rank holds B*T valid rows, the total is known on the host -- no copy, no collective (this
            # path runs inside captured steps)
            n_ranks = torch.distributed.get_world_size() if (dp_active() and torch.distributed.is_initialized()) else 1
            self._n_valid = B * T * n_ranks
            return torch.full((T * B,), 1.0 / float(B * T * n_ranks), device=device)
        mask = (torch.arange(T, device=device)[:, None] < lengths.to(device)[None, :]).float()
        n_tot = mask.sum()
        if dp_active() and not torch.cuda.is_current_stream_capturing():
            torch.distributed.all_reduce(n_tot)
        if self.ragged_on_device:
            # nothing is read on the host (a captured ragged step of a mode class: MultINNCore.graphed_train_step(lengths=...)): the valid-row
            # count stays a device scalar, and so does the f16 loss scale derived from it (LstmStack.loss_scale's rule, on the device)
            n_tot = n_tot.clamp_min(1.0)
            self._n_valid = None
            self._ls_dev = torch.exp2(torch.round(torch.log2(self._stack.loss_scale_rows * n_tot))).reshape(1) if self.dtype == torch.float16 else None
            return (mask / n_tot).reshape(-1).contiguous()
        self._n_valid = max(int(n_tot), 1)              # ragged windows run eagerly: a host read is allowed here
        return (mask / n_tot).reshape(-1).contiguous()

    # The sampling scans -- generate(), and the feedback modes' scans through steps() / single_step() -- run in DETERMINISTIC f32 arithmetic
    # on the master weights whatever the training precision is (csrc/det_step.hip; the reference samples in f32 too): every LSTM step, Dense
    # and conditional is a fixed sequence of IEEE operations that the tests' C checker restates, so a whole scan is checked bit for bit
    # (BASELINE.json: "bit-exact for Bernoulli sampling indices under a fixed RNG").  MULTINN_DET_SAMPLING=0 restores the throughput
    # kernels (hardware exp2 / rcp activations, packed 16-bit weights), whose scans can only be checked to a tolerance.
    det_sampling = flag("MULTINN_DET_SAMPLING")

    def steps(self, inputs, initial_state=None, lengths=None):
        """rnn_estimator.py:237-252: run the RNN over `inputs` [B,T,Din] and return the state after the last step.  lengths (optional;
        common.prompt_lengths): row b's sequence is inputs[b, :lengths[b]] and its state the one behind ITS last step -- bit for bit the
        state of the one-row call on that slice, whatever lies behind it in `inputs`."""
        if inputs.dim() == 2:
            lengths = prompt_lengths(lengths, inputs.shape[0], 1)
        else:
            lengths = prompt_lengths(lengths, inputs.shape[0], inputs.shape[1])
        if lengths is not None:
            self._refuse_prompt_lengths("steps(lengths=)")
            return self._det_steps(inputs, initial_state, prompt_lengths_device(lengths, inputs.device))
        if self.det_sampling:
            return self._det_steps(inputs, initial_state)
        return self._get_state(inputs, initial_state=initial_state, last_outputs=True)

    def _det_steps(self, inputs, initial_state=None, lengths=None):
        """steps in the deterministic arithmetic; lengths: normalised prompt lengths on the device (int32 [B]) or None."""
        self._materialize(inputs.shape[-1])
        if inputs.dim() == 2:
            inputs = inputs[:, None, :]
        x = inputs if inputs.dtype in (torch.uint8, torch.float32) else inputs.float()
        st = self._state0(x.shape[0], torch.float32) if initial_state is None else [(c, h) for c, h in initial_state.rnn_state]
        h = None
        for t in range(x.shape[1]):
            if lengths is None:
                h, st = self._stack.det_step(x[:, t], st)
            else:                           # a row whose prompt has ended keeps its state: h is then its last live step's output
                h, st = self._stack.det_step(x[:, t], st, lengths=lengths, t=t)
        return self._det_state(h, st)

    def _refuse_prompt_lengths(self, what):
        """MnnUnsupported, before any device work, where prompt lengths have no form: a model on the host, and the throughput recurrences
        (MULTINN_DET_SAMPLING=0), which return only the state behind the intro's last step."""
        refuse_host_model(self.store.device, what)
        if not self.det_sampling:
            raise MnnUnsupported(f"{what} needs the deterministic sampling steps: with MULTINN_DET_SAMPLING=0 the intro pass runs the throughput "
                                 "recurrences, which return only the state behind the intro's last step")

    def _temperature(self, temperature):
        """generate's `temperature`, normalised (common.sampling_temperature): NADE estimators take None and one value per track (of a
        MultiNADE, or by visible index for the one NADE of joint mode), RBM estimators a positive number (per track: RnnMultiRBM)."""
        raise NotImplementedError

    def _max_notes(self, max_notes):
        """generate's `max_notes`, normalised on the host (common.sampling_max_notes) before any device work.  Here: the refusal of the
        estimators that have no cap (RBM: a Gibbs chain has no visible order in which to stop); the NADE estimators override it."""
        if max_notes is not None:
            raise MnnUnsupported(f"max_notes exists for NADE generators only: the Gibbs chain of {type(self).__name__} updates all visibles of a "
                                 "step at once and has no visible order in which a track's count could stop it")
        return None

    def _particles(self, particles, temperature, max_notes, given):
        """generate's `particles`, normalised on the host before any device work.  Here: the estimators that ignore it (RBM: the clamped
        Gibbs chain already conditions on every given cell); the NADE estimators override it."""
        return 0

    def _scan_in_one_call(self, x, num_steps, given=None, temperature=1.0, max_notes=None, redraws=0, particles=0, lengths=None):
        return None                         # estimators without a one-call scan (RnnRBM) step through sample_single / single_step

    # -- generation sessions (session.py) --------------------------------------------------------
    subs_per_step = 1                      # Philox sub-counters a generated step owns (RBM estimators: max(k, 1))

    def session(self, x):
        """A generation session on the intro x [B, Ti, Din] (generate's x): session.GeneratorSession -- sess.generate(num_steps, given,
        temperature) continues the piece chunk by chunk, the chunks concatenated being generate(x, n, ...) bit for bit."""
        from .session import GeneratorSession
        return GeneratorSession(self, x)

    def ragged_session(self, x, lengths):
        """session(x) on ragged prompts: generate's `lengths` (GeneratorSession(gen, x, lengths)).  The session opens behind every row's own
        prompt; its chunks need nothing new, and concatenated they are generate(x, n, ..., lengths=lengths) bit for bit."""
        from .session import GeneratorSession
        return GeneratorSession(self, x, lengths)

    def _state_of(self, out, rnn_state):
        """The estimator state of a Dense output block [B, ldo] and an LSTM state (a session rebuilds it from its static arrays)."""
        raise NotImplementedError

    def _scan_layers(self):
        """What a session's one-call chunks (ops.generate_scan_chunk) need: dict(layers, dense_W, dense_bias, ...), or None for an estimator
        without a one-call scan."""
        return None

    @contextlib.contextmanager
    def _sampling_scope(self):
        """Around the steps of one scan (RnnMultiRBM: its internal bias vectors are formed once per scan)."""
        yield

    def _det_single_step(self, inputs, initial_state, x2=None):
        """single_step in the deterministic arithmetic: inputs u8 | f32 [B, n_x]; x2 (optional, f32 [B, F]) is concatenated behind it -- the
        feedback vector of multinn_feedback.py:85-91, read in place instead of through a torch.cat."""
        h, new = self._stack.det_step(inputs, [(c, hh) for c, hh in initial_state.rnn_state], x2=x2)
        return self._det_state(h, new)

    def check(self, tolerate_overflow=False):
        """Raise if a persistent recurrence launch of this generator ever gave up on a bounded spin (LstmStack.check)."""
        if getattr(self, "_stack", None) is not None:
            self._stack.check()
        # an optimiser step the device skipped (non-finite gradient norm) raises here -- unless the caller is a training loop in precision "fp16",
        # whose dynamic loss scale has already answered the overflow (ParamStore.check)
        self.store.check(tolerate_overflow and self.dtype == torch.float16)

    def _unscale(self, ls):
        """End of a loss-scaled backward pass (LstmStack.loss_scale): gradients and d loss / d inputs back to their true scale."""
        if torch.is_tensor(ls):                         # compacted ragged window: ls is the device word 1 / scale (ops.ragged_index)
            self.store.grad.mul_(ls)
            if self._dx is not None:
                self._dx.mul_(ls)
        elif ls != 1.0:
            ops.axpby(1.0 / ls, self.store.grad, 0.0, None, self.store.grad)
            if self._dx is not None:
                flat = self._dx.view(-1)
                ops.axpby(1.0 / ls, flat, 0.0, None, flat)

    def graphed_build_train(self, x, y, optimizer, lr=None, warmup=2):
        """The generic captured optimiser step: build(x, y, None, True, 'train') + train(optimizer, lr) as hipGraph replays, for the
        generators that train on encoder outputs rather than on a raw piano-roll batch (RnnRBM: jamming mode, RnnMultiNADE: composer
        mode; RnnNade.graphed_train_step is the fused piano-roll form).  Eagerly such a step is host-bound (RnnRBM at [256,128,88]:
        kernels 4 ms, wall 14 ms).  Returns run(x=None, y=None) -> loss.  Step-dependent values (dropout seed, Gibbs seed, Adam step)
        are read from store.step_dev on the device; under data parallelism the gradient all-reduce stays an eager call between two
        graphs (common.capture_train_step).  Full-length batches only."""
        sx, sy = x.clone(), y.clone()

        def feed(x=None, y=None):
            if x is not None:
                sx.copy_(x)
            if y is not None:
                sy.copy_(y)
        return self._capture_step(feed, lambda: self.build(sx, sy, None, True, "train"), optimizer, lr, warmup, error_mode="thread_local")

    def _capture_step(self, feed, forward, optimizer, lr, warmup, **kw):
        """common.capture_train_step of this generator's step: forward() (a train-mode build) + train, or under data parallelism
        forward() + backward | clip + Adam."""
        def step():
            forward()
            self.train(optimizer, lr)
            return self._loss

        def fwd_bwd():
            forward()
            self.backward()
            return self._loss

        def opt():
            self._grad_sumsq = compute_gradients(optimizer, self.store, self.clip_norm, lr, reduce=False)
        return capture_train_step(feed, step, warmup, [self], lambda: [self.store], split=dp_active(), fwd_bwd=fwd_bwd, opt=opt, **kw)

    def estimate_nll(self, x, lengths=None, num_chains=64, num_betas=1000, betas=None, seed=None, method="ais", given_mask=None, partial="refuse"):
        """NLL of every step of x [B, T, F] (or [B, T, P, M]) given the steps before it: builds in eval mode (keep_prob 1) on inputs = x
        shifted by one all-zero step, targets = x, and returns an NllEstimate over the valid rows.  RnnNade: exact (the AIS arguments are
        ignored).  RnnRBM: AIS (see RnnRBM._nll_rows_built).  method: "ais" (biased low), "raise" (reverse AIS from the target rows, the same
        ladder, chains and seed arguments: biased the other way) or "both" -> NllBracket(lower = the "ais" estimate, upper = the "raise" one).
        given_mask (optional, bool, broadcastable to x): the CONDITIONAL NLL of every step -- row t is -log p(x_t,free | x_t,given, x_<t),
        teacher-forced on all of x_<t, the cells under the mask given.  RBM estimators: the clamped estimators (DESIGN.md section 4 "Clamped
        AIS"), any mask; a track wholly given adds exactly 0 and runs no chain.  NADE estimators: exact where every NADE is wholly given or
        wholly free, MnnUnsupported otherwise.  The sum over t is NOT -log p(x_free | x_given) of the sequence: later given cells say
        something about earlier free ones, which no teacher-forced row sees.
        partial ("refuse", the default, or "importance"; RBM estimators accept and ignore it -- they take any mask): what a NADE does under
        a mask that leaves it partly given.  "importance": the importance estimator (DESIGN.md section 4 "NADE importance estimator") --
        row t of a partly given track is NLL(x_t) + log p^(x_t,given), with log p^ from num_chains clamped ancestral scans per row (seed:
        default self.seed; particles keyed by the row ids like an RBM's chains).  method "ais": the lower side, biased LOW; "raise": the
        upper side (one particle carries the targets' free cells), biased HIGH in expectation over data drawn from the model, not a bound
        per row; "both": the NllBracket.  The estimate's log_z is log p^(x_given) and its free_energy the exact NLL(x) of the whole row."""
        nll_sides(method)
        nll_partial(partial)
        cond = None
        if given_mask is not None:                                  # host checks and refusals, before any device work
            cond = given_mask_tracks(given_mask, x.shape, getattr(self, "num_tracks", 1))
            self._refuse_nll_given(cond[2], cond[3], partial, num_chains)
        refuse_host_model(self.store.device, "estimate_nll")
        dev = self.store.device if self.store.device is not None else default_device()
        inputs, targets = shifted_sequences(x.to(dev))
        self.build(inputs, targets, lengths, is_train=False, mode="eval")
        kw = {}
        if cond is not None:
            mask4, shape4, whole, some = cond
            kw["given"] = (given_codes(targets.reshape(shape4), mask4, shape4).reshape(targets.shape), whole, some)
        if partial != "refuse":
            kw["partial"] = partial
        return self._nll_rows_built(num_chains=num_chains, num_betas=num_betas, betas=betas, seed=seed, method=method, **kw)

    def _refuse_nll_given(self, whole, some, partial="refuse", num_chains=None):
        """MnnUnsupported for a conditional-NLL mask this estimator cannot honour (per track of it: every / any cell given); host only.
        partial / num_chains: estimate_nll's (nll_partial) -- an estimator that takes any mask ignores them."""

    def _step_input(self, B, device):
        """[B, ld0] staging row block of single_step: the zero padding beyond the input width is written once, every step converts its
        input into the prefix (the step's GEMM has read the previous contents by then: same stream)."""
        buf = getattr(self, "_xstep", None)
        if buf is None or buf.shape[0] != B or buf.device != torch.device(device) or buf.shape[1] != self._stack.ld0 \
                or torch.cuda.is_current_stream_capturing() != getattr(self, "_xstep_captured", False):
            buf = self._xstep = torch.zeros((B, self._stack.ld0), device=device, dtype=self.dtype)
            self._xstep_captured = torch.cuda.is_current_stream_capturing()
        return buf

    # -- sampling -------------------------------------------------------------------------------
    def generate(self, x, num_steps, given=None, temperature=1.0, max_notes=None, redraws=0, particles=None, lengths=None):
        """rnn_estimator.py:271-298: intro pass, then num_steps x {sample_single, single_step}.
        lengths (common.prompt_lengths: B ints in 1..Ti on the host): ragged prompts -- row b continues x[b, :lengths[b]], its generated
        step j being the step at absolute time lengths[b] + j; the row is, bit for bit, the one-row call on that slice with row0 + b, under
        any given / temperature / max_notes / redraws / particles, and no cell of x behind a row's length is part of its arithmetic.  The
        output, and given, stay row-relative.  None, or every entry Ti, is the call without it: the same kernels, bits and captured scan.
        particles (NADE estimators, with given; common.sampling_particles): importance resampling -- every partly given step runs C clamped
        scans and emits one, picked with probability proportional to the probability it gives the step's given cells: an approximate draw
        from p(free | this step's given cells, the past), exact as C grows; particle_ess() / particle_picks() report how approximate.  None,
        0, 1, or no given, is the call without it: the same kernels, bits and captured scan.  RBM estimators ignore it.
        redraws (0..255, with max_notes; common.sampling_redraws): the cap by rejection -- a row whose step would emit a 1 past a cap is
        drawn again, up to `redraws` times, before the truncating scan serves it; redraw_counts() reports what happened.  0, or no cap, is
        the call without it: the same kernels, bits and captured scan.
        max_notes (NADE estimators; common.sampling_max_notes): at most K ones per track and generated step -- an integer >= 0, or one per
        track (None: no cap for that track); the scan counts a track's ones, given ones included, and a free visible of a track that has
        reached its cap is a settled 0.  None is the call without it: the same kernels, bits and captured scan.
        temperature: a positive float, one per track where the estimator has tracks, or (NADE estimators) None for threshold decoding --
        common.sampling_temperature.  1.0 is the call without it: the same kernels, bits and captured scan.
        x [B,Ti,Din]; returns samples u8 [B,num_steps,num_output].  On the device the whole scan is ONE hipGraph
        replay (captured per shape / num_steps / seed, see common.ScanGraphs); same kernels, same RNG counters, same bits.
        given (optional): codes u8 [B, num_steps, num_output] in the generator's feature order (common.given_codes): a clamped visible is
        emitted as given and fed forward like a draw, every free one is drawn from the uniform it draws unconditioned."""
        if given is not None:
            check_given(given, x.shape[0], num_steps, self._num_output)
            given = given.contiguous()
        max_notes = self._max_notes(max_notes)
        temperature = self._temperature(temperature)
        redraws = sampling_redraws(redraws, max_notes, temperature)
        particles = self._particles(particles, temperature, max_notes, given)
        if max_notes is not None:
            refuse_host_model(self.store.device, "generate(max_notes=)")
        if particles:
            refuse_host_model(self.store.device, "generate(particles=)")
        lengths = prompt_lengths(lengths, x.shape[0], x.shape[1])
        if lengths is not None:
            self._refuse_prompt_lengths("generate(lengths=)")
        self._redraw_live = redraws > 0
        self._particle_live = None          # (with particles: set by ScanGraphs.generate to the arrays the scan writes)

        def stale():
            self._packed_step = -1
        return ScanGraphs.generate(self, (tuple(x.shape), x.dtype, int(num_steps), self.seed, self.row0), x, num_steps, given,
                                   temperature, self._generate_scan, stale, max_notes, redraws, particles,
                                   stats_shape=(int(num_steps), self.num_tracks, x.shape[0]) if particles else None,
                                   **({} if lengths is None else dict(lengths=prompt_lengths_device(lengths, x.device))))

    def particle_ess(self):
        """The effective sample size (sum w)^2 / sum w^2 of every scan of the last generate call or session chunk that ran with particles:
        f32 [B, num_steps, tracks] on the host, in [1, C] -- C where nothing was resampled (no given cell behind a free one), near 1 where
        one particle carried the weight and the emitted vector is little better than the clamped scan's.  None without particles.
        Synchronises."""
        return particle_stats(self, 0)

    def particle_picks(self):
        """The picked particle of every scan, int32 [B, num_steps, tracks] (0: the scan of the call without particles); see particle_ess."""
        return particle_stats(self, 1)

    def redraw_counts(self):
        """(redrawn, fallback) of the last generate call or session chunk: how many scans -- one per row, track and generated step -- were
        drawn again at least once, and how many of them fell back to the truncating scan (and carry its bias).  Ints; synchronises."""
        return redraw_counts(self)

    def _generate_scan(self, x, num_steps, given=None, temperature=1.0, max_notes=None, redraws=0, particles=0, lengths=None):
        """The scan of generate; lengths: normalised prompt lengths on the device (int32 [B]; a static input of a captured scan) or None."""
        self._materialize(x.shape[-1])
        self._rnn.build_cell(False)
        if redraws:
            redraw_cell(self, x.device).zero_()        # the call's statistics start at zero (in a captured scan: a fill node of the graph)
        with self._sampling_scope():
            if self.det_sampling:
                whole = self._scan_in_one_call(x, num_steps, given, temperature, max_notes, redraws, particles,     # LSTM-(Multi)NADE on a byte piano-roll: mnn_generate_scan runs the whole scan
                                               **({} if lengths is None else dict(lengths=lengths)))
                if whole is not None:
                    return whole
                state = self.steps(x) if lengths is None else self._det_steps(x, None, lengths)
            else:
                self._ensure_packed()
                state = self._get_state(x, lengths=None, last_outputs=True)
            # the first chain's start: the intro's last row -- with prompt lengths every row's own, gathered on the device
            last_row = x[:, -1, :] if lengths is None else last_prompt_rows(x, lengths)
            return self._scan_steps(state, last_row, num_steps, DrawAt(self.seed, self.row0, 0), given, temperature, max_notes, redraws, particles)[0]

    def _scan_steps(self, state, last_row, n, at0, given=None, temperature=1.0, max_notes=None, redraws=0, particles=0):
        """The step loop of a single generator (rnn_estimator.py:283-298): n x {sample_single, single_step} from `state` and the last emitted
        row, step j drawing at at0's position moved on by j steps under given[:, j] -> (samples u8 [B, n, num_output], state, last row).
        generate runs it from step 0, a session's chunk from where the piece stands.  max_notes (normalised; None: the call without it)
        makes every step a sample_single_capped, which the estimators that have caps define; redraws (normalised; 0: nothing changes) a
        sample_single_redrawn that adds to the generator's statistics cell; particles (normalised; 0: nothing changes) a
        sample_single_resampled that writes step j's plane of the generator's particle statistics."""
        out = []
        cells = particle_cells(self, n, self.num_tracks, last_row.shape[0], last_row.device) if particles and given is not None else None
        sample = self.sample_single if max_notes is None else functools.partial(self.sample_single_capped, max_notes=max_notes)
        if redraws:
            sample = functools.partial(self.sample_single_redrawn, max_notes=max_notes, redraws=redraws, redraw_stats=redraw_cell(self, last_row.device))
        for j in range(n):
            if cells is not None:
                sample = functools.partial(self.sample_single_resampled, particles=particles, ess=cells[0][j], pick=cells[1][j])
            last_row, _ = sample(last_row, state, given=None if given is None else given[:, j], temperature=temperature,
                                 at=at0._replace(step=at0.step + j))
            state = self.single_step(last_row, state)
            out.append(last_row)
        return torch.stack(out, 1), state, last_row


# ------------------------------------------------------------------------------------------------
class RnnNade(RnnEstimator):
    """models/generators/rnn_nade.py: LSTM -> Dense -> NADE."""

    def __init__(self, num_dims, num_hidden, num_hidden_rnn, keep_prob=1.0, internal_bias=False, name="rnn-nade", track_name="all", **kw):
        self._tracks = getattr(self, "_tracks", ["all"])
        super().__init__(num_dims, num_hidden, num_hidden_rnn, keep_prob, internal_bias, name, track_name, **kw)
        self._num_output = self.num_tracks * self.num_dims

    tracks = property(lambda self: self._tracks)
    num_tracks = property(lambda self: len(self._tracks))

    def _init_estimator(self):
        # internal_bias=True (nade.py:69-87, rnn_nade.py:245-251): the NADE's own b_enc / b_dec are ADDED to the Dense outputs.  A broadcast
        # add in front of the scan is the same as adding them to the Dense layer's bias vector, so the kernels never see them: the forward GEMM
        # takes dense/bias + [b_enc | b_dec] (one axpby over n_out words), and their gradient is the Dense bias gradient (same column sums).
        self._nades = [NADE(self.num_dims, self.num_hidden[-1], internal_bias=False, name=f"nade_{m}") for m in range(self.num_tracks)]
        self._nade = self._nades[0]

    def _declare(self, num_inputs):
        """Variable order rnn, nade(s), dense (rnn_nade.py:117-120)."""
        M, D, Hn, R = self.num_tracks, self.num_dims, self.num_hidden[-1], self.num_hidden_rnn[-1]
        self._rnn.declare(self.store, num_inputs, self._gen)
        # all tracks' NADE weights are contiguous so that the kernels see [tracks, D, Hn]
        from .common import truncated_normal
        std = 1.0 / (D ** 0.5)
        self.store.declare("nade/w_enc", (M, D, Hn), truncated_normal(self._gen, std))
        self.store.declare("nade/w_dec", (M, D, Hn), truncated_normal(self._gen, std))
        if self.internal_bias:                          # adjacent in the flat buffer, in the Dense output's column order [tracks x Hn | tracks x D]
            self.store.declare("nade/b_enc", (M, Hn), truncated_normal(self._gen, std))
            self.store.declare("nade/b_dec", (M, D), truncated_normal(self._gen, std))
        n_out = M * (D + Hn)
        self.store.declare("dense/kernel", (R, n_out), glorot_uniform(self._gen, R, n_out))
        self.store.declare("dense/bias", (n_out,), zeros_init)
        self.n_out = n_out
        self.ldo = ops.round_up(n_out, 64)

    def _materialize(self, num_inputs):
        first = self.store.theta is None
        super()._materialize(num_inputs)
        if first:
            for m, nd in enumerate(self._nades):            # per-track views of the stacked NADE weights
                nd._w_enc_t, nd._w_dec_t = self.store["nade/w_enc"][m], self.store["nade/w_dec"][m]

    def _pack_estimator(self):
        dev = self.store.theta.device
        R = self.num_hidden_rnn[-1]
        self._fc_t = torch.empty((self.n_out, R), device=dev, dtype=self.dtype)        # [n_out, R]: forward B operand
        ops.transpose(self.store["dense/kernel"], self._fc_t)
        self._fc_p = torch.zeros((R, self.ldo), device=dev, dtype=self.dtype)           # [R, n_out]: dgrad B operand
        ops.convert2d(self.store["dense/kernel"], self._fc_p[:, :self.n_out])
        if self.internal_bias:
            self._fc_bias = torch.empty(self.n_out, device=dev)
            ops.axpby(1.0, self.store["dense/bias"], 1.0, self._internal_flat(self.store.theta), self._fc_bias)
        else:
            self._fc_bias = self.store["dense/bias"]
        if self._nade_mfma():                           # 16-bit copy of the decoder weights for the matrix-core NADE kernels
            M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
            if self._nade_exact():                      # fp16 mode: the weights as f16 hi | lo pairs for the split-operand MFMA form
                self._wdec_bf = torch.empty((M, D, Hn), device=dev, dtype=torch.float32)
                ops.nade_f32_pack(self.store["nade/w_dec"].view(M * D, Hn), self._wdec_bf.view(M * D, Hn))
            else:
                self._wdec_bf = torch.empty((M, D, Hn), device=dev, dtype=torch.bfloat16)
                ops.convert2d(self.store["nade/w_dec"].view(M * D, Hn), self._wdec_bf.view(M * D, Hn))

    def _internal_flat(self, flat):
        """[b_enc | b_dec] of all tracks as one n_out-long slice of a flat parameter-shaped buffer (theta or its gradient)."""
        o = self.store.offset("nade/b_enc")
        return flat[o:o + self.n_out]

    nade_mfma = flag("MULTINN_NADE_MFMA")

    nade_dense_above = value("MULTINN_NADE_DENSE_ABOVE")   # density above which the f32 scan replaces the matrix-core form

    def _nade_fwd(self, v, out, rw, nll, cond_p, d_out, a_fin, n_rows_dev=None, unsafe=None):
        M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
        exact = self._nade_exact()
        if self.nade_dense_above >= 1.0:                 # gate off: always the matrix-core form
            return ops.nade_logprob_fwd_auto(v, out, self.store["nade/w_enc"], self.store["nade/w_dec"], self._wdec_bf, M, D, Hn, None, None,
                                             1.0, rw, nll, cond_p, d_out, a_fin, exact=exact, n_rows_dev=n_rows_dev)
        if getattr(self, "_gate", None) is None or self._gate.device != out.device:
            self._gate = torch.zeros(1 + ops.DENSITY_SLOTS, device=out.device, dtype=torch.int32)            # [gate | partial counts]
        counted = bool(getattr(self, "_v_counted", False)) and rw is not None      # (the on-demand conditionals pass of a train build runs later: not counted)
        return ops.nade_logprob_fwd_auto(v, out, self.store["nade/w_enc"], self.store["nade/w_dec"], self._wdec_bf, M, D, Hn, self._gate[:1],
                                         self._gate[1:], self.nade_dense_above, rw, nll, cond_p, d_out, a_fin, exact=exact, counted=counted,
                                         n_rows_dev=n_rows_dev, unsafe=unsafe)

    # fp16 mode: the split-operand matrix-core scan (nade_mfma.hip, SPLIT: f16 hi + lo pairs, three 16-bit MFMA products) or the f32 vector scan
    nade_exact = flag("MULTINN_NADE_EXACT_MFMA")

    def _nade_mfma(self):
        """The matrix-core NADE forward is in use: bf16 mode (16-bit operands) or fp16 mode (hi + lo operand pairs, 22 bits), and a hidden width it covers;
        otherwise the f32 VALU kernels."""
        if not (self.nade_mfma and ops.nade_mfma_ok(self.num_hidden[-1])):
            return False
        return self.dtype == torch.bfloat16 or (self.dtype == torch.float16 and self.nade_exact)

    def _nade_exact(self):
        """fp16 mode: BASELINE.json's 1e-4 on every conditional needs more than the 8 / 11 bits of a single bf16 / f16 operand in the decoder
        dot products (the LSTM / Dense operands do not): the matrix-core scan carries them as f16 hi + lo pairs there."""
        return self.dtype == torch.float16

    # -- forward --------------------------------------------------------------------------------
    def build(self, x=None, y=None, lengths=None, is_train=None, mode="eval"):
        """rnn_nade.py:64-124.  x inputs [B,T,Din], y targets [B,T,tracks*D] (u8 or float)."""
        return drive(self._build_co(x, y, lengths, is_train, mode))

    def _build_co(self, x=None, y=None, lengths=None, is_train=None, mode="eval"):
        """`build` as a generator function (drive / drive_group: the LSTM recurrences are yielded to the driver)."""
        Generator.build(self, x, y, lengths, is_train, mode)
        self._materialize(x.shape[-1] if x is not None else self._num_inputs)
        self._rnn.build_cell(is_train)
        if mode in ("train", "eval"):
            B, T, _ = x.shape
            M, D = self.num_tracks, self.num_dims
            x_tm = self._to_time_major_inputs(x)
            # rnn_multinade.py:97-101: reshape(flat,[-1,D,M]) unstacked on the last axis (track-minor)
            v = y.to(torch.uint8).transpose(0, 1).reshape(T, B, D, M).permute(3, 0, 1, 2).contiguous() if M > 1 \
                else y.to(torch.uint8).transpose(0, 1).contiguous().view(1, T, B, D)
            compact = None
            if lengths is not None and mode == "train" and self.dtype in ops.H16 and self.ragged_compact and x.is_cuda:
                # ragged window of a generator that trains on encoder outputs (composer: RnnMultiNADE; jamming / feedback with NADE generators):
                # Dense + NADE on the valid rows only, as build_pianoroll does for the joint mode (see there); the targets and row weights are
                # brought into compact order here (the piano-roll pass does it for the joint path)
                dev = x.device
                len_dev = lengths.to(device=dev, dtype=torch.int32).contiguous()
                n_total_dev = None
                if dp_active():
                    n_total_dev = len_dev.clamp(0, T).sum().float().reshape(1)
                    torch.distributed.all_reduce(n_total_dev)
                idx, inv, hdr = ops.ragged_index(len_dev, B, T, n_total_dev, self._stack.loss_scale_rows if self.dtype == torch.float16 else 0.0)
                compact = dict(idx=idx, inv=inv, hdr=hdr, hdr_f=hdr.view(torch.float32))
                v = v.view(M, T * B, D).index_select(1, idx.long()).view(M, T, B, D)          # every row of the permutation: padding rows behind the valid ones
                k = torch.arange(T * B, device=dev, dtype=torch.int32)
                rw = torch.where(k < hdr[0], compact["hdr_f"][1], torch.zeros((), device=dev))
                lengths = len_dev
                self._n_valid = None
            else:
                rw = self._row_weight(lengths, B, T, x.device)
            yield from self._forward_tm_co(x_tm, v, rw, lengths, B, T, train=(mode == "train"), compact=compact)
        self._is_built = True

    # MULTINN_RAGGED_COMPACT=0: ragged windows keep their padding rows in the Dense + NADE part (weight 0), as before round 6
    ragged_compact = flag("MULTINN_RAGGED_COMPACT")
    ragged_gemm_rows = flag("MULTINN_RAGGED_GEMM_ROWS")     # the Dense GEMMs of a compacted window skip their padding too (ops.gemm_tn m_rows / k_rows)

    def build_pianoroll(self, x_u8, lengths=None, is_train=True, mode="train", n_total_dev=None):
        """Fast joint path: x_u8 [B,T,P,M] piano-roll batch; fuses multinn_joint.py:83-89,132-139
        (zero first step, inputs = enc[:, :-1], targets = enc[:, 1:]) into one kernel.
        n_total_dev (f32 [1], optional): valid rows of ALL ranks of a ragged window, for callers that must not run a collective here
        (a captured step under data parallelism)."""
        if self.num_tracks != 1:
            raise ValueError("build_pianoroll is the joint (single NADE) path")
        B, T, P, Mtr = x_u8.shape
        D = P * Mtr
        self._materialize(D)
        Generator.build(self, None, None, lengths, is_train, mode)
        self._rnn.build_cell(is_train)
        dev = x_u8.device
        x_tm = torch.empty((T, B, self._stack.ld0), device=dev, dtype=self.dtype)
        v = torch.empty((T, B, D), device=dev, dtype=torch.uint8)
        rw = torch.empty(T * B, device=dev)
        # Ragged window, 16-bit train step: Dense + NADE run on the VALID rows only (the reference drops padded rows before the NADE:
        # utils/sequences.py:6-37, rnn_nade.py:91-92,225; the LSTM still steps them: impute_finished=False).  The compaction index, the row
        # count, 1 / n_valid and the f16 loss scale all live on the device (ops.ragged_index): nothing of the step depends on a host-side
        # count, so graphed_train_step captures it once for any lengths.
        compact = None
        if lengths is not None and mode == "train" and self.dtype in ops.H16 and self.ragged_compact:
            len_dev = lengths.to(device=dev, dtype=torch.int32).contiguous()
            if n_total_dev is None and dp_active():
                n_total_dev = len_dev.clamp(0, T).sum().float().reshape(1)
                torch.distributed.all_reduce(n_total_dev)
            idx, inv, hdr = ops.ragged_index(len_dev, B, T, n_total_dev, self._stack.loss_scale_rows if self.dtype == torch.float16 else 0.0)
            compact = dict(idx=idx, inv=inv, hdr=hdr, hdr_f=hdr.view(torch.float32))
            lengths = len_dev
            n_valid = 0
            self._n_valid = None                    # device-side only (compact["hdr"])
        elif lengths is not None:
            n_tot = lengths.sum().to(dev).float()
            if dp_active():
                torch.distributed.all_reduce(n_tot)
            n_valid = int(n_tot)
            self._n_valid = max(n_valid, 1)
        else:
            n_valid = B * T * world()[1]
            self._n_valid = max(n_valid, 1)
        x_tmT = None
        if mode == "train" and self.dtype in ops.H16:              # the same pass also writes x^T, layer 1's weight-gradient operand
            self._ensure_packed()
            x_tmT = self._stack.input_T(T, B, dev)                  # (a view of the layer's concatenated operand where that form runs)
            if x_tmT is None:
                Np = ops.round_up(T * B, 64)
                x_tmT = (torch.zeros if Np != T * B else torch.empty)((self._stack.ld0, Np), device=dev, dtype=self.dtype)
        # the NADE forward's density gate needs the number of set target cells: counted by this pass while it writes them (no second pass over v)
        cnt = None
        if x_tmT is not None and self._nade_mfma() and self.nade_dense_above < 1.0:
            if getattr(self, "_gate", None) is None or self._gate.device != dev:
                self._gate = torch.zeros(1 + ops.DENSITY_SLOTS, device=dev, dtype=torch.int32)            # [gate | partial counts]
            cnt = self._gate[1:]
        self._v_counted = ops.pianoroll_shift_timemajor(x_u8.view(B, T, D), lengths, x_tm, v, rw, n_valid, inputs_t=x_tmT, count=cnt,
                                                        compact=(compact["inv"], compact["hdr"]) if compact else None)
        self._forward_tm(x_tm, v.view(1, T, B, D), rw, lengths, B, T, train=(mode == "train"), x_tmT=x_tmT, compact=compact)
        self._v_counted = False
        self._is_built = True

    def _forward_tm(self, x_tm, v, rw, lengths, B, T, train, x_tmT=None, compact=None):
        return drive(self._forward_tm_co(x_tm, v, rw, lengths, B, T, train, x_tmT, compact))

    def _forward_tm_co(self, x_tm, v, rw, lengths, B, T, train, x_tmT=None, compact=None):
        """compact (build_pianoroll, ragged windows): v and rw arrive in COMPACT row order; the LSTM output is gathered into it (rows behind the
        valid ones zeroed) and everything from the Dense layer on -- out, nll, d_out, a_fin -- lives in compact order too."""
        M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
        N, dev = T * B, x_tm.device
        self._ensure_packed()
        kp = self._rnn.effective_keep_prob()
        y, ctx, _ = yield from self._stack.forward_co(x_tm, kp, self.seed, self.row0, save=train, state0=self._state0(B),
                                                      step_dev=self.store.step_dev, state_grad=train)
        if ctx and x_tmT is not None:
            ctx[0]["inT"] = x_tmT
        nrows = None
        if compact is not None:
            R = y.shape[-1]
            Np = ops.round_up(N, 64)
            y_c = torch.empty((N, R), device=dev, dtype=self.dtype)
            y_cT = (torch.zeros if Np != N else torch.empty)((R, Np), device=dev, dtype=self.dtype) if train else None
            ops.rows_gather16(y.view(N, R), compact["idx"], compact["hdr"], y_c, y_cT)
            compact["y_cT"] = y_cT
            y_dense, nrows = y_c, compact["hdr"]
        else:
            y_dense = y.view(N, -1)
        out = torch.empty((N, self.ldo), device=dev)      # columns >= n_out are padding of the row pitch: never read
        ops.gemm_tn(y_dense, self._fc_t, out[:, :self.n_out], bias=self._fc_bias, m_rows=nrows if self.ragged_gemm_rows else None)      # (compact: row tiles of padding are skipped)
        nll = torch.empty((M, N), device=dev)
        cond_p = None if train else torch.empty((M, N, D), device=dev)     # the train step needs the loss only: 4 N D bytes less to write per
        rw_m = rw / M if M > 1 else rw                                       # step; `cond_probs` fills it on demand (see the property)
        d_out = None
        if train:
            d_out = torch.empty((N, self.ldo), device=dev)
            if self.ldo != self.n_out and self.dtype == torch.float32:
                d_out[:, self.n_out:].zero_()       # fp32: d_out itself is the dgrad operand; bf16: grad_rows_fanout writes the zero padding
        a_fin = torch.empty((M, N, Hn), device=dev) if train else None
        # gradient seed only (the reported loss stays unscaled): the mode's weight of this generator's loss, and the f16 loss scale
        # (f16: times the DYNAMIC multiplier m of the store, a device word a skipped step halves -- ParamStore.ls_dyn; _unscale gets 1 / (scale m))
        dyn = self.store.ls_dyn if (train and self.dtype == torch.float16) else None
        if compact is not None:                         # the scale is a device word (hdr[2]); its inverse is applied by _unscale
            ls = compact["hdr_f"][2:3] if (train and self.dtype == torch.float16) else 1.0
            if torch.is_tensor(ls):
                rw_g = rw_m * (ls * dyn[0:1] * self.grad_scale)
                ls = compact["hdr_f"][3:4] * dyn[1:2]    # what _unscale multiplies by
            else:
                rw_g = rw_m if self.grad_scale == 1.0 else rw_m * self.grad_scale
        elif train and self._n_valid is None and self.dtype == torch.float16:     # ragged_on_device without compaction: the device-side scale
            rw_g = rw_m * (self._ls_dev * dyn[0:1] * self.grad_scale)
            ls = dyn[1:2] / self._ls_dev
        else:
            ls = self._stack.loss_scale(self._n_valid) if (train and self._n_valid is not None) else 1.0
            gs = self.grad_scale * ls
            if dyn is not None:
                rw_g = rw_m * (dyn[0:1] * gs)
                ls = dyn[1:2] * (1.0 / ls)               # a tensor: _unscale multiplies by it
            else:
                rw_g = rw_m if gs == 1.0 else rw_m * gs
        if self._nade_mfma():
            # bf16 compute mode: the decoder dot products run as a block-sparse bf16 GEMM over each row's hidden states while the batch is
            # piano-roll-sparse; a dense batch takes the f32 vector form (decided on the device, per launch: ops.nade_logprob_fwd_auto)
            # (train, density gate in use: the dense forward also counts the waves that left |a| <= 40 -- none = the dense backward's licence, see ops.nade_logprob_bwd)
            unsafe = torch.empty(1, device=dev, dtype=torch.int32) if (train and self.nade_dense_above < 1.0) else None
            self._nade_fwd(v.view(M, N, D), out, rw_g if train else None, nll, cond_p, d_out, a_fin, n_rows_dev=nrows, unsafe=unsafe)
        else:
            assert compact is None or Hn <= 256, "compacted rows: the f32 scan covers Hn <= 256"
            ops.nade_logprob_fwd(v.view(M, N, D), out, self.store["nade/w_enc"], self.store["nade/w_dec"], M, D, Hn,
                                 rw_g if train else None, nll, cond_p, d_out, a_fin, n_rows_dev=nrows)
        loss = torch.zeros(1, device=dev)
        ops.weighted_sum(nll.view(-1), rw_m.repeat(M) if M > 1 else rw_m, loss)      # statistical.py:34 / rnn_multinade.py:202-203
        self._ctx = dict(x_tm=x_tm, v=v, rw=rw_m, y=y, lstm=ctx, out=out, d_out=d_out, a_fin=a_fin, kp=kp, seed=self.seed, B=B, T=T, ls=ls,
                         compact=compact, unsafe=unsafe if self._nade_mfma() else None)
        self._nll_tm, self._cond_tm, self._loss = nll, cond_p, loss
        self._flat_idx = None
        self._lengths = lengths
        self._metrics = {"batch/loss": loss, "log_likelihood": loss}
        self._metrics_upd = []

    # -- API-order views of the flat outputs (b-major then t, sequences.py:30-31; RnnEstimator._idx) ---------------
    @property
    def log_probs(self):
        r = [self._nll_tm[m][self._idx()] for m in range(self.num_tracks)]
        return r[0] if self.num_tracks == 1 else r

    def _refuse_nll_given(self, whole, some, partial="refuse", num_chains=None):
        if any(s and not w for w, s in zip(whole, some)):
            if nll_partial(partial, num_chains) == "refuse":
                raise MnnUnsupported(NADE_MASK_REFUSAL)

    def _nll_rows_built(self, method="ais", given=None, partial="refuse", num_chains=64, seed=None, **ais):
        """The exact NLL rows of the last build (API order, valid rows), summed over the NADE tracks: an NllEstimate with stderr 0, whatever
        the method ("both": the bracket of that one estimate with itself).  given (optional): (codes, whole, some) as RnnRBM._nll_rows_built
        takes them -- the NADE of a wholly given track adds 0, that of a wholly free track its rows (the tracks of a step are independent
        given the history); any other mask is refused, or with partial "importance" estimated: a partly given track adds NLL(x) + log
        p^(x_given) (nade_is_side: num_chains particles per row keyed by the row ids of build, seed default self.seed, the tracks apart
        by their elements m D + i), the parts combined by NllEstimate.total -- so log_z sums the log p^ and free_energy the exact rows of
        the partly given tracks.  The remaining AIS arguments are ignored."""
        sides = nll_sides(method)
        idx = self._idx()
        M = self.num_tracks
        free, part = range(M), []
        if given is not None:
            self._refuse_nll_given(given[1], given[2], partial, num_chains)
            free = [m for m in free if not given[1][m]]
            part = [m for m in free if given[2][m]]
            if not free:
                return given_nll_result(method, idx.numel(), idx.device)
        if not part or idx.numel() == 0:
            est = NllEstimate(sum(self._nll_tm[m][idx] for m in free))
            return nll_result(method, (est, est))
        cx = self._ctx
        B, T, D, Hn = cx["B"], cx["T"], self.num_dims, self.num_hidden[-1]
        dev = cx["out"].device
        # the codes of the partly given tracks as time-major planes (track-minor features d M + m: build's reshape of the targets); every
        # other track all free: its scans have nothing to weigh
        planes = given[0].to(torch.uint8).reshape(B, T, D, M).permute(3, 1, 0, 2).reshape(M, T * B, D)[:, idx]
        codes = torch.full_like(planes, 255)
        codes[part] = planes[part]
        tgt = cx["v"].view(M, T * B, D)[:, idx].contiguous()
        bias = cx["out"][idx].contiguous()
        ids = self._row_ids(B, T, dev)[idx].to(torch.int32).contiguous()
        rows = {m: self._nll_tm[m][idx] for m in free}
        s0 = self.seed if seed is None else seed
        out = []
        for side in sides:
            est = nade_is_side(side, bias, self.store["nade/w_enc"], self.store["nade/w_dec"], M, D, Hn, codes, tgt, rows, part, num_chains, s0, ids)
            out.append(NllEstimate.total([est[m] if m in est else NllEstimate(rows[m]) for m in free]))
        return nll_result(method, out)

    @property
    def cond_probs(self):
        if self._cond_tm is None:           # built in train mode: one more decoder pass over the saved Dense output, conditionals only
            cx = self._ctx
            M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
            N = cx["B"] * cx["T"]
            cp = torch.empty((M, N, D), device=cx["out"].device)
            if self._nade_mfma():
                self._nade_fwd(cx["v"].view(M, N, D), cx["out"], None, None, cp, None, None,
                               n_rows_dev=cx["compact"]["hdr"] if cx.get("compact") else None)
            else:
                ops.nade_logprob_fwd(cx["v"].view(M, N, D), cx["out"], self.store["nade/w_enc"], self.store["nade/w_dec"], M, D, Hn, None, None, cp, None,
                                     None)
            self._cond_tm = cp
        r = [self._cond_tm[m][self._idx()] for m in range(self.num_tracks)]
        return r[0] if self.num_tracks == 1 else r

    @property
    def _outputs(self):
        """rnn_nade.py:100: cast(cond_probs >= .5)."""
        cp = self.cond_probs
        return (cp >= 0.5).float() if self.num_tracks == 1 else [(c >= 0.5).float() for c in cp]

    def build_metrics(self, targets, predictions, cond_probs=None, log_probs=None):
        return self._nade.build_metrics(targets, predictions, cond_probs, log_probs)

    # -- backward -------------------------------------------------------------------------------
    def backward(self):
        """Gradient of metrics['batch/loss'] wrt rnn + nade + dense variables into store.grad."""
        return drive(self._backward_co())

    def _backward_co(self):
        cx = self._ctx
        if cx["d_out"] is None:
            raise RuntimeError("build(..., mode='train') must run before train()")
        M, D, Hn, R = self.num_tracks, self.num_dims, self.num_hidden[-1], self.num_hidden_rnn[-1]
        B, T = cx["B"], cx["T"]
        N, dev = B * T, cx["out"].device
        g = self.store.gviews
        self.store.grad.zero_()
        d_out = cx["d_out"]
        compact = cx.get("compact")
        ops.nade_logprob_bwd(cx["v"].view(M, N, D), cx["out"], self.store["nade/w_enc"], self.store["nade/w_dec"], M, D, Hn, cx["a_fin"],
                             d_out, g["nade/w_enc"], g["nade/w_dec"], n_rows_dev=compact["hdr"] if compact else None,
                             unsafe=cx.get("unsafe"))
        # dense: dK[R,n_out] = y^T d_out ; db = sum d_out ; dy = d_out K^T
        Np = ops.round_up(N, 64)
        zalloc = torch.zeros if Np != N else torch.empty
        yT = cx["lstm"][-1].get("yT") if cx["lstm"] else None      # emitted by the persistent recurrence
        if compact is not None:
            yT = compact["y_cT"]                                    # compact row order, like d_out (rows behind the valid ones are zero in both)
        if yT is None:
            yT = zalloc((R, Np), device=dev, dtype=self.dtype)
            ops.transpose(cx["y"].view(N, R), yT)
        doT = zalloc((self.n_out, Np), device=dev, dtype=self.dtype)
        if self.dtype == torch.float32:
            ops.transpose(d_out[:, :self.n_out], doT)
            ops.bias_grad(d_out[:, :self.n_out], g["dense/bias"], accumulate=True)
            do_c = d_out
        else:                               # one pass over d_out: bf16 copy, bf16 transpose, bias gradient
            do_c = torch.empty((N, self.ldo), device=dev, dtype=self.dtype)
            ops.grad_rows_fanout(d_out, self.n_out, do_c, doT, g["dense/bias"])
        if self.internal_bias:              # d b_enc / d b_dec = the Dense bias gradient (same column sums of d_out)
            gi = self._internal_flat(self.store.grad)
            ops.axpby(1.0, gi, 1.0, g["dense/bias"], gi)
        nrows = compact["hdr"] if (compact is not None and self.ragged_gemm_rows) else None      # compact: the row sums stop at the valid rows, padding row tiles are skipped
        ops.gemm_tn(yT, doT, g["dense/kernel"], accumulate=True, split_k=LstmStack._split_k(R, self.n_out, Np), k_rows=nrows)
        del yT, doT
        dy = torch.empty((N, R), device=dev)
        ops.gemm_tn(do_c, self._fc_p, dy, m_rows=nrows)
        if compact is not None:                                     # back into time-major order for the LSTM backward (padding rows: 0)
            dy_c, dy = dy, torch.empty((N, R), device=dev)
            ops.rows_scatter_f32(dy_c, compact["inv"], compact["hdr"], dy)
        self._dx = yield from self._lstm_backward_co(dy, cx)
        self._unscale(cx.get("ls", 1.0))

    def train_step(self, x_u8, lengths, optimizer, lr=None):
        """One optimiser step on a piano-roll batch (train.py:178-189's sess.run)."""
        self.build_pianoroll(x_u8, lengths, is_train=True, mode="train")
        self.train(optimizer, lr)
        return self._loss

    def capturable(self, shape, ragged):
        """Whether windows of this shape (full-length, or ragged) may train as replays of graphed_train_step (driver._captured_step): only the
        paths the captured step is tested on -- the two-layer persistent recurrence and the row-parallel (CU-resident / cluster) one; ragged
        windows where they run compacted (16-bit, one track: every row count lives on the device, so one graph serves any lengths)."""
        B, T = shape[0], shape[1]
        stack = getattr(self, "_stack", None)
        if stack is None or stack.packed is None or not (stack._persist(B, T) or stack._rowpar(B, T)):
            return False
        if self.learn_zero_state and not stack._rowpar_state0(B, T):
            return False                    # a learned start off the resident / cluster kernels trains on the launch-per-timestep path, eagerly
        return not ragged or (self.ragged_compact and self.dtype in ops.H16 and self.num_tracks == 1)

    def graphed_train_step(self, x_u8, optimizer, lr=None, warmup=2, lengths=None):
        """Capture one whole optimiser step (plumbing, packing, forward, backward, clip, Adam: ~300 launches) into
        hipGraphs and return ``run(x=None, lengths=None) -> loss``: the T-step recurrences are launch-bound on the host otherwise.
        Step-dependent values (dropout seed, Adam step) are read from store.step_dev on the device.  Under data
        parallelism the ONE gradient all-reduce stays an eager torch.distributed call between two graphs
        (forward+backward | clip+Adam), so nothing of RCCL is captured.

        lengths (int32 [B], optional): capture the RAGGED step.  The captured graph holds a static copy of the lengths; the compaction index,
        the valid-row count, 1 / n_valid and the f16 loss scale are computed from it ON THE DEVICE inside the graph (ops.ragged_index), so one
        capture serves every later ``run(x, lengths)``.  16-bit modes only (the compacted path); under data parallelism the total row count of
        all ranks is all-reduced eagerly in front of the replay."""
        static_x = x_u8.clone()
        ragged = lengths is not None
        if ragged and not (self.dtype in ops.H16 and self.ragged_compact):
            raise ValueError("graphed_train_step(lengths=...) needs the compacted ragged path (16-bit precision, MULTINN_RAGGED_COMPACT unset)")
        dev = x_u8.device
        T = x_u8.shape[1]
        static_len = lengths.to(device=dev, dtype=torch.int32).clone() if ragged else None
        multi = dp_active()
        static_ntot = torch.zeros(1, device=dev) if (ragged and multi) else None

        def set_total():
            if static_ntot is not None:
                static_ntot.copy_(static_len.clamp(0, T).sum().float().reshape(1))
                torch.distributed.all_reduce(static_ntot)

        me = weakref.ref(self)                         # (run holds no model: capture_train_step)

        def feed(x=None, lengths=None):
            if x is not None:
                static_x.copy_(x)
            if lengths is not None:
                if not ragged:
                    raise ValueError("this step was captured for full-length windows: capture it with lengths= to feed ragged ones")
                static_len.copy_(lengths.to(device=dev, dtype=torch.int32))
                set_total()
                me().lengths_fed()

        set_total()
        run = self._capture_step(feed, lambda: self.build_pianoroll(static_x, static_len, is_train=True, mode="train", n_total_dev=static_ntot),
                                 optimizer, lr, warmup)
        run.ragged = ragged
        return run

    # -- state / sampling -----------------------------------------------------------------------
    def zero_state(self, batch_size):
        """rnn_nade.py:158-171 (RnnMultiNADE: per-track lists, R8)."""
        self._materialize(self._num_inputs)
        dev = self.store.theta.device
        z = lambda n: torch.zeros((batch_size, n), device=dev)
        be = z(self.num_hidden[-1]) if self.num_tracks == 1 else [z(self.num_hidden[-1]) for _ in self._tracks]
        bd = z(self.num_dims) if self.num_tracks == 1 else [z(self.num_dims) for _ in self._tracks]
        return RnnEstimatorStateTuple(be, bd, self._get_rnn_zero_state(batch_size))

    def _build_biases(self, outputs):
        """rnn_nade.py:234-251 / rnn_multinade.py:231-256: b_enc block(s) first, then b_dec block(s)."""
        M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
        be = [outputs[:, m * Hn:(m + 1) * Hn] for m in range(M)]
        bd = [outputs[:, M * Hn + m * D:M * Hn + (m + 1) * D] for m in range(M)]
        return (be[0], bd[0]) if M == 1 else (be, bd)

    def _dense(self, h):
        out = torch.empty((h.shape[0], self.ldo), device=h.device)        # columns [n_out, ldo) are alignment only: no kernel reads them
        ops.gemm_tn(h, self._fc_t, out[:, :self.n_out], bias=self._fc_bias)
        return out

    def _state_from_dense(self, out, rnn_state):
        be, bd = self._build_biases(out)
        st = RnnEstimatorStateTuple(be, bd, rnn_state)
        st.dense = out
        return st

    def _get_state(self, inputs, lengths=None, initial_state=None, last_outputs=False):
        """rnn_nade.py:173-232."""
        self._materialize(inputs.shape[-1])
        self._ensure_packed()
        if inputs.dim() == 2:
            inputs = inputs[:, None, :]
        B, T, _ = inputs.shape
        x_tm = self._to_time_major_inputs(inputs)
        st0 = [(c, h) for c, h in initial_state.rnn_state] if initial_state is not None else self._state0(B)
        y, _, final = self._stack.forward(x_tm, self._rnn.effective_keep_prob(), self.seed, self.row0, save=False, state0=st0)
        if last_outputs:
            out = self._dense(y[-1].contiguous())
        else:
            out = self._dense(y.view(T * B, -1))[flat_index(lengths, B, T, inputs.device)]
        return self._state_from_dense(out, tuple((c.clone(), h.clone()) for c, h in final))

    def _temperature(self, temperature):
        if self.num_tracks > 1:                        # a MultiNADE: one NADE, one temperature per track
            return sampling_temperature(temperature, self.num_tracks)
        # one NADE: a sequence of n values (n divides the visibles) gives visible i the temperature [i % n] -- the tracks of joint mode,
        # whose NADE orders its visibles p M + m (the mode has checked n == M)
        n = None
        if hasattr(temperature, "__len__") and len(temperature) > 0 and self.num_dims % len(temperature) == 0:
            n = len(temperature)
        return sampling_temperature(temperature, n, what="temperature (one NADE: a sequence whose length divides its visibles)")

    def _max_notes(self, max_notes):
        if self.num_tracks > 1:                        # a MultiNADE: track m's NADE emits at most max_notes[m] ones
            return sampling_max_notes(max_notes, self.num_tracks, self.num_dims)
        # one NADE: an integer caps the whole vector; a sequence of n entries (n divides the visibles) caps the visibles i with i % n == m at
        # entry m -- the tracks of joint mode, as _temperature's sequence (equal entries are NOT the integer here: they count apart)
        if max_notes is None or isinstance(max_notes, numbers.Real):
            return sampling_max_notes(max_notes, None, self.num_dims)
        n = None
        if hasattr(max_notes, "__len__") and len(max_notes) > 0 and self.num_dims % len(max_notes) == 0:
            n = len(max_notes)
        return sampling_max_notes(max_notes, n, None if n is None else self.num_dims // n, collapse=n == 1,
                                  what="max_notes (one NADE: a sequence whose length divides its visibles)")

    def _particles(self, particles, temperature, max_notes, given):
        return sampling_particles(particles, temperature, max_notes, given)

    def _scan_in_one_call(self, x, num_steps, given=None, temperature=1.0, max_notes=None, redraws=0, particles=0, lengths=None):
        """rnn_estimator.py:271-298 through ONE C-ABI call (mnn_generate_scan: intro pass + num_steps x {NADE sample, LSTM step, Dense} enqueued
        by the library's own host loop) when the inputs are the byte piano-roll itself; the same kernels and bits as the step-by-step path.
        given: the scan's codes u8 [B, num_steps, num_output] (generate)."""
        if x.dtype != torch.uint8 or x.shape[-1] != self.num_tracks * self.num_dims or int(num_steps) < 1:
            return None
        sir = {}
        if particles and given is not None:
            ess, pick = particle_cells(self, num_steps, self.num_tracks, x.shape[0], x.device)
            sir = dict(particles=particles, ess=ess, pick=pick)
        return ops.generate_scan(x.contiguous(), num_steps, temperature=temperature, seed=self.seed, row0=self.row0, given=given, max_notes=max_notes,
                                 **sir, redraws=redraws, redraw_stats=redraw_cell(self, x.device) if redraws else None,
                                 **({} if lengths is None else dict(lengths=lengths)),
                                 state0=self._state0(x.shape[0], torch.float32), **self._scan_layers())      # (learn_zero_state: tiled on the device here, an input array of the scan)

    def _state_of(self, out, rnn_state):
        return self._state_from_dense(out, rnn_state)

    def _scan_layers(self):
        """The weights of the one-call scan, as keyword arguments of ops.generate_scan / generate_scan_chunk."""
        pre = self._rnn.prefix
        return dict(layers=[(self.store[f"{pre}/cell_{l}/kernel"], self.store[f"{pre}/cell_{l}/bias"]) for l in range(len(self._rnn.num_units))],
                    dense_W=self.store["dense/kernel"], dense_bias=self._det_fc_bias(), tracks=self.num_tracks, D=self.num_dims, Hn=self.num_hidden[-1],
                    w_enc=self.store["nade/w_enc"], w_dec=self.store["nade/w_dec"], by_visible=self.num_tracks == 1)

    def _det_fc_bias(self):
        if not self.internal_bias:
            return self.store["dense/bias"]
        b = torch.empty(self.n_out, device=self.store.theta.device)          # dense/bias + [b_enc | b_dec] (see _init_estimator)
        ops.axpby(1.0, self.store["dense/bias"], 1.0, self._internal_flat(self.store.theta), b)
        return b

    def _det_dense_job(self, h):
        """(job, out): the Dense layer on h f32 [B, R] in the deterministic arithmetic (ops.dense_det), master weights in place."""
        out = torch.empty((h.shape[0], self.ldo), device=h.device)            # columns [n_out, ldo) are alignment only: no kernel reads them
        return dict(x=h, W=self.store["dense/kernel"], bias=self._det_fc_bias(), out=out[:, :self.n_out]), out

    def _det_state(self, h, rnn_state):
        job, out = self._det_dense_job(h)
        ops.dense_det([job])
        return self._state_from_dense(out, tuple(rnn_state))

    def single_step(self, inputs, initial_state, x2=None):
        """rnn_nade.py:253-277."""
        if self.det_sampling:
            return self._det_single_step(inputs, initial_state, x2)
        if x2 is not None:
            inputs = torch.cat([inputs.float(), x2], 1)
        x = self._step_input(inputs.shape[0], inputs.device)
        ops.convert2d(inputs.contiguous() if inputs.dtype in (torch.uint8, torch.float32, torch.bfloat16, torch.float16) else inputs.float(),
                      x[:, :inputs.shape[1]])
        h, new = self._stack.single_step(x, [(c, hh) for c, hh in initial_state.rnn_state])
        return self._state_from_dense(self._dense(h.contiguous()), tuple(new))       # views of buffers this step allocated: no copies

    def log_prob(self, inputs, targets_flat, lengths=None):
        """rnn_nade.py:279-302 (API-order outputs)."""
        state = self._get_state(inputs, lengths=lengths)
        return self._nade.log_prob(targets_flat, state.b_enc, state.b_dec)

    def sample_single(self, inputs, state, *, given=None, temperature=1.0, at=None):
        """rnn_nade.py:304-318 / rnn_multinade.py:295-317: returns (sample u8 [B,num_output], nll).  given (optional): codes u8
        [B, num_output] (ops.nade_sample): clamped visibles are emitted as given, nll is that of the emitted vector.
        temperature: a float, None (threshold draws), or a sequence -- per track of a MultiNADE, by visible index modulo its length for
        the one NADE; the returned nll stays the model's own.  at (common.DrawAt; None: this generator's seed and row0, step 0): where
        the draws stand.  The biases are the state's Dense block (state.dense: every state a step or an intro pass returns has one)."""
        return self.sample_single_capped(inputs, state, given=given, temperature=temperature, at=at)

    def sample_single_capped(self, inputs, state, *, given=None, temperature=1.0, at=None, max_notes=None):
        """sample_single under a polyphony cap: max_notes is None (sample_single itself, which calls this), an integer, or a sequence read
        like the temperature's -- at most that many ones per track of this step (ops.nade_sample).  The signature every estimator's
        sample_single shares stays as it is; only the NADE estimators have this one."""
        return self.sample_single_redrawn(inputs, state, given=given, temperature=temperature, at=at, max_notes=max_notes)

    def sample_single_redrawn(self, inputs, state, *, given=None, temperature=1.0, at=None, max_notes=None, redraws=0, redraw_stats=None):
        """sample_single_capped with the cap by rejection: redraws (0: sample_single_capped itself, which calls this) tries before the
        truncating step (ops.nade_sample); redraw_stats: None, or an int32[2] on the device that gains this step's (redrawn, fallback)
        scans -- the caller's own cell: the generator's is written by generate and by sessions only."""
        redraws = sampling_redraws(redraws, max_notes, temperature)
        M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
        at = DrawAt(self.seed, self.row0, 0) if at is None else at
        out = state.dense
        Bn = out.shape[0]
        smp = torch.empty((Bn, M * D), device=out.device, dtype=torch.uint8)
        nll = torch.empty((M, Bn), device=out.device)
        ops.nade_sample(out, self.store["nade/w_enc"], self.store["nade/w_dec"], M, D, Hn, temperature, at.seed, at.row0, at.step, smp,
                        track_minor=(M > 1), nll=nll, given=None if given is None else given.contiguous(), by_visible=M == 1, sub_base=at.base,
                        max_notes=max_notes, redraws=redraws, redraw_stats=redraw_stats)
        return smp, (nll[0] if M == 1 else [nll[m] for m in range(M)])


    def sample_single_resampled(self, inputs, state, *, given=None, temperature=1.0, at=None, particles=None, ess=None, pick=None):
        """sample_single by importance resampling (ops.nade_sample_sir): particles = C clamped scans of this step, one emitted.  None, 0, 1
        or no given: sample_single itself.  ess f32 / pick int32 [num_tracks, B] (optional, on the device) receive the step's statistics;
        the returned nll is the model's own of the emitted vector."""
        particles = sampling_particles(particles, temperature, None, given)
        if not particles:
            return self.sample_single(inputs, state, given=given, temperature=temperature, at=at)
        M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
        at = DrawAt(self.seed, self.row0, 0) if at is None else at
        out = state.dense
        Bn = out.shape[0]
        smp = torch.empty((Bn, M * D), device=out.device, dtype=torch.uint8)
        nll = torch.empty((M, Bn), device=out.device)
        ops.nade_sample_sir(out, self.store["nade/w_enc"], self.store["nade/w_dec"], M, D, Hn, temperature, at.seed, at.row0, at.step, smp,
                            given.contiguous(), particles, track_minor=(M > 1), nll=nll, by_visible=M == 1, sub_base=at.base, ess=ess, pick=pick)
        return smp, (nll[0] if M == 1 else [nll[m] for m in range(M)])


class RnnMultiNADE(RnnNade):
    """models/generators/rnn_multinade.py: one LSTM, one Dense, ``len(tracks)`` NADEs."""

    def __init__(self, num_dims, num_hidden, num_hidden_rnn, tracks, keep_prob=1.0, internal_bias=False, name="rnn-multinade", **kw):
        self._tracks = list(tracks)
        super().__init__(num_dims, num_hidden, num_hidden_rnn, keep_prob, internal_bias, name, track_name="all", **kw)


# ------------------------------------------------------------------------------------------------
class RnnRBM(RnnEstimator):
    """models/generators/rnn_rbm.py: LSTM -> (Wuh, Wuv) -> RBM with CD-k Gibbs sampling.

    Reference defects R1-R4 are resolved as recorded there: k = rbm.k in
    sample_single, lengths forwarded to _get_state, per-row free energy, and
    ``bias_mode='conditional'`` (Boulanger-Lewandowski) as the trained loss; 'internal'
    reproduces the as-written metric.

    The step is written over the track list ``self._rbms`` (M = len; here M = 1, as RnnNade is over ``self._nades``): the Dense output of a
    row is [bh_0 .. bh_{M-1} | bv_0 .. bv_{M-1}], the chains' inputs, targets and outputs carry a leading track axis [M, N, .].
    RnnMultiRBM is the same code with M tracks; what it overrides is the launch form (_step_chains, _free_energies: this class calls the
    single-job entries, never a one-job grouped launch), the presentation of per-track values (_present: tensors here, lists there), the
    variable prefix, and the sampling step."""

    def __init__(self, num_dims, num_hidden, num_hidden_rnn, keep_prob=1.0, internal_bias=True, k=10, name="rnn-rbm", track_name="all",
                 bias_mode="conditional", **kw):
        self._k = k
        self.bias_mode = bias_mode
        self._tracks = getattr(self, "_tracks", ["all"])
        super().__init__(num_dims, num_hidden, num_hidden_rnn, keep_prob, internal_bias, name, track_name, **kw)
        self._num_output = self.num_tracks * self.num_dims

    k = property(lambda self: self._k)
    tracks = property(lambda self: self._tracks)
    num_tracks = property(lambda self: len(self._tracks))

    # -- what RnnMultiRBM overrides -------------------------------------------------------------
    def _rbm_prefix(self, m):
        return "rbm"

    def _present(self, per_track):
        """A per-track list as the API returns it: the one track's value itself."""
        return per_track[0]

    def _step_chains(self, v0, bh, bv, rows, p_v, v_s):
        """The CD-k chains of a built step, track m from v0[m] with seed + m.  seed + step, the step read on the device (store.step_dev ==
        store.step here): the same draws as passing seed + store.step, and a captured step (graphed_build_train) draws anew at every replay."""
        ops.rbm_gibbs(v0[0], self._rbm.W, bh[0], bv[0], self._k, self.seed, 0, rows, 0, p_v[0], v_s[0], seed_step=self.store.step_dev)

    def _free_energies(self, v, bh, bv, F, p_h):
        """F[m] = F_m(v[m]) of every track's rows; p_h (optional): sigmoid(z) of the same pass."""
        ops.rbm_free_energy(v[0], self._rbm.W, bh[0], bv[0], F[0], p_h=None if p_h is None else p_h[0])

    # -- construction ---------------------------------------------------------------------------
    def _init_estimator(self):
        self._rbms = [RBM(self.num_dims, self.num_hidden[-1], k=self._k, name=self._rbm_prefix(m)) for m in range(self.num_tracks)]
        self._rbm = self._rbms[0]

    def _declare(self, num_inputs):
        """Variable order rbm(s) [W, bv, bh], rnn, [Wuh, Wuv] (rnn_rbm.py:135-138); the columns of Wuh / Wuv are track-major."""
        M, D, Hn, R = self.num_tracks, self.num_dims, self.num_hidden[-1], self.num_hidden_rnn[-1]
        for m, r in enumerate(self._rbms):
            r.declare(self.store, self._gen, prefix=self._rbm_prefix(m))
        self._rnn.declare(self.store, num_inputs, self._gen)
        self.store.declare("Wuh", (R, M * Hn), glorot_uniform(self._gen, R, M * Hn))
        self.store.declare("Wuv", (R, M * D), glorot_uniform(self._gen, R, M * D))
        self.n_out = M * (Hn + D)
        self.ldo = ops.round_up(self.n_out, 64)

    def _internal_biases(self):
        """[bh_0 .. bh_{M-1}] and [bv_0 .. bv_{M-1}] as two flat vectors, in the Dense output's column order (one track: views of its own)."""
        if len(self._rbms) == 1:
            return self._rbm.bh.view(-1), self._rbm.bv.view(-1)
        return torch.cat([r.bh.view(-1) for r in self._rbms]), torch.cat([r.bv.view(-1) for r in self._rbms])

    def _pack_estimator(self):
        dev = self.store.theta.device
        R = self.num_hidden_rnn[-1]
        wu = torch.cat([self.store["Wuh"], self.store["Wuv"]], 1).contiguous()          # [R, M Hn + M D]
        self._wu_t = torch.empty((self.n_out, R), device=dev, dtype=self.dtype)
        ops.transpose(wu, self._wu_t)
        self._wu_p = torch.zeros((R, self.ldo), device=dev, dtype=self.dtype)
        ops.convert2d(wu, self._wu_p[:, :self.n_out])
        self._bias_cat = torch.cat(self._internal_biases()).contiguous() if self.internal_bias else torch.zeros(self.n_out, device=dev)

    def _biases(self, h):
        """rnn_rbm.py:240-259: bh_t = rbm.bh + o.Wuh ; bv_t = rbm.bv + o.Wuv as ONE GEMM."""
        out = torch.empty((h.shape[0], self.ldo), device=h.device)
        if self.ldo != self.n_out:
            out[:, self.n_out:].zero_()
        ops.gemm_tn(h, self._wu_t, out[:, :self.n_out], bias=self._bias_cat)
        return out

    def _split(self, out):
        """The per-track bias blocks of a Dense output [N, ld]: views, one leading dimension."""
        M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
        return ([out[:, m * Hn:(m + 1) * Hn] for m in range(M)], [out[:, M * Hn + m * D:M * Hn + (m + 1) * D] for m in range(M)])

    def _planes(self, x, B, T):
        """[B, T, D * M] composer layout (feature d * M + m) -> u8 [M, T * B, D]: every track's rows as a contiguous time-major plane."""
        M, D = self.num_tracks, self.num_dims
        return x[:, :, :D * M].to(torch.uint8).reshape(B, T, D, M).permute(3, 1, 0, 2).contiguous().view(M, T * B, D)

    # -- forward --------------------------------------------------------------------------------
    def build(self, x=None, y=None, lengths=None, is_train=None, mode="eval"):
        """rnn_rbm.py:71-143."""
        return drive(self._build_co(x, y, lengths, is_train, mode))

    def _build_co(self, x=None, y=None, lengths=None, is_train=None, mode="eval"):
        """`build` as a generator function (drive / drive_group: the LSTM recurrences are yielded to the driver).  Track m runs a CD-k chain
        from its slice of the inputs (rnn_rbm.py:112), cost_m = F_m(target_m) - F_m(v_s,m); the loss, `free_energy` and `log_likelihood` are
        the MEAN over the tracks of the row-weighted values (rnn_multinade.py:199-203)."""
        Generator.build(self, x, y, lengths, is_train, mode)
        self._materialize(x.shape[-1] if x is not None else self._num_inputs)
        self._rnn.build_cell(is_train)
        if mode in ("train", "eval"):
            B, T, _ = x.shape
            M, D, Hn = self.num_tracks, self.num_dims, self.num_hidden[-1]
            N, dev, train = B * T, x.device, mode == "train"
            self._ensure_packed()
            x_tm = self._to_time_major_inputs(x)
            v0, tgt = self._planes(x, B, T), self._planes(y, B, T)
            rw = self._row_weight(lengths, B, T, dev)
            kp = self._rnn.effective_keep_prob()
            seed = self.seed + self.store.step
            yy, ctx, _ = yield from self._stack.forward_co(x_tm, kp, self.seed, self.row0, save=train, state0=self._state0(B),
                                                           step_dev=self.store.step_dev, state_grad=train)
            out = self._biases(yy.view(N, -1))
            bh_t, bv_t = self._split(out)
            p_v = torch.empty((M, N, D), device=dev)
            v_s = torch.empty((M, N, D), device=dev, dtype=torch.uint8)
            self._step_chains(v0, bh_t, bv_t, self._row_ids(B, T, dev).int(), p_v, v_s)
            if self.bias_mode == "conditional":
                bh_u, bv_u = bh_t, bv_t
            else:
                bh_u, bv_u = [r.bh for r in self._rbms], [r.bv for r in self._rbms]
            Fv = torch.empty((M, N), device=dev); Fs = torch.empty((M, N), device=dev)
            # train mode: the same pass leaves sigmoid(z) of both chains' ends, the hidden activations of the free-energy gradient (backward)
            sv = torch.empty((M, N, Hn), device=dev) if train else None
            ss = torch.empty((M, N, Hn), device=dev) if train else None
            self._free_energies(tgt, bh_u, bv_u, Fv, sv)
            self._free_energies(v_s, bh_u, bv_u, Fs, ss)
            cost = Fv - Fs
            rwm = rw if M == 1 else (rw / M).repeat(M)                                   # mean over the tracks of the row-weighted sums
            loss = torch.zeros(1, device=dev)
            ops.weighted_sum(cost.view(-1), rwm, loss)
            self._ctx = dict(y=yy, lstm=ctx, out=out, tgt=tgt, v_s=v_s, rw=rw, kp=kp, seed=seed, B=B, T=T, n_valid=self._n_valid,
                             ls_dev=self._ls_dev if self._n_valid is None else None, sv=sv, ss=ss)
            self._cost_tm, self._F_tm, self._pv_tm, self._vs_tm, self._loss = cost, Fv, p_v, v_s, loss
            self._lengths, self._flat_idx = lengths, None
            self._recon_tm = torch.empty((M, N), device=dev)
            ops.log_loss_rows(tgt.view(M * N, D), p_v.view(M * N, D), self._recon_tm.view(-1))               # rbm.py:124-129
            fe, ll = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
            ops.weighted_sum(Fv.view(-1), rwm, fe)
            ops.weighted_sum(self._recon_tm.view(-1), rwm, ll)
            self._metrics = {"batch/loss": loss, "free_energy": fe, "log_likelihood": ll}
            self._metrics_upd = []
        self._is_built = True

    def _per_track(self, t, cast=None):
        idx = self._idx()
        return self._present([t[m][idx] if cast is None else t[m][idx].to(cast) for m in range(self.num_tracks)])

    cond_probs = property(lambda self: self._per_track(self._pv_tm))
    _outputs = property(lambda self: self._per_track(self._vs_tm, torch.float32))
    free_energy = property(lambda self: self._per_track(self._F_tm))
    cost = property(lambda self: self._per_track(self._cost_tm))
    reconstruction_cost = property(lambda self: self._per_track(self._recon_tm))

    def build_metrics(self, targets, predictions, cond_probs=None, log_probs=None):
        return self._rbm.build_metrics(targets, predictions, cond_probs, log_probs)

    def _nll_rows_built(self, num_chains=64, num_betas=1000, betas=None, seed=None, method="ais", given=None, partial="refuse"):
        """AIS NLL of the last build's valid rows (API order): the SUM over the tracks (independent given the history) of
        -log p(v_t | v_<t) = F_t(v_t) + log Z_t with the row's CONDITIONAL biases bh_t, bv_t (the distribution sample() draws from, whatever
        bias_mode trained) and log Z_t estimated by RBM.log_partition -- the chains keyed by the global row ids of build (_row_ids), track m
        with seed + m, seed default self.seed.  Biased low: see NllEstimate.  method "raise": log Z_t by RBM.log_partition_reverse from the
        row's target v_t (biased the other way); "both": the NllBracket, each side summed over the tracks.
        given (optional): (codes u8 [B, T, D * M] in the inputs' layout -- the targets at the given cells, 255 at the free ones:
        common.given_codes --, whole, some: per track, whether every / any cell is given: common.given_tracks) -> the conditional rows
        -log p(v_t,free | v_t,given, v_<t) = F_t(v_t) + log Z_t,c, the stationary distribution of the clamped chain generate(given=) runs at
        that step.  A wholly given track adds exactly 0 and runs no chain; a track with no given cell is estimated as without `given`.
        partial: estimate_nll's, accepted and ignored -- the clamped estimators take any mask."""
        sides = nll_sides(method)
        nll_partial(partial)
        cx = self._ctx
        B, T = cx["B"], cx["T"]
        bh_t, bv_t = self._split(cx["out"])
        dev = cx["out"].device
        idx = self._idx()
        n = idx.numel()
        if given is not None and all(given[1]):
            return given_nll_result(method, n, dev)
        if n == 0:
            e = torch.zeros(0, device=dev)
            return nll_result(method, [NllEstimate(e, e, e, e, e) for _ in sides])
        ids = self._row_ids(B, T, dev)[idx].to(torch.int32).contiguous()
        s0 = self.seed if seed is None else seed
        planes = self._planes(given[0], B, T) if given is not None and any(given[2]) else None
        parts = [[] for _ in sides]
        for m, r in enumerate(self._rbms):
            if given is not None and given[1][m]:
                continue
            codes = planes[m][idx].contiguous() if planes is not None and given[2][m] else None
            bh, bv = bh_t[m][idx].contiguous(), bv_t[m][idx].contiguous()
            tgt = cx["tgt"][m][idx].contiguous()
            F = torch.empty(n, device=dev)
            ops.rbm_free_energy(tgt, r.W, bh, bv, F)
            for side, part in zip(sides, parts):
                part.append(rbm_nll_side(side, r, tgt, F, bh, bv, num_chains, num_betas, betas, s0 + m, ids, codes))
        return nll_result(method, [NllEstimate.total(p) for p in parts])             # (one part: total returns the part itself)

    # -- backward -------------------------------------------------------------------------------
    def backward(self):
        return drive(self._backward_co())

    def _grad_seed(self, cx):
        """(row weights, scale, ls) of a built step's gradient rows: rbm_cd_rows weighs row n by rw[n] * scale -- the mode's weight of this
        generator's loss, the 1 / M of the mean over the tracks and the f16 loss scale (static x the dynamic multiplier of ParamStore.ls_dyn)
        -- and _unscale(ls) takes the loss scale out again."""
        M = self.num_tracks
        dyn = self.store.ls_dyn if self.dtype == torch.float16 else None
        gs = self.grad_scale / M if M > 1 else self.grad_scale
        if cx["n_valid"] is None:                    # ragged_on_device: the scale is a device scalar (folded into the row weights); _unscale gets its inverse
            lsd = cx.get("ls_dev")
            if lsd is not None and dyn is not None:
                lsd = lsd * dyn[0:1]
            return (cx["rw"] if lsd is None else cx["rw"] * lsd), gs, (1.0 if lsd is None else 1.0 / lsd)
        ls = self._stack.loss_scale(cx["n_valid"])
        if dyn is not None:
            return cx["rw"] * dyn[0:1], gs * ls, dyn[1:2] * (1.0 / ls)
        return cx["rw"], gs * ls, ls

    def _backward_co(self):
        cx = self._ctx
        M, D, Hn, R = self.num_tracks, self.num_dims, self.num_hidden[-1], self.num_hidden_rnn[-1]
        B, T = cx["B"], cx["T"]
        N, dev = B * T, cx["out"].device
        g = self.store.gviews
        self.store.grad.zero_()
        sv, ss = cx.get("sv"), cx.get("ss")           # sigmoid(z(v)), sigmoid(z(v_s)): left by the forward's free-energy passes
        if sv is None:
            raise RuntimeError("build(..., mode='train') must run before train()")
        rw, scale, ls = self._grad_seed(cx)
        # dF/dbh = -sigmoid(z), dF/dbv = -v, dF/dW = -v^T sigmoid(z); cost = F(v) - F(v_s), v_s constant (rbm.py:229).  Per track one pass writes
        # the rows of its gradient block [Hn | D] and the two scaled hidden blocks of d cost / d W = v_s^T (w ss) - v^T (w sv).  One track: the
        # block is the Dense-shaped d_out's own leading columns, written in place (padding zeroed by the pass); M tracks: a track's two column
        # blocks are not adjacent in d_out, so the rows are staged in d_m and copied into them
        d_out = (torch.empty if M == 1 else torch.zeros)((N, self.ldo), device=dev)
        d_m = d_out if M == 1 else torch.empty((N, Hn + D), device=dev)
        pos = torch.empty((M, N, Hn), device=dev); neg = torch.empty((M, N, Hn), device=dev)
        # d cost / d W = v_s^T pos + v^T neg, [D, N] . [N, Hn] with K = N rows.  16-bit modes: the operands in the compute type (v, v_s are 0 / 1:
        # exact; pos / neg are loss-scaled products of a weight and a sigmoid) on the LDS-DMA GEMM -- as f32 products on v_mfma_f32_32x32x2_f32
        # (1/16 of the 16-bit rate) the two GEMMs were 0.53 ms per track of the 3.6 ms jamming step (round 4 profile); fp32 mode keeps f32.
        h16 = self._stack.h16
        Np = ops.round_up(N, 64 if h16 else 4)
        def tr(xm, rows):                                # (the zero fill is for the padding columns only: four fills per track and step at C3 otherwise)
            o = (torch.zeros if Np != N else torch.empty)((rows, Np), device=dev, dtype=self.dtype if h16 else torch.float32)
            return ops.transpose(xm, o)
        # two output tiles and K = N rows -- without split-K two workgroups walk the whole batch (6.7 ms of a 19.6 ms step at N = 32 768);
        # slices of >= 256 rows, up to one workgroup per CU
        sk = int(max(1, min(256 // (-(-D // 128) * -(-Hn // 128)), Np // 256)))
        dbh, dbv = self._split(d_out)
        for m, r in enumerate(self._rbms):
            ops.rbm_cd_rows(cx["tgt"][m], cx["v_s"][m], sv[m], ss[m], rw, scale, d_m, pos[m], neg[m])
            if M > 1:
                dbh[m].copy_(d_m[:, :Hn]); dbv[m].copy_(d_m[:, Hn:])
            gW = g[f"{r.prefix}/W"]
            ops.gemm_tn(tr(cx["v_s"][m], D), tr(pos[m], Hn), gW, accumulate=True, split_k=sk)
            ops.gemm_tn(tr(cx["tgt"][m], D), tr(neg[m], Hn), gW, accumulate=True, split_k=sk)
        def bias_grads(col):                             # col(lo, hi, gv): the column sums [lo, hi) of d_out, accumulated into gv by the callee
            for m, r in enumerate(self._rbms):
                col(m * Hn, (m + 1) * Hn, g[f"{r.prefix}/bh"].view(-1))
                col(M * Hn + m * D, M * Hn + (m + 1) * D, g[f"{r.prefix}/bv"].view(-1))
        if self.bias_mode != "conditional":
            bias_grads(lambda lo, hi, gv: ops.bias_grad(d_out[:, lo:hi], gv, accumulate=True))
            self._dx = None
            self._unscale(ls)
            return                                   # as written: no gradient reaches the LSTM / Wuh / Wuv (R3)
        Np8 = ops.round_up(N, 64)
        zalloc = torch.zeros if Np8 != N else torch.empty
        yT = cx["lstm"][-1].get("yT") if cx["lstm"] else None      # emitted by the persistent / row-parallel recurrences
        if yT is None:
            yT = zalloc((R, Np8), device=dev, dtype=self.dtype)
            ops.transpose(cx["y"].view(N, R), yT)
        doT = zalloc((self.n_out, Np8), device=dev, dtype=self.dtype)
        if self.dtype == torch.float32:
            if self.internal_bias:
                bias_grads(lambda lo, hi, gv: ops.bias_grad(d_out[:, lo:hi], gv, accumulate=True))
            ops.transpose(d_out[:, :self.n_out], doT)
            do_c = d_out
        else:
            # one pass over d_out: 16-bit copy (the input-gradient operand), 16-bit transpose (the Wuh / Wuv gradient operand) and the column
            # sums, which ARE the gradients of rbm.bh | rbm.bv (internal_bias: rnn_rbm.py:240-259 adds them to the Dense outputs) -- instead of
            # two bias_grad passes, a transpose and a convert2d
            do_c = torch.empty((N, self.ldo), device=dev, dtype=self.dtype)
            colsum = torch.zeros(self.n_out, device=dev)
            ops.grad_rows_fanout(d_out, self.n_out, do_c, doT, colsum)
            if self.internal_bias:
                bias_grads(lambda lo, hi, gv: ops.axpby(1.0, colsum[lo:hi], 1.0, gv, gv))
        # Wuh [R, M Hn] and Wuv [R, M D] are separate variables: one accumulating product per variable, over all tracks' blocks
        ops.gemm_tn(yT, doT[:M * Hn], g["Wuh"], accumulate=True, split_k=LstmStack._split_k(R, M * Hn, Np8))
        ops.gemm_tn(yT, doT[M * Hn:self.n_out], g["Wuv"], accumulate=True, split_k=LstmStack._split_k(R, M * D, Np8))
        dy = torch.empty((N, R), device=dev)
        ops.gemm_tn(do_c, self._wu_p, dy)
        self._dx = yield from self._lstm_backward_co(dy, cx)
        self._unscale(ls)

    # -- states and sampling --------------------------------------------------------------------
    def zero_state(self, batch_size):
        self._materialize(self._num_inputs)
        dev = self.store.theta.device
        z = lambda n: torch.zeros((batch_size, n), device=dev)
        return RnnEstimatorStateTuple(self._present([z(self.num_hidden[-1]) for _ in self._rbms]), self._present([z(self.num_dims) for _ in self._rbms]),
                                      self._get_rnn_zero_state(batch_size))

    def _get_state(self, inputs, lengths=None, initial_state=None, last_outputs=False):
        """rnn_rbm.py:184-238 (dynamic_rnn; identical to the decode loop on valid rows)."""
        self._materialize(inputs.shape[-1])
        self._ensure_packed()
        if inputs.dim() == 2:
            inputs = inputs[:, None, :]
        B, T, _ = inputs.shape
        x_tm = self._to_time_major_inputs(inputs)
        st0 = [(c, h) for c, h in initial_state.rnn_state] if initial_state is not None else self._state0(B)
        y, _, final = self._stack.forward(x_tm, self._rnn.effective_keep_prob(), self.seed, self.row0, save=False, state0=st0)
        out = self._biases(y[-1].contiguous()) if last_outputs else self._biases(y.view(T * B, -1))[flat_index(lengths, B, T, inputs.device)]
        return self._state_from_out(out, tuple((c.clone(), h.clone()) for c, h in final))

    def _state_from_out(self, out, rnn_state):
        """The estimator state of a Dense output [B, ld]: the tracks' bias blocks bh_t | bv_t (views)."""
        be, bd = self._split(out)
        st = RnnEstimatorStateTuple(self._present(be), self._present(bd), rnn_state)
        st.dense = out
        return st

    def _state_of(self, out, rnn_state):
        return self._state_from_out(out, rnn_state)

    subs_per_step = property(lambda self: max(self._k, 1))

    _det_bias = None                       # inside RnnMultiRBM._sampling_scope: True, then the internal bias vectors the scan's first Dense formed

    def _det_state(self, h, rnn_state):
        """rnn_rbm.py:240-259 in the deterministic arithmetic: [bh_0 ..] = [rbm_m.bh] + h . Wuh, [bv_0 ..] = [rbm_m.bv] + h . Wuv (two jobs,
        one launch)."""
        M, Hn = self.num_tracks, self.num_hidden[-1]
        out = torch.empty((h.shape[0], self.ldo), device=h.device)
        bh = bv = None
        if self.internal_bias:
            ib = self._det_bias
            if ib is None or ib is True:
                cat = self._internal_biases()
                if ib is True:
                    self._det_bias = cat
                ib = cat
            bh, bv = ib
        ops.dense_det([dict(x=h, W=self.store["Wuh"], bias=bh, out=out[:, :M * Hn]),
                       dict(x=h, W=self.store["Wuv"], bias=bv, out=out[:, M * Hn:self.n_out])])
        return self._state_from_out(out, tuple(rnn_state))

    def single_step(self, inputs, initial_state, x2=None):
        """rnn_rbm.py:261-281."""
        if self.det_sampling:
            return self._det_single_step(inputs, initial_state, x2)
        if x2 is not None:
            inputs = torch.cat([inputs.float(), x2], 1)
        x = self._step_input(inputs.shape[0], inputs.device)
        ops.convert2d(inputs.contiguous(), x[:, :inputs.shape[1]])
        h, new = self._stack.single_step(x, [(c, hh) for c, hh in initial_state.rnn_state])
        return self._state_from_out(self._biases(h.contiguous()), tuple(new))

    def _temperature(self, temperature):
        return sampling_temperature(temperature, allow_none=False, allow_sequence=False)

    def sample_single(self, inputs, state, *, given=None, temperature=1.0, at=None):
        """rnn_rbm.py:283-297 with k = rbm.k (R1): returns (sample u8, cond_prob).  temperature: the chain of exp(-E / T), cond_prob the
        tempered probability.  given (optional): codes u8 [B, D] (a step slice of
        generate's [B, num_steps, D] is read in place): the clamped Gibbs chain -- clamped visibles are emitted as given, every free one is
        sampled conditioned on all of them (RBM.sample); cond_prob is sigmoid(logit) at every visible.  at (common.DrawAt; None: this
        generator's seed and row0, step 0): where the chain's draws stand -- a step owns max(k, 1) sub-counters."""
        at = DrawAt(self.seed, self.row0, 0) if at is None else at
        p_v, v = self._rbm.sample(inputs[:, :self.num_dims], state.b_enc, state.b_dec, self._k, at.seed, at.row0, None,
                                  at.step * self.subs_per_step, given=given, temperature=temperature, sub_base=at.base)
        return v, p_v

    def pretrain(self, optimizer, lr, run_optimizer=True):
        """rnn_rbm.py:299-322: one CD-k update of every track's RBM on its track of the flattened inputs (`rbm.train`, seed + m; no
        optimiser, no clipping).  Returns the documented 5-tuple (the reference returns `rbm.train`'s 3-tuple although its docstring and
        every caller -- multinn_jamming.py:219-221 -- expect five values)."""
        x = self._inputs
        B, T, _ = x.shape
        M, D = self.num_tracks, self.num_dims
        xt = x.to(torch.uint8)[:, :, :D * M].reshape(B * T, D, M)
        keep = None
        if self._lengths is not None:
            keep = (torch.arange(T, device=x.device)[None, :] < self._lengths.to(x.device)[:, None]).reshape(-1)
        self._materialize(x.shape[-1])
        init_ops, update_ops, grads = [], [], []
        for m, r in enumerate(self._rbms):
            flat = (xt[:, :, m] if keep is None else xt[:, :, m][keep]).contiguous()
            if not run_optimizer:
                # the only caller that passes False (multinn_jamming.py:219-241 without separate losses) discards the CD update ops in favour
                # of its joint gradient step and keeps the init ops: nothing is applied here
                init_ops += r.visible_bias_init_ops(flat)
                continue
            # eager semantics: the CD-k update is APPLIED by this call and update_ops comes back empty, while init_ops are
            # returned unexecuted (the reference runs them once, before the first update: train_encoders.py:150-153) -- run them BEFORE the
            # first pretrain() call, not after it, or the first update's visible-bias delta is overwritten
            io, uo, gr = r.train(flat, lr, seed=self.seed + m + self.store.step, row0=self.row0 * T)
            init_ops += io; update_ops += uo; grads.append(gr)
        if run_optimizer:
            self._cd_gradients = self._present(grads)
            self._packed_step = -1                      # rbm.bh / rbm.bv feed the packed bias row
        return init_ops, update_ops, self.metrics, self.metrics_upd, self.summaries


# ------------------------------------------------------------------------------------------------
class RnnMultiRBM(RnnRBM):
    """A shared-LSTM multi-track LSTM-RBM: one LSTM, one Dense (Wuh | Wuv), ``len(tracks)`` RBMs -- the structure of rnn_multinade.py with
    the estimator of rnn_rbm.py (the reference stops at multinn_composer.py:44-45; it has no such model).  The step is RnnRBM's, over M tracks.

    Inputs / targets are [B, T, M * D] in composer layout (feature d * M + m).  The Dense output of a step is
    [bh_0 .. bh_{M-1} | bv_0 .. bv_{M-1}] (track-major blocks: RnnNade._build_biases' split order); track m runs a CD-k chain with seed
    ``seed + m`` from its slice of the inputs.  The M chains of a step -- training's and every sampling step's -- are ONE grouped launch
    (ops.rbm_gibbs_multi), the free energies one per chain end (ops.rbm_free_energy_multi); per-track values come back as lists."""

    def __init__(self, num_dims, num_hidden, num_hidden_rnn, tracks, keep_prob=1.0, internal_bias=True, k=10, name="rnn-multirbm",
                 bias_mode="conditional", **kw):
        self._tracks = list(tracks)
        if not 1 <= len(self._tracks) <= ops.RBM_MULTI_MAX_JOBS:
            raise ValueError(f"RnnMultiRBM takes 1..{ops.RBM_MULTI_MAX_JOBS} tracks (one grouped launch), got {len(self._tracks)}")
        super().__init__(num_dims, num_hidden, num_hidden_rnn, keep_prob, internal_bias, k, name, "all", bias_mode, **kw)

    def _rbm_prefix(self, m):
        return f"rbm_{m}"

    def _present(self, per_track):
        return per_track

    def _step_chains(self, v0, bh, bv, rows, p_v, v_s):
        ops.rbm_gibbs_multi([dict(v0=v0[m], W=r.W, bh=bh[m], bv=bv[m], seed=self.seed + m, p_v=p_v[m], v_out=v_s[m]) for m, r in enumerate(self._rbms)],
                            self._k, 0, rows, 0, seed_step=self.store.step_dev)

    def _free_energies(self, v, bh, bv, F, p_h):
        ops.rbm_free_energy_multi([dict(v=v[m], W=r.W, bh=bh[m], bv=bv[m], F=F[m], p_h=None if p_h is None else p_h[m]) for m, r in enumerate(self._rbms)])

    def _temperature(self, temperature):
        return sampling_temperature(temperature, self.num_tracks, allow_none=False)

    @contextlib.contextmanager
    def _sampling_scope(self):
        self._det_bias = True              # the first Dense of this scan forms the internal bias vectors, the later ones reuse them
        try:
            yield
        finally:
            self._det_bias = None

    def sample_single(self, inputs, state, *, given=None, temperature=1.0, at=None):
        """The M chains of a sampling step in ONE grouped launch (temperature: one for all, or track m's chain at temperature[m]): the previous row is read, and the new one written, in composer layout in
        place (element stride M), track m with seed + m.  Returns (sample u8 [B, M * D], cond_prob f32 [B, M * D]).  given (optional):
        codes u8 [B, M * D] in the same layout (a step slice of generate's block is read in place): every track runs the clamped chain.
        at: RnnRBM.sample_single's."""
        M, D = self.num_tracks, self.num_dims
        at = DrawAt(self.seed, self.row0, 0) if at is None else at
        v0 = inputs[:, :M * D]
        v0 = (v0 if v0.dtype == torch.uint8 else v0.to(torch.uint8)).contiguous()
        Bn = v0.shape[0]
        smp = torch.empty((Bn, M * D), device=v0.device, dtype=torch.uint8)
        p_v = torch.empty((Bn, M * D), device=v0.device)
        jobs = [dict(v0=v0[:, m::M], W=r.W, bh=state.b_enc[m], bv=state.b_dec[m], seed=at.seed + m, p_v=p_v[:, m::M], v_out=smp[:, m::M],
                     given=None if given is None else given[:, m::M]) for m, r in enumerate(self._rbms)]
        ops.rbm_gibbs_multi(jobs, self._k, at.row0, None, at.step * self.subs_per_step, temperature=temperature, sub_base=at.base)
        return smp, p_v
