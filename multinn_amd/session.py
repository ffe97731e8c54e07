"""Generation sessions: continue a sampled piece in chunks, bit for bit.

``generate(x, num_steps)`` runs the intro pass and the whole scan in one call and keeps nothing.  A session keeps what the scan carries from
step to step -- the LSTM state, the last Dense output, the last emitted row (an RBM chain's start) and the number of generated steps -- so that

    sess = gen.session(x);  cat([sess.generate(n_i, given=g_i, temperature=T) for i]) == gen.generate(x, sum n_i, given=cat g_i, temperature=T)

in every cell, for every split (with ``sess.max_notes = K`` set first: ``gen.generate(..., max_notes=K)``).  Every draw is keyed (stream, global row, sub-counter, element) with the sub-counter "the generated step"
(times max(k, 1) for a Gibbs chain): a chunk that starts at step s draws at s, s + 1, ...  Eagerly that offset is a host number in the launch
arguments.  A CAPTURED chunk cannot bake it in -- every chunk would need a new capture -- so the sampling kernels read it from a one-word
step cell on the device (mnn_nade_sample_temps_at, mnn_rbm_gibbs_at, mnn_rbm_gibbs_multi_at, mnn_generate_scan_chunk): the session fills
the cell with ``steps`` on the stream, then replays the chunk's graph.  Graphs are cached per session by (num_steps, has given, temperature, max_notes):
the addresses of the session's state arrays are baked into them.  Each is a linear graph on one stream.

GeneratorSession: one RnnEstimator (RnnNade, RnnMultiNADE, RnnRBM, RnnMultiRBM).  ModeSession: the joint, jamming and composer modes with
Pass encoders.  Captured (common.ScanGraphs.enabled) and eager chunks run the same launches and give the same bits.
"""
import collections

import torch

from . import ops
from ._lib import MnnUnsupported
from .common import DrawAt, ScanGraphs, _warm_up, check_given, graph_capture, last_prompt_rows, max_notes_key, new_particle_cells, particle_cells, particles_key, prompt_lengths, prompt_lengths_device, redraw_cell, redraws_key, sampling_particles, sampling_redraws, temperature_key

__all__ = ["GeneratorSession", "ModeSession"]

MAX_GRAPHS = 8            # captured chunks a session keeps (least recently used first out)


def _num_steps(steps, num_steps, subs_per_step):
    if isinstance(num_steps, bool) or not isinstance(num_steps, int) or num_steps < 1:
        raise ValueError(f"num_steps must be an integer >= 1, got {num_steps!r}")
    if (int(steps) + num_steps) * max(int(subs_per_step), 1) > 1 << 32:
        raise ValueError(f"{steps} + {num_steps} generated steps of {max(int(subs_per_step), 1)} sub-counter(s) each pass the 2^32 sub-counters of a row")
    return num_steps


def _chunk_arguments(gen, batch, steps, num_steps, given=None, temperature=1.0):
    """The host checks of GeneratorSession.generate, before any device work -> (num_steps, given, temperature) normalised.  ValueError for
    num_steps < 1, a step count that would pass 2^32 sub-counters ((steps + num_steps) * max(k, 1)), a `given` that is not u8
    [batch, num_steps, num_output], or a bad temperature (the generator's own _temperature)."""
    num_steps = _num_steps(steps, num_steps, gen.subs_per_step)
    if given is not None:
        check_given(given, batch, num_steps, gen._num_output)
    return num_steps, given, gen._temperature(temperature)


class GeneratorSession:
    """gen.session(x): the intro pass on x [B, Ti, Din] (from the learned state with learn_zero_state), then generate() chunk by chunk.
    gen.ragged_session(x, lengths) = GeneratorSession(gen, x, lengths): generate's prompt lengths -- the intro pass stops every row at its own length and the first chain starts from
    the row's own last prompt row; the chunks are those of any session.

    State (static device arrays, their addresses baked into the session's captured chunks): per LSTM layer (c, h); where the chunk is the
    generator's step loop also the last Dense output block and the last emitted row; the step cell.  A byte piano-roll into an LSTM-(Multi)NADE
    runs each chunk as ONE library call (mnn_generate_scan_chunk, which forms the first Dense of a chunk from h of the last layer again: the
    same product, the same bits); every other case steps through sample_single / single_step like generate.
    seed and row0 are the generator's when the session is opened; every chunk hands them, the step and the step cell to the generator's
    draws as a common.DrawAt, and nothing on the generator is set or restored: changing gen.seed / gen.row0 later moves generate, not the
    session.  Sessions and generate calls on one generator interleave freely.  What they still share is the generator's per-scan state --
    RnnMultiRBM._det_bias inside _sampling_scope, the packed weight copies, the step staging buffer -- so two scans of ONE generator must
    not run from two threads at once."""

    def __init__(self, gen, x, lengths=None):
        from .generators import refuse_host_model
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x must be a tensor [B, Ti, Din] with at least one intro step, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        lengths = prompt_lengths(lengths, x.shape[0], x.shape[1])
        if lengths is not None:
            gen._refuse_prompt_lengths("ragged_session")
        refuse_host_model(gen.store.device, "a generation session")
        refuse_host_model(x.device, "a generation session")
        self._gen, self.seed, self.row0 = gen, gen.seed, gen.row0
        self._max_notes = None
        self._redraws = 0
        self._particles = 0
        self.steps = 0
        self.batch = int(x.shape[0])
        self._graphs = collections.OrderedDict()
        gen._materialize(x.shape[-1])
        gen._rnn.build_cell(False)
        dev = x.device
        self._cell = torch.zeros(1, dtype=torch.int32, device=dev)            # the step cell: `steps` as 32 bits, filled before every replay
        ldev = None if lengths is None else prompt_lengths_device(lengths, dev)
        self._scan = gen.det_sampling and x.dtype == torch.uint8 and gen._scan_layers() is not None and x.shape[-1] == gen.num_tracks * gen.num_dims
        if self._scan:
            B = self.batch
            self._rnn = [(torch.zeros((B, u), device=dev), torch.zeros((B, u), device=dev)) for u in gen._rnn.num_units]
            self._out = self._last = None
            ops.generate_scan_chunk(x.contiguous(), 0, temperature=1.0, seed=self.seed, row0=self.row0, state_in=gen._state0(B, torch.float32),
                                    state_out=self._rnn, **({} if ldev is None else dict(lengths=ldev)), **gen._scan_layers())
            return
        with gen._sampling_scope():
            if ldev is not None:
                state = gen._det_steps(x, None, ldev)
            elif gen.det_sampling:
                state = gen.steps(x)
            else:
                gen._ensure_packed()
                state = gen._get_state(x, lengths=None, last_outputs=True)
        self._rnn = [(c.clone(), h.clone()) for c, h in state.rnn_state]
        self._out = state.dense.clone()
        last = x[:, -1] if ldev is None else last_prompt_rows(x, ldev)                      # the first chain's start (rnn_estimator.py:283: the intro's last row; with prompt lengths every row's own)
        self._last = last[:, :gen._num_output].to(torch.uint8).contiguous().clone()

    # -- state ----------------------------------------------------------------------------------
    def _tensors(self):
        ts = [t for pair in self._rnn for t in pair]
        return ts if self._scan else ts + [self._out, self._last]

    def snapshot(self):
        """(steps, device copies of the state): restore() rewinds to it -- redraw a bar at another temperature or under another `given`."""
        return self.steps, [t.clone() for t in self._tensors()]

    def restore(self, snap):
        steps, tensors = snap
        mine = self._tensors()
        if len(tensors) != len(mine) or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(mine, tensors)):
            raise ValueError("restore: not a snapshot of this session")
        for a, b in zip(mine, tensors):
            a.copy_(b)
        self.steps = int(steps)

    # -- chunks ---------------------------------------------------------------------------------
    def _run(self, n, given, temperature, base, max_notes=None, redraws=0, particles=0):
        """The launches of one chunk of n steps from the static state, which they advance in place.  base: the step cell (a captured chunk:
        the kernels add its word to their counters) or None (eager: the host adds `steps`).  redraws > 0: the chunk first zeroes the
        generator's statistics cell (a fill node of a captured chunk).  particles > 0: the chunk writes the generator's particle statistics
        of a scan of n steps (common.particle_cells)."""
        gen = self._gen
        sir = {}
        if particles and given is not None and self._scan:
            ess, pick = particle_cells(gen, n, gen.num_tracks, self.batch, self._cell.device)
            sir = dict(particles=particles, ess=ess, pick=pick)
        step0 = 0 if base is not None else self.steps
        stats = None
        if redraws:
            stats = redraw_cell(gen, self._cell.device)
            stats.zero_()
        if self._scan:
            return ops.generate_scan_chunk(None, n, temperature=temperature, seed=self.seed, row0=self.row0, state_in=self._rnn, state_out=self._rnn,
                                           given=given, step0=step0, step_base=base, max_notes=max_notes, redraws=redraws, redraw_stats=stats,
                                           **sir, **gen._scan_layers())
        with gen._sampling_scope():
            if not gen.det_sampling:
                gen._ensure_packed()
            out, state, last = gen._scan_steps(gen._state_of(self._out, tuple(self._rnn)), self._last, n,
                                               DrawAt(self.seed, self.row0, step0, base), given, temperature, max_notes, redraws,
                                               **(dict(particles=particles) if particles else {}))
            for (c, h), (nc, nh) in zip(self._rnn, state.rnn_state):      # behind the last read of the static arrays
                c.copy_(nc)
                h.copy_(nh)
            self._out.copy_(state.dense)
            self._last.copy_(last)
        return out

    # The polyphony cap of the chunks to come (generate's max_notes): a property of the session, set between chunks -- `sess.max_notes = (1,
    # None, 4)` -- and checked when it is set (the generator's own _max_notes: ValueError, or MnnUnsupported on an RBM generator, before
    # any device work).  None, the default, is the session without it: the same launches, keys and captured chunks.
    @property
    def max_notes(self):
        return self._max_notes

    @max_notes.setter
    def max_notes(self, value):
        self._max_notes = self._gen._max_notes(value)

    # The redraws of the chunks to come (generate's redraws), beside max_notes: set between chunks, checked when set; 0, the default, or no
    # cap: the session without them.  Against the chunk's temperature they are checked per chunk (threshold decoding cannot be redrawn).
    @property
    def redraws(self):
        return self._redraws

    @redraws.setter
    def redraws(self, value):
        self._redraws = sampling_redraws(value, 0, 1.0)

    def redraw_counts(self):
        """The generator's redraw_counts(): (redrawn, fallback) of the last chunk (or generate call) that ran on it."""
        return self._gen.redraw_counts()

    # The particles of the chunks to come (generate's particles): set between chunks, checked when set (common.sampling_particles); None, 0
    # and 1 are the session without them.  Against the chunk's temperature and the session's max_notes they are checked per chunk; a chunk
    # without `given`, and an RBM generator, run without them.
    @property
    def particles(self):
        return self._particles

    @particles.setter
    def particles(self, value):
        self._particles = sampling_particles(value)

    def particle_ess(self):
        """The generator's particle_ess() of the last chunk: f32 [B, num_steps, tracks], or None where it ran without particles."""
        return self._gen.particle_ess()

    def particle_picks(self):
        return self._gen.particle_picks()

    def generate(self, num_steps, given=None, temperature=1.0):
        """The next num_steps steps -> u8 [B, num_steps, num_output].  given: the chunk's codes u8 [B, num_steps, num_output] as generate's
        (None: every cell free); temperature: as generate's, and free to change from chunk to chunk.  The chunk runs under the session's
        max_notes and redraws."""
        n, given, temperature = _chunk_arguments(self._gen, self.batch, self.steps, num_steps, given, temperature)
        max_notes = self._max_notes
        redraws = sampling_redraws(self._redraws, max_notes, temperature)
        gen = self._gen
        particles = gen._particles(self._particles, temperature, max_notes, given)
        gen._redraw_live = redraws > 0
        fresh = (lambda: new_particle_cells(n, gen.num_tracks, self.batch, self._cell.device)) if particles else (lambda: None)
        gen._particle_live = None
        if given is not None:
            given = given.to(self._cell.device).contiguous()
        if not ScanGraphs.enabled(self._cell):
            gen._particle_live = fresh()
            out = self._run(n, given, temperature, None, max_notes, redraws, particles)
            self.steps += n
            return out
        key = (n, given is not None) + temperature_key(temperature) + max_notes_key(max_notes) + redraws_key(redraws) + particles_key(particles)
        ent = self._graphs.get(key)
        if ent is None:
            static_g = None if given is None else given.clone()
            cells = gen._particle_live = fresh()     # the statistics arrays of this graph: created before the capture, kept with its entry
            snap = self.snapshot()
            w = min(n, 2)                            # a short eager run: kernel attributes and workspaces exist before the capture
            _warm_up(lambda: self._run(w, None if static_g is None else static_g[:, :w].contiguous(), temperature, self._cell, max_notes, redraws, particles))
            self.restore(snap)
            g = torch.cuda.CUDAGraph()
            gen._packed_step = -1                    # pack inside the graph: a replay always sees the current weights
            with graph_capture(g, capture_error_mode="thread_local"):
                out = self._run(n, static_g, temperature, self._cell, max_notes, redraws, particles)
            gen._packed_step = -1                    # the packed copies now live in the graph's pool
            ent = self._graphs[key] = (g, static_g, out, cells)
            while len(self._graphs) > MAX_GRAPHS:
                self._graphs.popitem(last=False)
        else:
            self._graphs.move_to_end(key)
        g, static_g, out, gen._particle_live = ent
        if static_g is not None:
            static_g.copy_(given)
        self._cell.fill_(self.steps - (1 << 32) if self.steps >= 1 << 31 else self.steps)      # the word, as int32
        g.replay()
        self.steps += n
        return out.clone()


class ModeSession:
    """model.session() of a built joint, jamming or composer model with Pass encoders (generate's precondition): one GeneratorSession per
    generator on the model's encoded intro.  generate(num_steps, given, given_mask, temperature) -> u8 [B, num_steps, P, M]; the chunk's
    arguments go through the mode's own _temperature / _given / _refuse_given.  Jamming: a track that a chunk gives as a whole still runs
    through its generator's clamped scan for that chunk (the output equals the given notes), so its state and counters advance and a later
    chunk can free it."""

    def __init__(self, model, intro_lengths=None):
        from .generators import refuse_host_model
        from .modes import MultINNCore
        mode = model._mode
        if mode not in ("joint", "jamming", "composer"):
            raise MnnUnsupported(f"generation sessions exist for the joint, jamming and composer modes: the sampling scan of the {mode} mode also "
                                 "carries its feedback module's state")
        if model._encoder_type != "Pass":
            raise MnnUnsupported("generation sessions through DBN encoders are not implemented: use Pass encoders")
        refuse_host_model(model.device, "a generation session")
        lengths = model._intro_lengths(intro_lengths, "ragged_session")
        self._model = model
        self.steps = 0
        self._max_notes = None
        self._redraws = 0
        self._particles = 0
        if model._x_encoded is None:
            MultINNCore._build_all(model, "generate")
        self._subs = [g.session(x) if lengths is None else g.ragged_session(x, lengths) for g, x in zip(model.generators, model._generator_inputs())]

    def snapshot(self):
        return self.steps, [s.snapshot() for s in self._subs]

    def restore(self, snap):
        steps, subs = snap
        if len(subs) != len(self._subs):
            raise ValueError("restore: not a snapshot of this session")
        for s, sn in zip(self._subs, subs):
            s.restore(sn)
        self.steps = int(steps)

    # The polyphony cap of the chunks to come, as GeneratorSession's: set between chunks, checked by the mode's own _max_notes when it is
    # set, handed to every generator's session as the mode's generate hands it to the generators (_generator_max_notes).
    @property
    def max_notes(self):
        return self._max_notes

    @max_notes.setter
    def max_notes(self, value):
        m = self._model
        value = m._max_notes(value)
        for s, k in zip(self._subs, m._generator_max_notes(value) if value is not None else [None] * len(self._subs)):
            s.max_notes = k
        self._max_notes = value

    # The redraws of the chunks to come, as GeneratorSession's: checked when set, handed to every generator's session (one without a cap
    # ignores them).
    @property
    def redraws(self):
        return self._redraws

    @redraws.setter
    def redraws(self, value):
        value = sampling_redraws(value, 0, 1.0)
        for s in self._subs:
            s.redraws = value
        self._redraws = value

    # The particles of the chunks to come, as GeneratorSession's: checked when set, handed to every generator's session (an RBM generator
    # ignores them).
    @property
    def particles(self):
        return self._particles

    @particles.setter
    def particles(self, value):
        value = sampling_particles(value)
        for s in self._subs:
            s.particles = value
        self._particles = value

    def particle_ess(self):
        """The mode's particle_ess() of the last chunk: per generator f32 [B, num_steps, its tracks], or None where it ran without particles."""
        return self._model.particle_ess()

    def particle_picks(self):
        return self._model.particle_picks()

    def redraw_counts(self):
        """(redrawn, fallback) of the last chunk, summed over the generators."""
        counts = [s.redraw_counts() for s in self._subs]
        return sum(c[0] for c in counts), sum(c[1] for c in counts)

    def generate(self, num_steps, given=None, given_mask=None, temperature=1.0):
        """The next num_steps steps -> u8 [B, num_steps, P, M].  given u8 [B, num_steps, P, M] / given_mask / temperature: as the mode's
        generate, checked once per chunk, and free to change from chunk to chunk.  The chunk runs under the session's max_notes and
        redraws."""
        m = self._model
        n = _num_steps(self.steps, num_steps, max(s._gen.subs_per_step for s in self._subs))
        temperature, cond, _ = m._generate_arguments(n, given, given_mask, temperature)
        snap = self.snapshot() if len(self._subs) > 1 else None      # several generators advance one after another: a chunk that fails half way leaves none of them advanced
        try:
            out = m._sample_generators([s.generate for s in self._subs], n, cond, temperature, session=True)
        except BaseException:
            if snap is not None:
                self.restore(snap)
            raise
        self.steps += n
        return out
