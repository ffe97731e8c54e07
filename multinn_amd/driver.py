"""train.py:138-282 counterpart: the batching / windowing loop, loss accumulation,
best/last checkpoint policy and early stopping around ``Generator.train_step``.

Same YAML keys as multinn/configs/default_config.yaml / default_params.yaml and the same CLI flags as
train.py:287-329 (``python -m multinn_amd.driver -m NAME -c CONFIG -p PARAMS``).  Every mode of
``params['mode']`` is wired through ``multinn_amd.modes`` (``build_model``); joint + PassEncoder + NADE takes the
fused, hipGraph-replayed RnnNade step directly.
"""
import argparse
import math
import os
import pickle
import sys
import time

import numpy as np

from .switches import flag


class LossAccumulator:
    """Running mean of the per-batch losses of an epoch that keeps non-finite values OUT of the mean and tallies them by kind (the
    behaviour train.py:150-195 relies on from utils/training.py:98-148: a NaN batch is reported, not averaged)."""

    KINDS = ("nan", "+inf", "-inf")

    def __init__(self):
        self.clear()

    def clear(self):
        self.finite_sum, self.finite_n = 0.0, 0
        self.bad = dict.fromkeys(self.KINDS, 0)

    @staticmethod
    def _kind(x):
        if math.isnan(x):
            return "nan"
        if math.isinf(x):
            return "+inf" if x > 0 else "-inf"
        return None

    def update(self, loss):
        loss = float(loss)
        kind = self._kind(loss)
        if kind is None:
            self.finite_sum += loss
            self.finite_n += 1
        else:
            self.bad[kind] += 1

    def loss(self):
        return self.finite_sum / self.finite_n if self.finite_n else float("nan")

    def num_bad(self):
        return sum(self.bad.values())

    def ratio_bad(self):
        seen = self.finite_n + self.num_bad()
        return self.num_bad() / seen if seen else 0.0

    def __str__(self):
        tally = ", ".join(f"{k}: {n}" for k, n in self.bad.items())
        return f" - loss: {self.loss():7.3f} ({tally}, bad: {100.0 * self.ratio_bad():.2f}%)"


class TrainingStats:
    """utils/training.py:12-95: (steps, epoch, run, metric_best) pickled next to the checkpoint."""

    def __init__(self):
        self.steps, self.epoch, self.run, self.metric_best, self.idle_epochs = 0, 0, 1, float("inf"), 0

    def new_step(self):
        self.steps += 1

    def new_epoch(self):
        self.epoch += 1

    def new_idle_epoch(self):
        self.idle_epochs += 1

    def reset_idle_epochs(self):
        self.idle_epochs = 0

    def update_metric_best(self, m):
        self.metric_best = m

    def save(self, path):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump((self.steps, self.epoch, self.run, self.metric_best), f)

    def load(self, path):
        if not os.path.exists(path):
            return False
        with open(path, "rb") as f:
            self.steps, self.epoch, self.run, self.metric_best = pickle.load(f)
        self.run += 1
        return True


def iter_windows(ids, lengths, T_total, batch_size, piece_size):
    """train.py:164-173: for every batch of shuffled song ids and every piece of ``piece_size`` steps yield
    (song_ids, j, max_length, clipped_lengths) for the songs that still have steps (empty songs dropped)."""
    lengths = np.asarray(lengths)
    for i in range(0, len(ids), batch_size):
        batch = ids[i:i + batch_size]
        for j in range(0, T_total, piece_size):
            len_batch = lengths[batch] - j
            non_empty = np.where(len_batch > 0)[0]
            if len(non_empty) > 0:
                lb = np.minimum(len_batch[non_empty], piece_size)
                yield batch[non_empty], j, int(lb.max()), lb.astype(np.int32)
        yield None                                    # end of a song batch: stats.new_step() (train.py:194)


def _dataset(X):
    """X if it is a device-resident dataset (device_data.DeviceDataset), else None: a NumPy X keeps the host path of every function below."""
    if isinstance(X, np.ndarray):
        return None
    from .device_data import DeviceDataset
    return X if isinstance(X, DeviceDataset) else None


def _host_only(drain_every):
    if drain_every is not None:
        raise ValueError("drain_every batches the loss read-backs of a DeviceDataset; a NumPy X reads every loss as it is produced")


class _Augment:
    """A data.Transpose bound to one training set for one epoch: the moving tracks (as a list and as the kernels' bit mask) and the epoch's
    shift per song (int32 [S], positions of the pitch axis).  The shifts are drawn once, here; nothing of the global np.random is used."""

    def __init__(self, augment, X, lengths, epoch):
        from .data import Transpose, moving_bits, pitch_extents
        if not isinstance(augment, Transpose):
            raise ValueError(f"augment must be a data.Transpose or None, got {type(augment).__name__}")
        P, M = X.shape[2:]
        self.tracks = augment.bind(P, M)
        self.bits = moving_bits(self.tracks, M)
        ds = _dataset(X)
        if ds is not None:
            extents = ds.extents(self.tracks)
        else:                                             # a NumPy X: computed once per array and lengths, kept on the Transpose
            kept = getattr(augment, "_host_extents", None)
            if kept is None or kept[0] is not X or not np.array_equal(kept[1], lengths):
                kept = augment._host_extents = (X, np.array(lengths), pitch_extents(X, lengths, self.tracks))
            extents = kept[2]
        self.shifts = augment.shifts(extents, epoch, P)

    def apply(self, xb, song_ids):
        """The NumPy path: the fancy-indexed window [B, Tw, P, M], transposed."""
        from .data import transpose_rolls
        return transpose_rolls(xb, self.shifts[song_ids], self.tracks)


def _dataset_windows(ds, lengths, ids, batch_size, piece_size, shifts=None):
    """iter_windows over a DeviceDataset, with the song ids of the WHOLE epoch uploaded once (int32, the windows' ids back to back) in front
    of the first step: yields None, or (song_ids, j, max_length, clipped_lengths, ids_dev, shifts_dev) with ids_dev the window's slice of
    that upload.  shifts (int32 [S], a shift per song) ride in the same upload, laid out like the ids behind them, and shifts_dev is the
    window's slice of those; None without shifts."""
    if lengths is not None and not np.array_equal(np.asarray(lengths), ds.lengths):
        raise ValueError("the lengths passed beside a DeviceDataset differ from the dataset's own (pass None, or the ones it was built with)")
    if len(ids):
        ds.check_ids(ids)                                 # before they index the host lengths
    windows = list(iter_windows(ids, ds.lengths, ds.shape[1], batch_size, piece_size))
    real = [w[0] for w in windows if w is not None]
    shifts_dev = None
    if shifts is None or not real:
        ids_dev, at = ds.upload_ids(np.concatenate(real)) if real else None, 0
    else:
        import torch
        row_ids = np.concatenate(real)
        both = torch.from_numpy(np.stack([row_ids, shifts[row_ids]]).astype(np.int32)).to(ds.device)
        (ids_dev, shifts_dev), at = both, 0
    for w in windows:
        if w is None:
            yield None
            continue
        n = len(w[0])
        yield w + (ids_dev[at:at + n], None if shifts_dev is None else shifts_dev[at:at + n])
        at += n


class LossRing:
    """The losses of consecutive steps, kept on the device and read back in batches: `put` copies a loss TENSOR into the next slot of a small
    ring (no synchronisation: the host runs ahead of the device) and `drain` hands the slots to `sink(value, note)` in step order -- when the
    ring is full, every `drain_every` puts if given, and at `flush` (the end of an epoch).  A loss that already is a host number goes to the
    sink at once, behind whatever the ring still holds, so the sink sees every loss in step order and ends in the state that per-step
    `float(loss)` reads would have left.  The slots are float64: every float dtype a step returns converts to it exactly, like float() does."""

    def __init__(self, sink, slots=1024, drain_every=None):
        if drain_every is not None and drain_every < 1:
            raise ValueError(f"drain_every must be a positive number of steps, got {drain_every}")
        self.sink, self.slots = sink, slots if drain_every is None else min(slots, drain_every)
        self._ring, self._notes = None, []

    def put(self, loss, note=None):
        import torch
        if not isinstance(loss, torch.Tensor):
            self.flush()
            self.sink(float(loss), note)
            return
        if self._ring is None or self._ring.device != loss.device:
            self.flush()
            self._ring = torch.empty(self.slots, dtype=torch.float64, device=loss.device)
        self._ring[len(self._notes)].copy_(loss.detach().reshape(()))
        self._notes.append(note)
        if len(self._notes) == self.slots:
            self.drain()

    def flush(self):
        if self._notes:
            self.drain()

    def drain(self):
        """One device synchronisation and one copy for all the losses held."""
        notes, self._notes = self._notes, []
        for value, note in zip(self._ring[:len(notes)].tolist(), notes):
            self.sink(value, note)


def _train_epoch_dataset(generator, ds, lengths, ids, batch_size, piece_size, optimizer, loss_accum, stats, lr, drain_every, aug=None):
    """train_epoch over a DeviceDataset: the same windows in the same order, cut out of the dataset on its device; the same step."""
    ring = LossRing(lambda value, _: loss_accum.update(value), drain_every=drain_every)
    for w in _dataset_windows(ds, lengths, ids, batch_size, piece_size, None if aug is None else aug.shifts):
        if w is None:
            stats.new_step()
            continue
        song_ids, j, max_len, len_batch, ids_dev, shifts_dev = w
        if aug is None:
            xb, lb = ds.window(song_ids, j, max_len, ids_dev=ids_dev)
        else:
            xb, lb = ds.window(song_ids, j, max_len, ids_dev=ids_dev, shifts_dev=shifts_dev, moving=aug.bits)
        xb = xb.view(xb.shape[0], max_len, *ds.shape[2:])             # [B, Tw, P, M], what the NumPy path feeds
        full = bool((len_batch == max_len).all())
        lb = None if full else lb
        run = _captured_step(generator, xb, optimizer, lr, lengths=lb)
        if run is not None:
            loss = run(xb) if full else run(xb, lb)
        else:
            loss = generator.train_step(xb, lb, optimizer, lr)
        ring.put(loss)
    ring.flush()
    return loss_accum.loss()


def train_epoch(generator, X, lengths, ids, batch_size, piece_size, optimizer, loss_accum, stats, lr=None, device=None, drain_every=None,
                augment=None):
    """One epoch of train.py:164-194.  X uint8 [S,T,P,M] (numpy); every window starts from a ZERO rnn state.
    X may be a DeviceDataset instead (lengths: None or its own; `device` is the dataset's): the windows are cut out of it on the device and
    the losses are read back in one batch at the end of the epoch (LossRing), or every `drain_every` steps.
    augment (a data.Transpose, or None): every song's moving tracks are transposed by the shift it draws for (its seed, stats.epoch, song)
    -- inside the gather of a DeviceDataset, by data.transpose_rolls on the NumPy path; both feed the step the same bytes."""
    import torch
    aug = None if augment is None else _Augment(augment, X, lengths, stats.epoch)
    if _dataset(X) is not None:
        return _train_epoch_dataset(generator, X, lengths, ids, batch_size, piece_size, optimizer, loss_accum, stats, lr, drain_every, aug)
    _host_only(drain_every)
    for w in iter_windows(ids, lengths, X.shape[1], batch_size, piece_size):
        if w is None:
            stats.new_step()
            continue
        song_ids, j, max_len, len_batch = w
        xw = X[song_ids, j:j + max_len]
        xb = torch.from_numpy(np.ascontiguousarray(xw if aug is None else aug.apply(xw, song_ids))).to(device or "cuda")
        full = bool((len_batch == max_len).all())
        lb = None if full else torch.from_numpy(len_batch).to(xb.device)
        run = _captured_step(generator, xb, optimizer, lr, lengths=lb)
        if run is not None:
            loss = run(xb) if full else run(xb, lb)
        else:
            loss = generator.train_step(xb, lb, optimizer, lr)
        loss_accum.update(float(loss))
    return loss_accum.loss()


def _captured_step(generator, xb, optimizer, lr, max_graphs=8, lengths=None):
    """An eager optimiser step is host-bound (C2 shape: 7.2 ms eager, 2.85 ms as a hipGraph replay), so windows of a shape that keeps
    coming back -- batch_size x piece_size, i.e. nearly all of an epoch -- run as replays of the model's graphed_train_step (RnnNade,
    MultINNCore), for the windows its `capturable(shape, ragged)` accepts.
    A shape is captured at its SECOND occurrence (the first one runs eagerly and creates every workspace; capturing executes nothing,
    so the trajectory is the eager one), keyed by optimiser and learning rate (both are baked into the graph).
    RAGGED windows (lengths given) get their own graph beside the full-length one of the same shape, which skips the compaction passes:
    ONE graph per window shape serves any lengths (the reference's data is ragged, train.py:165-173).  MULTINN_TRAIN_GRAPH=0 keeps every
    step eager."""
    ragged = lengths is not None
    if not flag("MULTINN_TRAIN_GRAPH") or not xb.is_cuda or not hasattr(generator, "capturable") \
            or not generator.capturable(tuple(xb.shape), ragged):
        return None
    key = (tuple(xb.shape), id(optimizer), lr, "ragged" if ragged else "full")
    graphs = generator.__dict__.setdefault("_step_graphs", {})
    if key in graphs:
        return graphs[key]
    seen = generator.__dict__.setdefault("_step_shapes_seen", set())
    if key not in seen or len(graphs) >= max_graphs:
        seen.add(key)
        return None
    graphs[key] = generator.graphed_train_step(xb, optimizer, lr, warmup=0, lengths=lengths)
    return graphs[key]


def evaluate(generator, X, lengths, batch_size, piece_size, device=None, nll="loss", ais=None, given_mask=None, partial="refuse", drain_every=None):
    """utils/training.py:180-213 collect_metrics: mean generator NLL per valid row over all windows.
    nll="loss" (default): the training loss (an RBM generator's is the CD cost, a difference of free energies, not a likelihood).
    nll="ais": the model's estimate_nll(x, lengths, **ais) -- exact for NADE generators, annealed importance sampling for RBM generators
    (biased low), summed over a mode's generators.
    nll="raise": the same with estimate_nll(method="raise") -- reverse AIS, biased the other way (conservative).
    nll="bracket": estimate_nll(method="both"); returns {"lower": the "ais" mean, "upper": the "raise" mean, "gap": upper - lower}, each
    equal to its own call's value: a gap well above its noise says the ladder (ais: num_betas) is too short for either end to be trusted.
    given_mask (optional, with nll "ais" / "raise" / "bracket"): a batch-independent bool mask, [M] or [P, M], passed to every window's
    estimate_nll -- the mean CONDITIONAL NLL per valid step of the cells outside the mask given those under it (and the past).
    partial ("refuse" or "importance", with given_mask): estimate_nll's -- "importance" estimates a NADE that the mask leaves partly given
    by importance sampling (ais: num_chains particles per row) where "refuse" raises; nll "bracket" then reports its two sides and their gap.
    X may be a DeviceDataset (lengths: None or its own): every window is cut out of it on its device, and nll="loss" reads its losses back
    in one batch (LossRing; every `drain_every` windows if given) -- the estimator modes take the gathered window and are otherwise unchanged."""
    import torch
    methods = {"ais": "ais", "raise": "raise", "bracket": "both"}
    if nll != "loss" and nll not in methods:
        raise ValueError(f"nll must be 'loss', 'ais', 'raise' or 'bracket', got {nll!r}")
    cond = {}
    if partial not in ("refuse", "importance"):
        raise ValueError(f"partial must be 'refuse' or 'importance', got {partial!r}")
    if given_mask is not None:
        if nll == "loss":
            raise ValueError("given_mask needs nll 'ais', 'raise' or 'bracket': the training loss has no conditional form")
        given_mask = torch.as_tensor(given_mask)
        if given_mask.dtype != torch.bool or given_mask.dim() not in (1, 2):
            raise ValueError(f"given_mask must be a batch-independent bool mask [M] or [P, M], got {given_mask.dtype} {tuple(given_mask.shape)}")
        cond = dict(given_mask=given_mask) if partial == "refuse" else dict(given_mask=given_mask, partial=partial)
    tot, cnt, tot_upper = 0.0, 0, 0.0
    ids = np.arange(X.shape[0])
    ds = _dataset(X)
    if ds is None:
        _host_only(drain_every)
        windows = iter_windows(ids, lengths, X.shape[1], batch_size, piece_size)
    else:
        windows = _dataset_windows(ds, lengths, ids, batch_size, piece_size)
        weighted = [0.0]

        def add_weighted(value, n):
            weighted[0] += value * n
        ring = LossRing(add_weighted, drain_every=drain_every)
    for w in windows:
        if w is None:
            continue
        song_ids, j, max_len, len_batch = w[:4]
        full = bool((len_batch == max_len).all())
        if ds is None:
            xb = torch.from_numpy(np.ascontiguousarray(X[song_ids, j:j + max_len])).to(device or "cuda")
            lb = None if full else torch.from_numpy(len_batch).to(xb.device)
        else:
            xb, lb = ds.window(song_ids, j, max_len, ids_dev=w[4])
            xb, lb = xb.view(xb.shape[0], max_len, *ds.shape[2:]), None if full else lb
        if nll != "loss":
            n = int(len_batch.sum())
            est = generator.estimate_nll(xb, lb, **dict(ais or {}, method=methods[nll]), **cond)
            tot += (est.lower if nll == "bracket" else est).mean * n
            tot_upper += est.upper.mean * n if nll == "bracket" else 0.0
            cnt += n
            continue
        generator.build_pianoroll(xb, lb, is_train=False, mode="eval")
        n = int(len_batch.sum())
        loss = generator.generator_loss() if hasattr(generator, "generator_loss") else generator.metrics["batch/loss"]
        if ds is None:
            tot += float(loss) * n
        else:
            ring.put(loss, n)
        cnt += n
    if ds is not None:
        ring.flush()
        tot += weighted[0]
    if nll == "bracket":
        lower, upper = tot / max(cnt, 1), tot_upper / max(cnt, 1)
        return {"lower": lower, "upper": upper, "gap": upper - lower}
    return tot / max(cnt, 1)


def check_recurrences(model):
    """Raise if any persistent-recurrence launch of the model's LSTM stacks timed out on a bounded spin since the last check (its sticky
    status word: LstmStack.check / MultINNCore.check; synchronises the device).  The persistent and row-parallel recurrence launches need
    their whole grid resident at once; one that could not become resident returns garbage and only sets that word."""
    if hasattr(model, "check"):
        model.check(tolerate_overflow=True)          # the training loop: f16 overflows are answered by the dynamic loss scale (a warning)
    elif getattr(model, "_stack", None) is not None:
        model._stack.check()


def fit(generator, optimizer, X_train, len_train, X_valid, len_valid, training_config, logs_config, dirs, stats=None, beat_size=4,
        save_best_only=False, log=print, pitch_stride=1):
    """train.py:150-282: epochs, shuffling (np.random.seed(epoch)), evaluation, best / last checkpoints,
    early stopping after ``early_stopping`` idle epochs.
    training_config["transpose"] (optional, a mapping {max_shift, fixed_tracks}): the TRAINING windows are transposed (data.Transpose,
    seeded with random_seed; pitch_stride: positions of the pitch axis per semitone, `num_pixels` in `main`); validation never is."""
    stats = stats or TrainingStats()
    augment = None
    if training_config.get("transpose") is not None:
        from .data import Transpose
        tp = training_config["transpose"]
        if not isinstance(tp, dict) or "max_shift" not in tp or set(tp) - {"max_shift", "fixed_tracks"}:
            raise ValueError(f"training.transpose must be a mapping {{max_shift, fixed_tracks}}, got {tp!r}")
        augment = Transpose(tp["max_shift"], tuple(tp.get("fixed_tracks") or ()), seed=training_config["random_seed"], pitch_stride=pitch_stride)
        augment.bind(*X_train.shape[2:])
    batch_size = training_config["batch_size"]
    piece_size = int(training_config["piece_size"] * beat_size)
    ids = np.arange(X_train.shape[0])
    acc = LossAccumulator()
    past = stats.epoch
    for epoch in range(past + 1, past + training_config["epochs"] + 1):
        stats.new_epoch()
        np.random.seed(epoch)
        t0 = time.time()
        np.random.shuffle(ids)
        acc.clear()
        if augment is None:
            train_epoch(generator, X_train, len_train, ids, batch_size, piece_size, optimizer, acc, stats, training_config.get("learning_rate"))
        else:
            train_epoch(generator, X_train, len_train, ids, batch_size, piece_size, optimizer, acc, stats, training_config.get("learning_rate"),
                        augment=augment)
        check_recurrences(generator)            # a persistent launch that gave up would have trained on garbage: raise before validating / saving
        loglik_val = evaluate(generator, X_valid, len_valid, batch_size, piece_size) if logs_config.get("evaluate_epochs", 1) else acc.loss()
        log(f" epoch: {epoch:3d} (steps: {stats.steps:5d}) time: {time.time() - t0:.2f}s{acc} valid nll: {loglik_val:.4f}")
        if loglik_val < stats.metric_best:
            stats.update_metric_best(loglik_val)
            stats.reset_idle_epochs()
            if logs_config.get("save_checkpoint_epochs", 1) > 0 and epoch % logs_config.get("save_checkpoint_epochs", 1) == 0:
                generator.save(None, dirs["model_dir"], global_step=stats.steps)
                stats.save(os.path.join(dirs["model_dir"], "steps"))
        else:
            stats.new_idle_epoch()
            if stats.idle_epochs >= training_config["early_stopping"]:
                log(f"[WARN]  No improvement after {training_config['early_stopping']} epochs, quiting")
                break
    check_recurrences(generator)
    if not save_best_only:
        generator.save(None, dirs["model_last_dir"], global_step=stats.steps)
        stats.save(os.path.join(dirs["model_last_dir"], "steps"))
    return stats


def pretrain_encoders(encoders, X_train, len_train, training_config, beat_size=4, lr=None, device=None, log=None, augment=None):
    """train_encoders.py:118-200: greedy layer-wise pre-training of the per-track (or joint) DBN encoders.  For every layer, for
    `epochs` epochs, every shuffled song batch and every piece of `piece_size` beats: the encoder is built on the window of its
    track (`x[..., i]` for track i, all tracks flattened for a single joint encoder) and `encoder.train(None, lr, layer)` runs one
    CD-k update of that layer's RBM fed with the sampled codes of the layers below (dbn_encoder.py:192-240).
    X_train uint8 [songs, T, P, M] (numpy), or a DeviceDataset (len_train: None or its own): track i's windows are then gathered on its device.
    augment (a data.Transpose, or None): train_epoch's, with the loop's own `epoch`; a per-track encoder gets its track's single-track form.
    Returns {(encoder index, layer): [mean reconstruction cost per epoch]}."""
    import torch
    batch_size = training_config['batch_size']
    piece_size = int(training_config['piece_size'] * beat_size)
    lr = training_config['learning_rate'] if lr is None else lr
    ids = np.arange(X_train.shape[0])
    ds = _dataset(X_train)
    history = {}
    for e_i, enc in enumerate(encoders):
        for layer in range(enc.num_layers):
            costs = []
            for epoch in range(1, training_config['epochs'] + 1):
                np.random.seed(epoch)                           # train_encoders.py:134-135
                np.random.shuffle(ids)
                acc = LossAccumulator()
                aug = None if augment is None else _Augment(augment, X_train, len_train, epoch)
                if ds is None:
                    windows = iter_windows(ids, len_train, X_train.shape[1], batch_size, piece_size)
                else:
                    windows = _dataset_windows(ds, len_train, ids, batch_size, piece_size, None if aug is None else aug.shifts)
                    ring = LossRing(lambda value, _, acc=acc: acc.update(value))
                for w in windows:
                    if w is None:
                        continue
                    song_ids, j, max_len = w[:3]
                    if ds is None:
                        xb = X_train[song_ids, j:j + max_len]
                        xb = xb if aug is None else aug.apply(xb, song_ids)
                        xb = xb[..., e_i] if len(encoders) > 1 else xb.reshape(xb.shape[0], xb.shape[1], -1)
                        xt = torch.from_numpy(np.ascontiguousarray(xb)).to(device or "cuda")
                    else:
                        shifted = {} if aug is None else dict(shifts_dev=w[5], moving=aug.bits)
                        xt, _ = ds.window(song_ids, j, max_len, track=e_i if len(encoders) > 1 else None, ids_dev=w[4], **shifted)
                    enc.build(x=xt, is_train=True, mode="train")
                    _, _, metrics, _, _ = enc.train(None, lr, layer=layer)
                    if ds is None:
                        acc.update(float(metrics["batch/loss"]) if metrics else 0.0)
                    else:
                        ring.put(metrics["batch/loss"] if metrics else 0.0)
                if ds is not None:
                    ring.flush()
                costs.append(acc.loss())
                if log is not None:
                    log(f"[PRETRAIN] encoder {e_i} layer {layer} epoch {epoch}: reconstruction cost {costs[-1]:.4f}")
            history[(e_i, layer)] = costs
    return history


def build_generator(params, P, M, precision="bf16", seed=23):
    """multinn_joint.py:41-74 for `mode: joint`, `encoder.type: Pass`, `generator.type: NADE|RBM`: the bare generator (kept for
    callers that drive a Generator directly; `build_model` wires every mode)."""
    from .generators import RnnNade, RnnRBM
    if params.get("mode", "joint") != "joint" or (params.get("encoder") or {}).get("type", "Pass") != "Pass":
        raise ValueError("build_generator is the joint / PassEncoder shortcut: use build_model(config, params) for the other modes")
    g = params["generator"]
    if g["type"] == "MultiRBM":
        raise ValueError("generator type `MultiRBM` is the composer mode's (one shared LSTM, one RBM per track): use build_model(config, params) "
                         "with mode: composer")
    cls = {"NADE": RnnNade, "RBM": RnnRBM}[g["type"]]
    return cls(P * M, g["num_hidden"], g["num_hidden_rnn"], keep_prob=params.get("keep_prob", 0.9), precision=precision, seed=seed,
               learn_zero_state=bool(g.get("learn_zero_state", False)))


def build_model(config, params, precision="bf16", seed=None, device=None):
    """train.py:50: `MultINN(config, params, mode=params['mode'], name=config['model_name'])` -- any of the five modes
    (multinn_amd.modes), with the train_step / build_pianoroll / save / load surface `fit` drives."""
    from .modes import MultINN
    return MultINN(config, params, mode=params["mode"], name=config.get("model_name", "MultINN"), precision=precision, seed=seed, device=device)


def main(argv=None):
    import yaml
    ap = argparse.ArgumentParser(description="MultINN joint LSTM-NADE training on MI355X (flags of multinn/train.py)")
    ap.add_argument("--model-name", "-m", required=True)
    ap.add_argument("--config", "-c", default="configs/default_config.yaml")
    ap.add_argument("--params", "-p", default="configs/default_params.yaml")
    ap.add_argument("--epochs", "-e", type=int, default=None)
    ap.add_argument("--learning-rate", "--lr", type=float, default=None)
    ap.add_argument("--from-init", action="store_true")
    ap.add_argument("--from-last", action="store_true")
    ap.add_argument("--encoders", default=None)
    ap.add_argument("--save-best-only", action="store_true")
    ap.add_argument("--reuse-config", action="store_true")
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16", "fp32"],
                    help="fp16: IEEE-half operands, the mode that meets the 1e-4 parity gate at full speed; bf16; fp32: v_mfma_f32 GEMMs, launch-per-step recurrence")
    ap.add_argument("--device-data", action="store_true",
                    help="keep the train and validation splits on the device (DeviceDataset): windows are cut out of them there, losses read back per epoch")
    a = ap.parse_args(argv)
    from .training import AdamOptimizer
    root = os.path.join("..", "results", a.model_name)                  # utils/setup.py:50
    dirs = dict(model_dir=os.path.join(root, "ckpt", "model"), model_last_dir=os.path.join(root, "ckpt", "model", "last"),
                config_dir=os.path.join(root, "config"))
    if a.reuse_config:
        a.config, a.params = os.path.join(dirs["config_dir"], "config.yaml"), os.path.join(dirs["config_dir"], "params.yaml")
    config, params = yaml.safe_load(open(a.config)), yaml.safe_load(open(a.params))
    if a.epochs is not None:
        config["training"]["epochs"] = a.epochs
    if a.learning_rate is not None:
        config["training"]["learning_rate"] = a.learning_rate
    os.makedirs(dirs["config_dir"], exist_ok=True)
    yaml.safe_dump(config, open(os.path.join(dirs["config_dir"], "config.yaml"), "w"))
    yaml.safe_dump(params, open(os.path.join(dirs["config_dir"], "params.yaml"), "w"))
    d, tr = config["data"], config["training"]
    X = np.load(d["filename"] if d["filename"].endswith(".npy") else d["filename"] + ".npy").astype(np.uint8)
    npx = tr.get("num_pixels", 1)
    if npx > 1:                                                            # utils/data.py:71-79
        S, T, P, M = X.shape
        X = X[:, :T // npx * npx].reshape(S, T // npx, npx, P, M).transpose(0, 1, 3, 2, 4).reshape(S, T // npx, P * npx, M)
    lengths = np.full(X.shape[0], X.shape[1], np.int64) if not d.get("sequence_lengths") else np.load(d["sequence_lengths"]) // npx
    nt, nv = d["split"]["num_train"], d["split"]["num_valid"]
    if params.get("mode", "joint") == "joint" and (params.get("encoder") or {}).get("type", "Pass") == "Pass" \
            and params["generator"]["type"] == "NADE":
        gen = build_generator(params, X.shape[2], X.shape[3], a.precision, tr["random_seed"])     # the fused, hipGraph-replayed step
        gen._materialize(X.shape[2] * X.shape[3])
    else:
        config.setdefault("data", {}).setdefault("pitch_range", {"lowest": 0, "highest": X.shape[2] // max(npx, 1)})
        gen = build_model(config, params, a.precision, tr["random_seed"])
    stats = TrainingStats()
    if not a.from_init:
        src = dirs["model_last_dir"] if a.from_last else dirs["model_dir"]
        if gen.load(None, src):
            stats.load(os.path.join(src, "steps"))
    X_train, X_valid = X[:nt], X[nt:nt + nv]
    if a.device_data:
        from .device_data import DeviceDataset
        X_train, X_valid = DeviceDataset(X_train, lengths[:nt]), DeviceDataset(X_valid, lengths[nt:nt + nv])
    fit(gen, AdamOptimizer(tr["learning_rate"]), X_train, lengths[:nt], X_valid, lengths[nt:nt + nv], tr, config["logs"], dirs, stats,
        beat_size=d["beat_resolution"] / npx, save_best_only=a.save_best_only, pitch_stride=npx)


if __name__ == "__main__":
    main()
