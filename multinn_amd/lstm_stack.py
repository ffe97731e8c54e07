"""LstmStack: a multi-layer LSTM on packed, gate-interleaved weights, and the drivers of its recurrence launches (drive / drive_group).
Imported back by name into multinn_amd.generators, which every model builds on."""
import math
from typing import NamedTuple

import torch

from . import ops
from .switches import flag, value


# ------------------------------------------------------------------------------------------------
# Lockstep execution of several generators (the M per-track generators of the jamming mode, multinn_jamming.py:40-68,213-221).  The parts of a
# generator that launch an LSTM recurrence are written as Python generator functions (`*_co`) that YIELD the launch instead of issuing it:
#     ("resident_fwd" | "resident_bwd" | "cluster_fwd" | "cluster_bwd" | "rowpar_fwd" | "rowpar_bwd", T, B, descriptor, keep_prob, workspace)
# `drive` runs one of them alone (every request becomes its own launch: the ordinary path).  `drive_group` advances M of them side by side and
# turns the M requests of a rendezvous into ONE launch where the library has a multi-job form (ops.lstm_recurrence_multi: the CU-resident and
# cluster recurrences own their rows for the whole sequence, so independent layers simply share a grid); everything between two rendezvous
# (GEMMs, Gibbs chains, ...) is issued per generator, in generator order, on the same stream.
# A backward request of the resident / cluster form may carry a seventh element: dc0 f32 [B, u], the output for the gradient wrt the layer's
# initial cell state (a stack that started from a state: LstmStack.backward(need_dstate=True)).
_SINGLE = {"resident_fwd": lambda T, B, d, kp, ws: ops.lstm_resident_fwd(T, B, d, kp),
           "resident_bwd": lambda T, B, d, kp, ws, dc0=None: ops.lstm_resident_bwd(T, B, d, kp, dc0),
           "cluster_fwd": lambda T, B, d, kp, ws: ops.lstm_cluster_fwd(T, B, d, kp, ws),
           "cluster_bwd": lambda T, B, d, kp, ws, dc0=None: ops.lstm_cluster_bwd(T, B, d, kp, ws, dc0),
           "rowpar_fwd": lambda T, B, d, kp, ws: ops.lstm_rowpar_fwd(T, B, d, kp, ws),
           "rowpar_bwd": lambda T, B, d, kp, ws: ops.lstm_rowpar_bwd(T, B, d, kp, ws)}


def drive(co):
    """Run one `*_co` generator function to its end, issuing every recurrence it asks for as a launch of its own; returns its return value."""
    try:
        req = next(co)
        while True:
            _SINGLE[req[0]](*req[1:])
            req = co.send(None)
    except StopIteration as e:
        return e.value


def drive_group(cos):
    """Run M `*_co` generator functions in lockstep (see above); returns the list of their return values.  They must ask for the same
    sequence of recurrences (same kinds and shapes: the caller checks that the generators are alike before grouping them)."""
    n = len(cos)
    results, reqs, alive = [None] * n, [None] * n, [True] * n

    def advance(i, first):
        try:
            reqs[i] = next(cos[i]) if first else cos[i].send(None)
        except StopIteration as e:
            results[i], reqs[i], alive[i] = e.value, None, False

    for i in range(n):
        advance(i, True)
    while any(alive):
        if not all(alive):
            raise RuntimeError("drive_group: the grouped generators did not ask for the same sequence of recurrences")
        kind, T, B, kp = reqs[0][0], reqs[0][1], reqs[0][2], reqs[0][4]
        same = all(r[0] == kind and r[1] == T and r[2] == B and r[4] == kp and r[3].units == reqs[0][3].units for r in reqs)
        multi = same and n > 1 and kind.split("_")[0] in ("resident", "cluster")
        if multi and kind == "cluster_bwd" and not ops.lstm_cluster_bwd_multi_ok(B, reqs[0][3].units, n):
            multi = False
        if multi and kind.startswith("cluster") and (n * (B // 32)) % 8 != 0:
            multi = False
        if multi:
            ops.lstm_recurrence_multi(kind, T, B, [r[3] for r in reqs], kp, [r[5] for r in reqs] if kind.startswith("cluster") else None,
                                      [r[6] if len(r) > 6 else None for r in reqs])
        else:
            for r in reqs:
                _SINGLE[r[0]](*r[1:])
        for i in range(n):
            advance(i, False)
    return results


# ------------------------------------------------------------------------------------------------
class Plan(NamedTuple):
    """How one forward of an LstmStack, and the backward of what it saved, run (LstmStack.plan)."""
    path: str                 # "rowpar" | "persist" | "fused2" | "seq"
    fwd: tuple = ()           # "rowpar": each layer's forward kernel, "resident" | "cluster" | "rowpar"
    bwd: tuple = ()           # the same for each layer's backward kernel
    merged: bool = False      # "rowpar": [x^T ; h_prev^T] is one buffer per layer (one weight-gradient GEMM for dWx and dWh)


class LstmStack:
    """Executes an RNN (multi-layer LSTM) on packed, gate-interleaved weights."""

    def __init__(self, rnn, store, dtype):
        self.rnn, self.store, self.dtype = rnn, store, dtype
        self.al = 8 if dtype in ops.H16 else 4
        self.h16 = dtype in ops.H16                     # 16-bit operands (bf16 or IEEE half): the persistent / matrix-core forms apply
        self.ld0 = ops.round_up(rnn.n_in, 64)          # K of the input projection: multiple of 64 selects the LDS-DMA GEMM
        self.packed = None

    # IEEE half has 5 exponent bits: the backward pass of a mean-over-rows loss (seeds of 1/N ~ 4e-6 at the bench shape) would sit in its
    # subnormals.  The owner of a backward pass (RnnNade / RnnRBM / FeedbackRnn) multiplies its gradient seed by loss_scale(N) -- a power of
    # two, so every f32 result is the unscaled one times 2^k exactly -- and multiplies store.grad (and d loss / d inputs) by 1/scale at its
    # end: callers always see unscaled gradients.  The seed of a row is 1 / n_valid (VALID rows of all ranks, not B*T: on a ragged window the
    # two differ by up to max_len), so 256 * n_valid keeps |d logits| <= 256 and typical dz around 1..100 (f16: 6e-5 .. 65504) for ragged
    # batches too.  An overflow that happens anyway leaves a non-finite gradient norm: mnn_clip_adam_step skips that update on the device
    # and Generator.check() raises.
    loss_scale_rows = 256.0

    def loss_scale(self, n_valid):
        """n_valid: number of VALID rows the mean-over-rows loss divides by (summed over all ranks)."""
        if self.dtype != torch.float16:
            return 1.0
        if n_valid is None:
            raise RuntimeError("loss_scale: the valid-row count lives on the device (ragged_on_device): use the generator's device-side scale")
        return float(2.0 ** round(math.log2(self.loss_scale_rows * max(int(n_valid), 1))))

    def pack(self):
        dev = self.store.theta.device
        self.packed = []
        for l, (n_in, u) in enumerate(zip(self.rnn.layer_inputs(), self.rnn.num_units)):
            ld = self.ld0 if l == 0 else n_in
            p = dict(wx_t=torch.empty((4 * u, ld), device=dev, dtype=self.dtype), wh_t=torch.empty((4 * u, u), device=dev, dtype=self.dtype),
                     wh_p=torch.empty((u, 4 * u), device=dev, dtype=self.dtype),
                     wx_p=torch.empty((n_in, 4 * u), device=dev, dtype=self.dtype) if l > 0 else None,
                     bias_p=torch.empty(4 * u, device=dev), n_in=n_in, u=u, ld=ld)
            ops.lstm_pack_weights(self.store[f"{self.rnn.prefix}/cell_{l}/kernel"], self.store[f"{self.rnn.prefix}/cell_{l}/bias"], n_in, u,
                                  p["wx_t"], p["wh_t"], p["wh_p"], p["wx_p"], p["bias_p"])
            if self.h16 and (l == 0 or self.rowpar):
                # the persistent recurrences read xproj gate-minor: the projection GEMM gets the rows in that order (layer 1 of the two-layer
                # form; every layer of the row-parallel form, whose layers each have their own projection GEMM)
                p["wx_gm"], p["bias_gm"] = torch.empty_like(p["wx_t"]), torch.empty_like(p["bias_p"])
                ops.lstm_rows_gate_minor(p["wx_t"], p["bias_p"], p["wx_gm"], p["bias_gm"])
            self.packed.append(p)

    fused_layers = True   # run two-layer stacks as a wavefront inside single launches (mnn_lstm2_seq_*)

    def _fused2(self, B=0):
        """Two layers per launch pay off while one layer's step does not fill the chip (measured: C2 B=256 7.1 -> 6.2
        ms/step; TGT B=1024, 768 blocks per launch, 35.7 -> 36.4 ms/step)."""
        if not (self.fused_layers and len(self.packed) == 2 and self.dtype == torch.bfloat16
                and all(ops.lstm_fused_outputs(self.dtype, p["u"]) for p in self.packed)):
            return False
        blocks = sum(p["u"] // 32 for p in self.packed) * -(-max(B, 1) // 32)
        return blocks <= 512

    persistent = flag("MULTINN_PERSIST")   # one launch for all T steps (lstm_persist.hip) when the grid fits the device

    # A persistent launch spins on its own workgroups and needs ALL of them resident: two such launches must never share the device.
    # A caller that runs several stacks on concurrent streams (the feedback sampling scan) clears this for its single steps, which then
    # take the launch-per-step kernels (T = 1: nothing to keep resident anyway).
    persist_single_step = True

    def _persist(self, B, T=2):
        if not (self.persistent and len(self.packed) == 2 and self.h16):
            return False
        if T == 1 and not self.persist_single_step:
            return False
        return ops.lstm2_persist_ok(B, self.packed[0]["u"], self.packed[1]["u"])

    # Row-parallel persistent form (lstm_rowpar.hip): one launch per LAYER for all T steps, weights in LDS, a wave per 32-row tile.  For
    # large batches, where the two-layer form's fixed cost per 32-row item (K split over the waves, LDS reduction, workgroup barriers) is
    # paid several times per timestep: TGT [1024,256,88,5] forward 15.6 us per timestep there.
    rowpar = flag("MULTINN_ROWPAR")
    rowpar_min_batch = value("MULTINN_ROWPAR_MIN_BATCH")
    # input projections the row-parallel form reads (bias included): stored in the 16-bit compute type by default (half the bytes of the
    # step's largest tensor), f32 with MULTINN_ROWPAR_XPROJ=f32
    rowpar_xproj_f32 = value("MULTINN_ROWPAR_XPROJ") == "f32"

    # CU-resident form of a 256-unit layer inside the row-parallel path (lstm_resident.hip): the layer's whole recurrent matrix sits on every CU
    # and a workgroup owns four batch rows, so a timestep has no hand-off between workgroups (MULTINN_RESIDENT=0: row-parallel kernels only)
    resident = flag("MULTINN_RESIDENT")

    def _resident(self, l, B, T):
        # (the kernels address their tensors through 2 GB buffer descriptors: the saved gates [T, B, 4u] in 16 bits are the largest)
        return (self.resident and not self.rowpar_xproj_f32 and ops.lstm_resident_ok(B, self.packed[l]["u"])
                and T * B * self.packed[l]["u"] * 8 < 2 ** 31)

    # Cluster form of the same idea for a 512-unit layer (lstm_cluster.hip): eight CUs share 32 rows, each keeps 64 units' recurrent weights in
    # its registers, h[t] / dz[t] are exchanged through the XCD's L2 (MULTINN_CLUSTER=0: row-parallel kernels for that layer)
    cluster = flag("MULTINN_CLUSTER")

    def _cluster(self, l, B, T):
        return (self.cluster and not self.rowpar_xproj_f32 and ops.lstm_cluster_ok(B, self.packed[l]["u"])
                and T * B * self.packed[l]["u"] * 8 < 2 ** 31)

    def _cluster_bwd(self, l, B, T):
        """The cluster BACKWARD needs every cluster's eight workgroups on one XCD (its two-deep exchange area lives in that XCD's L2; the forward has
        a write-through fall-back).  The library asks the placement once per device and batch size on the host; when it says no -- a repartitioned
        device, MNN_PERSIST_NO_LOCAL -- this layer's backward takes the row-parallel kernels (same descriptors, same saved activations), said once."""
        if not (self._cluster(l, B, T) and T >= 4):
            return False
        if ops.lstm_cluster_bwd_ok(B, self.packed[l]["u"]):
            return True
        if not getattr(LstmStack, "_cluster_bwd_warned", False):
            LstmStack._cluster_bwd_warned = True
            import warnings
            warnings.warn("multinn_amd: the clusters of the 512-unit recurrence are not dealt onto single XCDs on this device; its backward runs on "
                          "the row-parallel kernels (lstm_rowpar_bwd) instead of lstm_cluster_bwd")
        return False

    @property
    def rowpar_xproj_dtype(self):
        return torch.float32 if self.rowpar_xproj_f32 else self.dtype

    # set by a mode that runs several stacks in lockstep (drive_group): the row-parallel path -- whose CU-resident / cluster recurrences have a
    # multi-job launch -- also below rowpar_min_batch, where one stack alone is faster on the two-layer persistent form
    group_rowpar = False

    def _rowpar(self, B, T=2, state0=None):
        if not (self.rowpar and self.h16 and state0 is None and T > 1 and (B >= self.rowpar_min_batch or self.group_rowpar) and B % 32 == 0):
            return False
        return all("wx_gm" in p and ops.lstm_rowpar_ok(B, p["u"]) for p in self.packed)

    def _rowpar_state0(self, B, T=2):
        """The row-parallel path for a stack that starts from an initial state: of its three recurrences only the CU-resident and the cluster
        form take one (and return its gradient), so every layer's forward AND backward must be theirs -- answered on the host, before the
        forward (the saved gates of this family and of the launch-per-timestep kernels differ).  Otherwise such a stack takes the
        launch-per-timestep path."""
        return self.plan(B, T, state0=True).path == "rowpar"

    def plan(self, B, T, state0=False, state_grad=False, save=True):
        """The one decision of a forward (and of the backward of what it saves): which of the recurrence forms runs, and for the row-parallel
        path which kernel each layer's forward and backward take.  state0 / state_grad / save: whether the forward starts from a state, will
        be asked for that state's gradient, and saves its activations."""
        if self._rowpar(B, T):
            layers = range(len(self.packed))
            fwd = tuple("resident" if self._resident(l, B, T) else "cluster" if self._cluster(l, B, T) else "rowpar" for l in layers)
            bwd = tuple("resident" if fwd[l] == "resident" else "cluster" if self._cluster_bwd(l, B, T) else "rowpar" for l in layers)
            if not state0 or "rowpar" not in fwd + bwd:
                return Plan("rowpar", fwd, bwd, bool(save and self.merge_wgrads))
        if self._persist(B, T) and not (state_grad and state0 and save):
            return Plan("persist")
        return Plan("fused2" if self._fused2(B) else "seq")

    def _rp_workspace(self, l, T, B, dev):
        if not hasattr(self, "_rpws"):
            self._rpws = {}
        key = (l, T, B)
        if key not in self._rpws:
            self._rpws[key] = ops.lstm_rowpar_workspace(T, B, self.packed[l]["u"], dev)
        return self._rpws[key]

    # One weight-gradient GEMM per layer over the concatenated operand [x^T ; h_prev^T] (row-parallel form): dz^T is streamed once for dWx and
    # dWh, and 2 x 4 column tiles of a K slice share every dz^T panel on an XCD's L2 instead of 2 x 2 (layer 1 at [1024,256,88,5]: 1.33 ->
    # 1.03 ms for the pair, scratch/gemm_merge_probe.py).  The layer's forward writes h^T -- and the layer below its y^T -- into views of it.
    merge_wgrads = flag("MULTINN_MERGE_WGRADS")

    def _cat_shape(self, l, Np):
        p = self.packed[l]
        return (p["ld"] + p["u"], Np)

    def input_T(self, T, B, dev):
        """Buffer for the caller's transposed copy of the stack's input (x^T [ld0, Np], layer 1's weight-gradient operand): a view of layer
        1's concatenated operand when the row-parallel form with merged weight-gradient GEMMs will run, else None (caller allocates)."""
        if not self.plan(B, T).merged:
            return None
        Np = ops.round_up(T * B, 64)
        self._cat0 = (torch.zeros if Np != T * B else torch.empty)(self._cat_shape(0, Np), device=dev, dtype=self.dtype)
        return self._cat0[:self.packed[0]["ld"]]

    def _forward_rowpar_co(self, plan, x_tm, keep_prob, seed, row0, save, step_dev, state0=None):
        """Layer by layer: gate-minor input projection (one GEMM over all T*B rows), then the layer's whole recurrence in one launch -- YIELDED
        to the driver (drive / drive_group above), which issues it alone or together with the same layer of other stacks.
        state0 ([(c0 f32, h0) [B, u]] per layer; only where the plan has no row-parallel kernel, _rowpar_state0): h0 rounded to the compute type and c0 go into the layer's
        descriptor, h0^T into columns [0, B) of h^T -- which puts the t = 0 term into dWh through the weight-gradient GEMM."""
        T, B, _ = x_tm.shape
        dev, N = x_tm.device, T * B
        Np = ops.round_up(N, 64)
        zalloc = torch.zeros if Np != N else torch.empty
        inp, ctx, final = x_tm, [], []
        cats = [None] * len(self.packed)
        if plan.merged:
            for l, p in enumerate(self.packed):
                if l > 0 and p["ld"] != self.packed[l - 1]["u"]:
                    continue                            # a padded input pitch: the layer below's y^T is not this layer's x^T row for row
                c0 = getattr(self, "_cat0", None) if l == 0 else None
                if c0 is not None and tuple(c0.shape) == self._cat_shape(0, Np) and c0.device == dev:
                    cats[l], self._cat0 = c0, None
                else:
                    cats[l] = zalloc(self._cat_shape(l, Np), device=dev, dtype=self.dtype)
        for l, p in enumerate(self.packed):
            u = p["u"]
            # the input projection is the step's largest tensor (TGT layer 1: 2.1 GB in f32): written and read once, in bf16 by default
            xproj = torch.empty((T, B, 4 * u), device=dev, dtype=self.rowpar_xproj_dtype)
            ops.gemm_tn(inp.view(N, -1), p["wx_gm"], xproj.view(N, -1), bias=p["bias_gm"])
            h = torch.empty((T, B, u), device=dev, dtype=self.dtype)
            mask = y = None
            if keep_prob < 1.0:
                mask = torch.empty((T, B, u), device=dev, dtype=torch.uint8)
                ops.dropout_mask(mask, keep_prob, seed, row0, l, step_dev)
                y = torch.empty_like(h)
            gates = torch.empty((T, B, 4 * u), device=dev, dtype=self.dtype) if save else None         # this form saves its activations in 16 bits
            c = torch.empty((T, B, u), device=dev)
            hT = yT = None
            if save:
                hT = cats[l][p["ld"]:] if cats[l] is not None else torch.empty((u, Np), device=dev, dtype=self.dtype)
                if Np != N:
                    hT[:, N:].zero_()
                nxt = cats[l + 1] if l + 1 < len(self.packed) else None
                yT = nxt[:u] if nxt is not None else zalloc((u, Np), device=dev, dtype=self.dtype)
            h0 = c0 = None
            if state0 is not None:
                c0, h0 = state0[l][0].float().contiguous(), state0[l][1].to(self.dtype).contiguous()
            if save:                                    # columns [0, B) of h^T = h_{-1}^T (zero, or h0^T); columns [B, T*B) are written by the launch
                if h0 is not None:
                    ops.transpose(h0, hT[:, :B])
                else:
                    hT[:, :B].zero_()
            d = ops.lstm2_fwd_layer(xproj, p["wh_t"], h0, c0, gates, c, h, hT, y, mask, yT=yT, gates_dtype=self.dtype,
                                    xproj_dtype=self.rowpar_xproj_dtype)
            assert h0 is None or plan.fwd[l] != "rowpar"        # (the plan's invariant: the row-parallel recurrence takes no initial state)
            yield (plan.fwd[l] + "_fwd", T, B, d, keep_prob, None if plan.fwd[l] == "resident" else self._rp_workspace(l, T, B, dev))
            out = y if y is not None else h
            if save:
                ctx.append(dict(inp=inp, gates=gates, c=c, h=h, c0=c0, h0=h0, hT=hT, mask=mask, yT=yT,
                                inT=ctx[l - 1]["yT"] if l > 0 else None, persist=True, rowpar=True, catT=cats[l], plan=plan))
            final.append((c[-1], h[-1]))
            inp = out
        return inp, ctx, final

    def _backward_rowpar_co(self, dy, ctx, keep_prob, need_dx=False, need_dstate=False):
        """Top layer first: the layer's whole backward recurrence in one launch (dropout backward of its output folded in; yielded to the
        driver like the forward's), then the gradient wrt its input as one GEMM (dz row-major x Wx), which is the next layer's dh_ext.
        need_dstate (a stack that started from a state): returns (dx, [(dc0, dh0) f32 [B, u]] per layer).  dc0 comes out of the launch
        (d_c . f of step 0); dh0 = dz[0] . Wh^T is one small GEMM over the 16-bit dz[0] the launch has written -- the operands the in-kernel
        contraction of every other step sees."""
        T, B, _ = dy.shape
        dev, N = dy.device, T * B
        Np = ops.round_up(N, 64)
        zalloc = torch.zeros if Np != N else torch.empty
        dh = dy.contiguous()
        st = [None] * len(self.packed)
        for l in range(len(self.packed) - 1, -1, -1):
            p, cx = self.packed[l], ctx[l]
            u = p["u"]
            # dz^T in the K-BLOCKED layout [N/32, 4u, 32] (MNN_GEMM_A_KBLOCK32): a wave's 128 gate columns x 32 rows are one contiguous
            # 8 KB slab (one kilobyte per store instruction) instead of 128 runs of 64 bytes 512 KB apart -- 0.7 us less per timestep on the
            # backward chain, and the GEMM only changes its LDS-DMA source addresses
            kb = self.kblock_wgrads and cx.get("catT") is not None and Np == N and N % 64 == 0
            dzT = torch.empty((N // 32, 4 * u, 32), device=dev, dtype=self.dtype) if kb else zalloc((4 * u, Np), device=dev, dtype=self.dtype)
            want0 = need_dstate and cx.get("c0") is not None
            dzc = torch.empty((T, B, 4 * u), device=dev, dtype=self.dtype) if (l > 0 or (kb and need_dx)) else None
            db_p = self._accum(l, dev)[2]
            e = ops.lstm2_bwd_layer(dh.view(T, B, u), p["wh_p"], cx["gates"], cx["c"], cx.get("c0"), dzc, ops.lstm_seq_bwd_workspace(B, u, dev), dzT, db_p,
                                    cx["mask"] if keep_prob < 1.0 else None, gates_dtype=self.dtype)
            dc0 = torch.empty((B, u), device=dev) if want0 else None
            tail = (dc0,) if want0 else ()
            kind = cx["plan"].bwd[l]                    # the forward's decision (the saved gates are this family's)
            assert cx.get("c0") is None or kind != "rowpar"
            yield (kind + "_bwd", T, B, e, keep_prob, None if kind == "resident" else self._rp_workspace(l, T, B, dev)) + tail
            st[l] = dict(dzT=dzT, dzc=dzc, db_p=db_p, dc0=dc0)
            if want0:
                # dz[0] row-major [B, 4u]: the first slab of the launch's row-major dz where this layer writes one, else read back out of dz^T
                # (step 0 is its first B columns / B / 32 K-blocks: 1 MB, not worth a [T, B, 4u] output of its own -- 1 GB at the bench shape)
                if dzc is not None:
                    dz0 = dzc[0]
                elif kb:
                    dz0 = dzT[:B // 32].permute(0, 2, 1).reshape(B, 4 * u)
                else:
                    dz0 = dzT[:, :B].t().contiguous()
                st[l]["dh0"] = ops.gemm_tn(dz0, p["wh_p"], torch.empty((B, u), device=dev))
            if l > 0:
                dh = torch.empty((N, p["n_in"]), device=dev)
                ops.gemm_tn(dzc.view(N, 4 * u), p["wx_p"], dh)
        self._debug_keep(st)
        keep = [self._weight_grads(l, ctx[l], st[l]["dzT"], st[l]["db_p"], T, B, dz=st[l]["dzc"]) for l in range(len(self.packed) - 1, -1, -1)]
        dx = self._input_grad(st[0]["dzT"], T, B, dz=st[0]["dzc"]) if need_dx else None
        if need_dstate:
            return dx, [(s_["dc0"], s_["dh0"]) if s_["dc0"] is not None else None for s_ in st]
        return dx

    def _workspace(self, T, B, dev):
        """Flags + exchange area of the persistent launches, one per (T, B) (kept alive: captured graphs point at it)."""
        if not hasattr(self, "_pws"):
            self._pws = {}
        if (T, B) not in self._pws:
            self._pws[(T, B)] = ops.lstm2_persist_workspace(T, B, self.packed[0]["u"], self.packed[1]["u"], dev)
        return self._pws[(T, B)]

    def check(self):
        """Raise if a persistent launch ever gave up waiting (synchronises the device)."""
        for (T, B), ws in getattr(self, "_pws", {}).items():
            ops.lstm2_persist_check(ws, B, self.packed[0]["u"], self.packed[1]["u"])
        for ws in getattr(self, "_rpws", {}).values():
            ops.lstm_rowpar_check(ws)

    def forward_co(self, x_tm, keep_prob=1.0, seed=0, row0=0, save=True, state0=None, step_dev=None, state_grad=False):
        """`forward` as a generator function for drive / drive_group, and the one dispatch on the plan: the row-parallel path yields its
        recurrence launches, every other path runs at once."""
        T, B, _ = x_tm.shape
        plan = self.plan(B, T, state0 is not None, state_grad, save)
        if plan.path == "rowpar":
            return (yield from self._forward_rowpar_co(plan, x_tm, keep_prob, seed, row0, save, step_dev, state0))
        body = self._forward_seq if plan.path == "seq" else self._forward_two_layer
        return body(plan, x_tm, keep_prob, seed, row0, save, state0, step_dev)

    def backward_co(self, dy, ctx, keep_prob=1.0, seed=0, row0=0, need_dx=False, step_dev=None, need_dstate=False):
        """`backward` likewise, on the plan the forward saved (the layout of the saved gates is the forward's choice)."""
        plan = ctx[0]["plan"]
        if plan.path == "rowpar":
            return (yield from self._backward_rowpar_co(dy, ctx, keep_prob, need_dx, need_dstate))
        if need_dstate and plan.path == "persist" and ctx[0].get("c0") is not None:
            raise RuntimeError("LstmStack.backward(need_dstate=True): the two-layer persistent form has no state gradient; run the forward with state_grad=True")
        two = plan.path == "persist" or (plan.path == "fused2" and ctx[0]["h0"] is None)
        body = self._backward_two_layer if two and (keep_prob >= 1.0 or ctx[0].get("mask") is not None) else self._backward_seq
        return body(plan, dy, ctx, keep_prob, seed, row0, need_dx, step_dev, need_dstate)

    def forward(self, x_tm, keep_prob=1.0, seed=0, row0=0, save=True, state0=None, step_dev=None, state_grad=False):
        """x_tm [T,B,ld0] compute dtype.  Returns (y [T,B,u_last], ctx, final_state[(c,h)...]).
        state0: [(c0 f32, h0) [B, u]] per layer.  state_grad: the backward will be asked for the gradient wrt state0 (need_dstate): where the
        resident / cluster recurrences do not cover the stack, the launch-per-timestep kernels run (the two-layer persistent form has a
        state input but no state gradient)."""
        return drive(self.forward_co(x_tm, keep_prob, seed, row0, save, state0, step_dev, state_grad))

    def _forward_bufs(self, T, B, dev, keep_prob, save, state0, persist=False):
        """Outputs of the two-layer and launch-per-timestep forms, per layer (f32 projections and gates)."""
        bufs = []
        for l, p in enumerate(self.packed):
            u = p["u"]
            h = torch.empty((T, B, u), device=dev, dtype=self.dtype)
            hT = None
            if save:                        # transposed previous-state operand of dWh, written by the step kernels
                Np = ops.round_up(T * B, 64)            # columns [0,B) = h_{-1} = 0 (or h0), [B, T*B) written by the step kernels
                hT = torch.empty((u, Np), device=dev, dtype=self.dtype)
                hT[:, :B].zero_()
                if Np != T * B:
                    hT[:, T * B:].zero_()
                if state0 is not None:
                    ops.transpose(state0[l][1].to(self.dtype).contiguous(), hT[:, :B])
            bufs.append(dict(xproj=None if (persist and l == 1) else torch.empty((T, B, 4 * u), device=dev), gates=torch.empty((T, B, 4 * u), device=dev) if save else None,
                             c=torch.empty((T, B, u), device=dev), h=h, y=torch.empty_like(h) if keep_prob < 1.0 else h, hT=hT,
                             c0=state0[l][0] if state0 is not None else None,
                             h0=state0[l][1].to(self.dtype) if state0 is not None else None))
        return bufs

    def _forward_result(self, plan, x_tm, bufs, save):
        ctx = []
        if save:
            for l, bf in enumerate(bufs):
                ctx.append(dict(inp=x_tm if l == 0 else bufs[l - 1]["y"], gates=bf["gates"], c=bf["c"], h=bf["h"], c0=bf["c0"], h0=bf["h0"],
                                hT=bf["hT"], mask=bf.get("mask"), yT=bf.get("yT"), inT=bufs[l - 1].get("yT") if l > 0 else None,
                                persist=plan.path == "persist", plan=plan))  # persist: the saved gates are gate-minor -- only the persistent backward reads them
        final = [(bf["c"][-1], bf["h"][-1]) for bf in bufs]
        return bufs[-1]["y"], ctx, final

    def _forward_two_layer(self, plan, x_tm, keep_prob, seed, row0, save, state0, step_dev):
        """persist: ONE launch for the whole recurrence of both layers; fused2: ONE launch per timestep for the whole stack: layer-0 step s |
        layer-1 projection s-1 | layer-1 step s-2."""
        T, B, _ = x_tm.shape
        dev = x_tm.device
        persist = plan.path == "persist"
        bufs = self._forward_bufs(T, B, dev, keep_prob, save, state0, persist)
        (p0, p1), (b0, b1) = self.packed, bufs
        # layer 0's input projection has no dependency: one big GEMM
        if persist:
            ops.gemm_tn(x_tm.view(T * B, -1), p0["wx_gm"], b0["xproj"].view(T * B, -1), bias=p0["bias_gm"])       # gate-minor columns
        else:
            ops.gemm_tn(x_tm.view(T * B, -1), p0["wx_t"], b0["xproj"].view(T * B, -1), bias=p0["bias_p"])
        masks = [None, None]
        if keep_prob < 1.0:
            for l, bf in enumerate(bufs):
                masks[l] = torch.empty(bf["h"].shape, device=dev, dtype=torch.uint8)
                ops.dropout_mask(masks[l], keep_prob, seed, row0, l, step_dev)
        yT = [None, None]
        if persist and save:            # the persistent launch also emits y^T of both layers: no transposes before the weight gradients
            Np = ops.round_up(T * B, 64)
            yT = [(torch.zeros if Np != T * B else torch.empty)((p["u"], Np), device=dev, dtype=self.dtype) for p in self.packed]
        d0 = ops.lstm2_fwd_layer(b0["xproj"], p0["wh_t"], b0["h0"], b0["c0"], b0["gates"], b0["c"], b0["h"], b0["hT"],
                                 b0["y"] if masks[0] is not None else None, masks[0], yT=yT[0])
        d1 = ops.lstm2_fwd_layer(b1["xproj"], p1["wh_t"], b1["h0"], b1["c0"], b1["gates"], b1["c"], b1["h"], b1["hT"],
                                 b1["y"] if masks[1] is not None else None, masks[1], p1["wx_t"], p1["bias_p"], yT=yT[1])
        if persist:
            ops.lstm2_persist_fwd(T, B, d0, d1, keep_prob, self._workspace(T, B, dev))
        else:
            ops.lstm2_seq_fwd(T, B, d0, d1, keep_prob)
        for bf, yt, mk in zip(bufs, yT, masks):
            bf["yT"], bf["mask"] = yt, mk
        return self._forward_result(plan, x_tm, bufs, save)

    def _forward_seq(self, plan, x_tm, keep_prob, seed, row0, save, state0, step_dev):
        """Layer by layer: one projection GEMM over all T*B rows, the recurrence as one launch per timestep, the dropout pass."""
        T, B, _ = x_tm.shape
        bufs = self._forward_bufs(T, B, x_tm.device, keep_prob, save, state0)
        inp = x_tm
        for l, (p, bf) in enumerate(zip(self.packed, bufs)):
            ops.gemm_tn(inp.view(T * B, -1), p["wx_t"], bf["xproj"].view(T * B, -1), bias=p["bias_p"])
            ops.lstm_seq_fwd(bf["xproj"], p["wh_t"], bf["h0"], bf["c0"], bf["gates"], bf["c"], bf["h"], 0, T, bf["hT"])
            if keep_prob < 1.0:
                ops.dropout_fwd(bf["h"], bf["y"], keep_prob, seed, row0, l, step_dev, 0)
            inp = bf["y"]
        return self._forward_result(plan, x_tm, bufs, save)

    @staticmethod
    def _split_k(rows_out, cols_out, K):
        # about 512 workgroups of the 128 x 128 tile (two per CU): every slice adds its tile with f32 atomics, and those run at one
        # chip-wide rate (~1.3 TB/s) -- 16 slices of dWh1 were 67 MB of adds, half of that GEMM's time (profiles/tools/gemm_sweep.py)
        # (at K >= 64 k the adds are a small share again and more slices win: 1024 workgroups)
        # a power of two from 8 up: equal K slices and the XCD-local mapping of id % split_k (the Dense gradient [256 x 704], K = 262144: 64
        # slices 159 us, 85 slices 213 us)
        tiles = -(-rows_out // 128) * -(-cols_out // 128)
        target = 512 if K < 65536 else 1024
        sk = int(max(1, min(target // max(tiles, 1), K // 1024)))
        return 1 << (sk.bit_length() - 1) if sk >= 8 else sk

    # MULTINN_KBLOCK_WGRADS=0: dz^T as a plain [4u, N] matrix instead of the K-blocked layout.  (A third form -- no dz^T at all, the GEMM reading
    # dz row-major through transposing LDS loads -- was measured net-neutral in round 3, profiles/round3_e_kmajor.md, and removed in round 4.)
    kblock_wgrads = flag("MULTINN_KBLOCK_WGRADS")

    def _weight_grads(self, l, cx, dzT, db_p, T, B, dz=None):
        """dWx^T[4u,ld] = dz^T . inp ; dWh^T[4u,u] = dz^T . h_prev  (reduction over the N rows); dzT [4u,Np] and
        h_prev^T come straight from the step kernels, db_p from their epilogue."""
        p = self.packed[l]
        u, ld, n_in = p["u"], p["ld"], p["n_in"]
        N = T * B
        Np = N if dzT.dim() == 3 else dzT.shape[1]
        dev = db_p.device
        inT = cx.get("inT")                 # the producer's own transposed copy (persistent forward: y^T of the layer below)
        cat = cx.get("catT")
        if cat is not None:                 # [x^T ; h_prev^T] in one buffer (h^T is a view of it): one GEMM for both gradients
            if inT is None:
                ops.transpose(cx["inp"].view(N, ld), cat[:ld])
            elif inT.data_ptr() != cat.data_ptr():
                cat[:ld].copy_(inT)
            if not hasattr(self, "_acc_cat"):
                self._acc_cat = {}
            if l not in self._acc_cat:
                self._acc_cat[l] = torch.zeros((4 * u, ld + u), device=dev)
            dw_cat = self._acc_cat[l]
            # one resident round of 256 x 256 tiles (one per CU), the slice count a multiple of 4: measured at [1024 x 768], K = 262144:
            # split 20 400 us, 16 461, 21 669, 24 613, 32 494 (scratch/gemm_merge_probe2.py)
            tiles = -(-4 * u // 256) * -(-(ld + u) // 256)
            sk = max(1, min(256 // tiles // 4 * 4 if 256 // tiles >= 4 else 256 // tiles, Np // 1024))
            if dzT.dim() == 3:              # K-blocked dz^T
                ops.gemm_tn(dzT, cat, dw_cat, accumulate=True, split_k=sk, a_kblock=True)
            else:
                ops.gemm_tn(dzT, cat, dw_cat, accumulate=True, split_k=sk)
            ops.lstm_unpack_grads_cat(dw_cat, db_p, n_in, u, ld, self.store.gviews[f"{self.rnn.prefix}/cell_{l}/kernel"],
                                      self.store.gviews[f"{self.rnn.prefix}/cell_{l}/bias"])
            return (cat, dw_cat)
        if inT is None:
            inT = (torch.zeros if Np != N else torch.empty)((ld, Np), device=dev, dtype=self.dtype)
            ops.transpose(cx["inp"].view(N, ld), inT)
        # dwx_t / dwh_t / db_p are persistent accumulators (zero between steps: the unpack below clears what it reads), so the
        # split-K slices add into them without a zero-fill launch in front of every GEMM
        dwx_t, dwh_t, _ = self._accum(l, dev)
        ops.gemm_tn(dzT, inT, dwx_t, accumulate=True, split_k=self._split_k(4 * u, ld, Np))
        ops.gemm_tn(dzT, cx["hT"], dwh_t, accumulate=True, split_k=self._split_k(4 * u, u, Np))
        ops.lstm_unpack_grads(dwx_t, dwh_t, db_p, n_in, u, self.store.gviews[f"{self.rnn.prefix}/cell_{l}/kernel"],
                              self.store.gviews[f"{self.rnn.prefix}/cell_{l}/bias"], consume=True)
        return (inT, dwx_t, dwh_t)      # kept alive until the streams are joined

    def _accum(self, l, dev):
        """Packed weight-gradient accumulators of layer l: (dWx^T [4u, ld], dWh^T [4u, u], db [4u]) f32, allocated zeroed once."""
        if not hasattr(self, "_acc"):
            self._acc = {}
        if l not in self._acc:
            p = self.packed[l]
            self._acc[l] = (torch.zeros((4 * p["u"], p["ld"]), device=dev), torch.zeros((4 * p["u"], p["u"]), device=dev),
                            torch.zeros(4 * p["u"], device=dev))
        return self._acc[l]

    def backward(self, dy, ctx, keep_prob=1.0, seed=0, row0=0, need_dx=False, step_dev=None, need_dstate=False):
        """dy f32 [T,B,u_last]: gradient wrt the (dropped) top output.  Accumulates the kernel / bias gradients
        into the store's flat gradient buffer.
        need_dstate: returns (dx, [(dc0, dh0) f32 [B, u]] per layer), the gradient wrt the forward's state0 (None for a layer without one)."""
        return drive(self.backward_co(dy, ctx, keep_prob, seed, row0, need_dx, step_dev, need_dstate))

    def _backward_bufs(self, dy, ctx, keep_prob, need_dstate, persist):
        """Outputs of the two-layer and launch-per-timestep backward forms: (per-layer dict, per-layer gradient wrt the layer's output)."""
        T, B, _ = dy.shape
        dev = dy.device
        L = len(self.packed)
        dyl = [None] * L
        dyl[L - 1] = dy.view(T, B, -1)
        st = []
        Np = ops.round_up(T * B, 64)
        for l, p in enumerate(self.packed):
            u = p["u"]
            fused = ops.lstm_fused_outputs(self.dtype, u)          # bf16 step kernels emit dz^T and sum(dz) themselves
            dz = None if fused else torch.empty((T, B, 4 * u), device=dev)
            st.append(dict(dz=dz, dzc=None if persist else (dz if self.dtype == torch.float32 else torch.empty((T, B, 4 * u), device=dev, dtype=self.dtype)),
                           dzT=(torch.zeros if Np != T * B else torch.empty)((4 * u, Np), device=dev, dtype=self.dtype),
                           db_p=self._accum(l, dev)[2],
                           dh=torch.empty((T, B, u), device=dev) if (keep_prob < 1.0 and not (persist and ctx[l].get("mask") is not None)) else None,
                           ws=ops.lstm_seq_bwd_workspace(B, u, dev)))
            if need_dstate and ctx[l].get("c0") is not None:
                st[-1]["dh0"], st[-1]["dc0"] = torch.empty((B, u), device=dev), torch.empty((B, u), device=dev)
            if l < L - 1 and not persist:
                dyl[l] = torch.empty((T, B, u), device=dev)
        return st, dyl

    def _backward_result(self, st, ctx, T, B, need_dx, need_dstate):
        """Weight gradients (top layer first), the input gradient, the state gradients."""
        self._debug_keep(st)
        keep = [self._weight_grads(l, ctx[l], st[l]["dzT"], st[l]["db_p"], T, B) for l in range(len(self.packed) - 1, -1, -1)]
        dx = self._input_grad(st[0]["dzT"], T, B) if need_dx else None
        if need_dstate:
            return dx, [(s_["dc0"], s_["dh0"]) if "dc0" in s_ else None for s_ in st]
        return dx

    def _debug_keep(self, st):
        if getattr(self, "keep_debug", False):      # tests: the recurrence's own (atomic-free, hence run-to-run bit-stable) outputs
            self._dbg_dzT = [s_["dzT"] for s_ in st]

    def _backward_two_layer(self, plan, dy, ctx, keep_prob, seed, row0, need_dx, step_dev, need_dstate):
        """Both layers' backward recurrences in one launch (persist) or one launch per timestep (fused2)."""
        T, B, _ = dy.shape
        persist = plan.path == "persist"
        st, dyl = self._backward_bufs(dy, ctx, keep_prob, need_dstate, persist)
        p0, p1 = self.packed
        fold = persist and keep_prob < 1.0 and ctx[1].get("mask") is not None    # the persistent backward applies layer 2's mask itself
        if keep_prob < 1.0 and not fold:
            ops.dropout_bwd(dyl[1], st[1]["dh"], keep_prob, seed, row0, 1, False, step_dev, 0)
        dh1 = st[1]["dh"] if (keep_prob < 1.0 and not fold) else dyl[1]
        dh0 = None if persist else dyl[0]              # written by the fused launches (stage Q), dropout already applied
        e0 = ops.lstm2_bwd_layer(dh0, p0["wh_p"], ctx[0]["gates"], ctx[0]["c"], ctx[0]["c0"], st[0]["dzc"], st[0]["ws"], st[0]["dzT"], st[0]["db_p"],
                                 ctx[0].get("mask"))
        e1 = ops.lstm2_bwd_layer(dh1, p1["wh_p"], ctx[1]["gates"], ctx[1]["c"], ctx[1]["c0"], st[1]["dzc"], st[1]["ws"], st[1]["dzT"], st[1]["db_p"],
                                 ctx[1]["mask"] if fold else None, p1["wx_p"])
        if persist:
            ops.lstm2_persist_bwd(T, B, e0, e1, keep_prob, self._workspace(T, B, dy.device))
        else:
            ops.lstm2_seq_bwd(T, B, e0, e1, keep_prob)
        return self._backward_result(st, ctx, T, B, need_dx, need_dstate)

    def _backward_seq(self, plan, dy, ctx, keep_prob, seed, row0, need_dx, step_dev, need_dstate):
        """Top layer first: the dropout backward, the recurrence as one launch per timestep, then the gradient wrt the layer's input as one
        GEMM over all T*B rows."""
        T, B, _ = dy.shape
        st, dyl = self._backward_bufs(dy, ctx, keep_prob, need_dstate, plan.path == "persist")
        for l in range(len(self.packed) - 1, -1, -1):
            p, cx, s_ = self.packed[l], ctx[l], st[l]
            if keep_prob < 1.0:
                ops.dropout_bwd(dyl[l], s_["dh"], keep_prob, seed, row0, l, False, step_dev, 0)
                dh = s_["dh"]
            else:
                dh = dyl[l]
            ops.lstm_seq_bwd(dh, p["wh_p"], cx["gates"], cx["c"], cx["c0"], s_["dz"], s_["dzc"], s_.get("dh0"), s_.get("dc0"), 0, T, s_["ws"],
                             s_["dzT"], s_["db_p"])
            if l > 0:
                ops.gemm_tn(s_["dzc"].view(T * B, -1), p["wx_p"], dyl[l - 1].view(T * B, -1))
        return self._backward_result(st, ctx, T, B, need_dx, need_dstate)

    def _input_grad(self, dzT0, T, B, dz=None):
        """Gradient wrt the stack's inputs, f32 [T,B,n_in] = dz_0 . Wx_0^T (only the feedback modes consume it: the feedback vector is part of
        every per-track generator's input, multinn_feedback.py:85-91).  Every form of the recurrence leaves layer 0's dz as dz^T [4u, N]
        (the weight-gradient operand): one transpose pass makes the K-contiguous A operand."""
        p = self.packed[0]
        N = T * B
        if p.get("wx_p0") is None:          # [ld0, 4u]: the packed (gate-interleaved) input weights with K = 4u contiguous, once per pack
            p["wx_p0"] = torch.empty((p["ld"], 4 * p["u"]), device=p["wx_t"].device, dtype=self.dtype)
            ops.transpose(p["wx_t"], p["wx_p0"])
        if dzT0.dim() == 3:
            dz = dz.view(N, 4 * p["u"])
        else:
            dz = torch.empty((N, 4 * p["u"]), device=dzT0.device, dtype=self.dtype)
            ops.transpose(dzT0[:, :N], dz)
        dx = torch.empty((N, p["n_in"]), device=dz.device)
        ops.gemm_tn(dz, p["wx_p0"][:p["n_in"]], dx)
        return dx.view(T, B, p["n_in"])

    def single_step(self, x, state):
        """One time step (rnn_nade.py:268): x [B,ld0] compute dtype, state [(c,h)...] -> (h_top, new_state)."""
        y, _, final = self.forward(x.view(1, *x.shape), 1.0, save=False, state0=state)
        return y[0], [(c, h) for c, h in final]

    # -- deterministic f32 single steps (csrc/det_step.hip): the arithmetic of every sampling scan -----------------------------------
    owner = None          # weakref to the estimator this stack belongs to (its pack epoch dates the repacked weights below)
    _det_pack, _det_pack_key = None, None

    def det_job(self, l, x, n_x, x2, st):
        """Descriptor of layer l's deterministic step (ops.lstm_step_det) with fresh f32 outputs.  The master weights are read through their
        repacked copy (ops.det_lstm_pack: the same numbers in the kernel's load order), remade when the weights may have changed: a new
        store.step or a new pack epoch of the owner -- once per sampling scan, inside its graph."""
        u = self.rnn.num_units[l]
        ref = x if x is not None else x2
        c = torch.empty((ref.shape[0], u), device=ref.device)
        h = torch.empty_like(c)
        pre = self.rnn.prefix
        key = (self.store.step, getattr(self.owner() if self.owner is not None else None, "_pack_epoch", 0))
        if self._det_pack is None or self._det_pack_key != key:
            self._det_pack = [ops.det_lstm_pack(self.store[f"{pre}/cell_{k}/kernel"], self.rnn.num_units[k]) for k in range(len(self.rnn.num_units))]
            self._det_pack_key = key
        return dict(x=x, n_x=n_x, x2=x2, h_prev=None if st is None else st[1], c_prev=None if st is None else st[0],
                    W=self.store[f"{pre}/cell_{l}/kernel"], Wp=self._det_pack[l], bias=self.store[f"{pre}/cell_{l}/bias"], c_out=c, h_out=h)

    def det_step(self, x, state, x2=None, lengths=None, t=0):
        """One deterministic f32 step of the stack: x u8 | f32 [B, n_x] (unit inner stride), optional x2 f32 [B, n_x2] concatenated behind
        it; state [(c, h)...] f32 or None (zero state) -> (h_top f32 [B, u_last], new_state).  lengths (int32 [B] on the device), t: step t
        of ragged prompts -- a row with t >= lengths[row] keeps its state (ops.lstm_step_det)."""
        return det_steps([self], [x], [state], [x2], lengths=lengths, t=t)[0]


def _det_f32(t):
    return t if t is None or t.dtype == torch.float32 else t.float()


def det_steps(stacks, xs, states, x2s=None, lengths=None, t=0):
    """One deterministic step of several LSTM stacks of equal depth (the M per-track generators of a feedback-scan step): layer by layer,
    the stacks' jobs of a layer run as ONE launch.  Returns [(h_top, new_state)] per stack.  lengths, t (optional): step t of ragged
    prompts, for every layer's launch (ops.lstm_step_det)."""
    n = len(stacks)
    x2s = x2s if x2s is not None else [None] * n
    L = len(stacks[0].rnn.num_units)
    assert all(len(s.rnn.num_units) == L for s in stacks)
    inp, inp2 = list(xs), list(x2s)
    new = [[] for _ in range(n)]
    for l in range(L):
        jobs = []
        for i, s in enumerate(stacks):
            x = inp[i]
            if x is not None and x.dtype not in (torch.uint8, torch.float32):
                x = x.float()
            st = None if states[i] is None else (_det_f32(states[i][l][0]).contiguous(), _det_f32(states[i][l][1]).contiguous())
            n_x = s.rnn.layer_inputs()[l] - (inp2[i].shape[1] if inp2[i] is not None else 0)
            jobs.append(s.det_job(l, x, n_x, inp2[i], st))
        if lengths is None:
            ops.lstm_step_det(jobs)
        else:
            ops.lstm_step_det(jobs, lengths=lengths, t=t)
        for i, j in enumerate(jobs):
            new[i].append((j["c_out"], j["h_out"]))
            inp[i], inp2[i] = j["h_out"], None
    return [(inp[i], new[i]) for i in range(n)]
