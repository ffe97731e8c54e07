"""float64 restatement of one LSTM layer's recurrence (rnn.py:104-145) in the layout of the single-layer persistent kernels
(lstm_resident.hip, lstm_cluster.hip, lstm_rowpar.hip): the reference their element-by-element tests share.

TEST INFRASTRUCTURE ONLY.  Layout (DESIGN.md "LSTM layout"): gate order i, g, f, o; the 4u gate columns are interleaved in blocks of 32 units
(`gate_perm`); `wh_t` is [gate-interleaved row][k] (z[n] += sum_k h[k] wh_t[n][k]); the input projection is gate-minor [T, B, u, 4] with the
bias included.  A kernel feeds back 16-bit values -- the rounded h forward, the rounded dz backward -- so a test hands those in through
`feedback`; without it the reference feeds back its own unrounded state (tests/test_lstm_float64_cpu.py pins that form on oracle/lstm.py)."""
import numpy as np


def gate_perm(u):
    """natural TF column g * u + unit -> (unit / 32) * 128 + g * 32 + unit % 32 (DESIGN.md "LSTM layout")"""
    unit = np.arange(u)
    return np.stack([(unit >> 5) * 128 + g * 32 + (unit & 31) for g in range(4)])        # [gate][unit]


def _sig(a):
    return 1.0 / (1.0 + np.exp(-a))


def forward(W, X, feedback=None, h0=None, c0=None):
    """W: wh_t [4u, u], X: xproj [T, B, u, 4], both float64.  feedback(t, h_t) -> the state step t + 1 reads (None: h_t itself).
    h0 / c0: the state step 0 starts from, [B, u] float64 (None: zeros).
    Returns dict(g = activations [T, B, u, 4], c [T, B, u], h [T, B, u])."""
    T, B, u, _ = X.shape
    perm = gate_perm(u)
    hp = np.zeros((B, u)) if h0 is None else np.asarray(h0, np.float64)
    cp = np.zeros((B, u)) if c0 is None else np.asarray(c0, np.float64)
    ref = dict(g=np.zeros((T, B, u, 4)), c=np.zeros((T, B, u)), h=np.zeros((T, B, u)))
    for t in range(T):
        z = np.stack([X[t, :, :, g] + hp @ W[perm[g]].T for g in range(4)], -1)     # [B, u, 4]
        gi, gg, gf, go = _sig(z[..., 0]), np.tanh(z[..., 1]), _sig(z[..., 2]), _sig(z[..., 3])
        cp = gg * gi + cp * gf
        hv = np.tanh(cp) * go
        ref["g"][t] = np.stack([gi, gg, gf, go], -1)
        ref["c"][t] = cp
        ref["h"][t] = hv
        hp = hv if feedback is None else feedback(t, hv)
    return ref


def backward(W, Gs, Cs, dh, mask=None, keep=1.0, feedback=None, c0=None):
    """W: wh_t [4u, u]; Gs: saved activations [T, B, u, 4]; Cs: saved cell states [T, B, u]; dh: external gradient of the layer's output
    [T, B, u] (of y = h / keep * mask when a keep mask [T, B, u] is given), all float64.  feedback(t, dz_t) -> the dz[t] step t - 1 reads
    (None: dz_t itself).  c0: the initial cell state [B, u] the forward started from (None: zeros) -- c[t - 1] of step 0.  Returns dz [T, B, 4u]: pre-activation gradients in gate-interleaved columns."""
    T, B, u = Cs.shape
    perm = gate_perm(u)
    dz_ref = np.zeros((T, B, 4 * u))
    dcv, dz_next = np.zeros((B, u)), np.zeros((B, 4 * u))
    for t in range(T - 1, -1, -1):
        gi, gg, gf, go = (Gs[t, :, :, k] for k in range(4))
        dhv = dh[t] * (mask[t] / keep if mask is not None else 1.0) + dz_next @ W      # sum_n dz[n] W[n][k]
        tc = np.tanh(Cs[t])
        d_o = dhv * tc
        d_c = dhv * go * (1 - tc * tc) + dcv
        cprev = Cs[t - 1] if t > 0 else (np.zeros((B, u)) if c0 is None else np.asarray(c0, np.float64))
        dzs = [d_c * gg * gi * (1 - gi), d_c * gi * (1 - gg * gg), d_c * cprev * gf * (1 - gf), d_o * go * (1 - go)]
        dcv = d_c * gf
        for g in range(4):
            dz_ref[t][:, perm[g]] = dzs[g]
        dz_next = dz_ref[t] if feedback is None else feedback(t, dz_ref[t])
    return dz_ref
