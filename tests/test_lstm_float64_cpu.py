"""tests/lstm_float64.py -- the float64 reference of the resident / cluster / row-parallel kernel tests -- pinned on oracle/lstm.py: with its own
unrounded state fed back and operands built from a natural-layout W, b and x, its forward (h, c, gates) and its backward (dz, and through dz
the weight, bias and input gradients) are seq_fwd / seq_bwd to 1e-12 relative.  No device."""
import numpy as np
import pytest

import lstm_float64 as L64
from oracle import lstm as olstm


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max())


def test_gate_perm_is_the_interleaved_layout():
    for u in (32, 128, 512):
        perm = L64.gate_perm(u)
        assert perm.shape == (4, u) and sorted(perm.ravel().tolist()) == list(range(4 * u))
        assert perm[2, 37 % u] == ((37 % u) // 32) * 128 + 2 * 32 + (37 % u) % 32


@pytest.mark.parametrize("keep", [1.0, 0.9])
@pytest.mark.parametrize("u", [32, 128])
def test_float64_reference_equals_the_oracle(u, keep):
    _compare_with_the_oracle(u, keep, None)


@pytest.mark.parametrize("keep", [1.0, 0.9])
@pytest.mark.parametrize("state", ["h0c0", "c0"])
def test_float64_reference_with_initial_state_equals_the_oracle(state, keep):
    """The stateful form: seq_fwd(init_state=[(c0, h0)]) / seq_bwd against forward(h0=, c0=) / backward(c0=) to the same 1e-12 --
    "h0c0": both given; "c0": a cell state alone (h0 = None here, zeros in the oracle)."""
    _compare_with_the_oracle(32, keep, state)


def _compare_with_the_oracle(u, keep, state):
    T, B, n_in = 4, 5, 7
    rng = np.random.default_rng(5 + u)
    W = rng.normal(0, 0.3, (n_in + u, 4 * u))               # natural layout: rows [x ; h], column blocks i | g | f | o
    b = rng.normal(0, 0.2, 4 * u)
    x = rng.normal(0, 1.0, (B, T, n_in))
    drop_u = [rng.random((B, T, u)).astype(np.float32)] if keep < 1.0 else None
    h0 = c0 = None
    if state is not None:                                    # drawn last: the stateless cases keep the operands they always had
        srng = np.random.default_rng(77 + u)
        c0 = srng.normal(0, 0.7, (B, u))
        h0 = np.tanh(srng.normal(0, 0.7, (B, u))) if state == "h0c0" else None
    init = None if state is None else [(c0, h0 if h0 is not None else np.zeros((B, u)))]
    y, final, cache = olstm.seq_fwd(x, [(W, b)], keep, drop_u, init_state=init)
    perm = L64.gate_perm(u)
    wh_t = np.zeros((4 * u, u))
    for g in range(4):
        wh_t[perm[g]] = W[n_in:, g * u:(g + 1) * u].T
    xp = x @ W[:n_in] + b                                    # [B, T, 4u], natural columns
    X = np.ascontiguousarray(xp.reshape(B, T, 4, u).transpose(1, 0, 3, 2))      # gate-minor [T, B, u, 4]
    ref = L64.forward(wh_t, X, h0=h0, c0=c0)
    tol = 1e-12
    assert rel(ref["c"][-1], final[0][0]) < tol and rel(ref["h"][-1], final[0][1]) < tol
    if state is not None:
        assert not np.allclose(ref["h"][0], L64.forward(wh_t, X, c0=None, h0=h0)["h"][0])        # c0 reaches step 0 ...
        assert h0 is None or not np.allclose(ref["h"][0], L64.forward(wh_t, X, c0=c0)["h"][0])    # ... and so does h0
    for t in range(T):
        assert rel(ref["h"][t], cache["h"][0][t]) < tol and rel(ref["c"][t], cache["c"][0][t]) < tol
        for g in range(4):
            assert rel(ref["g"][t][:, :, g], cache["gates"][0][t][g]) < tol
    mask = np.stack([cache["keep"][0][t] for t in range(T)]) if keep < 1.0 else None
    if mask is not None:
        assert 0 < mask.mean() < 1 and rel(ref["h"].transpose(1, 0, 2) / keep * mask.transpose(1, 0, 2), y) < tol
    dy = rng.normal(0, 0.5, (B, T, u))
    dx, grads = olstm.seq_bwd(dy, cache)
    dz = L64.backward(wh_t, ref["g"], ref["c"], np.ascontiguousarray(dy.transpose(1, 0, 2)), mask, keep, c0=c0)
    if state is not None:       # c0 is c[t - 1] of step 0: without it the forget gate's dz[0] is zero
        dz_no = L64.backward(wh_t, ref["g"], ref["c"], np.ascontiguousarray(dy.transpose(1, 0, 2)), mask, keep)
        assert np.array_equal(dz_no[1:], dz[1:]) and not dz_no[0][:, perm[2]].any() and dz[0][:, perm[2]].any()
    dzn = np.concatenate([dz[:, :, perm[g]] for g in range(4)], -1)              # back to natural columns [T, B, 4u]
    dW, db = np.zeros_like(W), np.zeros_like(b)
    for t in range(T):
        hprev = ref["h"][t - 1] if t > 0 else (np.zeros((B, u)) if h0 is None else h0)
        dW += np.concatenate([x[:, t], hprev], 1).T @ dzn[t]
        db += dzn[t].sum(0)
    assert rel(dW, grads[0][0]) < tol and rel(db, grads[0][1]) < tol
    assert rel((dzn @ W[:n_in].T).transpose(1, 0, 2), dx) < tol
    # ... and the feedback hooks see every step once, in order, and replace what is fed back
    seen = []
    ref2 = L64.forward(wh_t, X, feedback=lambda t, hv: (seen.append(t), np.zeros_like(hv))[1], h0=h0, c0=c0)
    assert seen == list(range(T)) and rel(ref2["h"][0], ref["h"][0]) < tol and not np.allclose(ref2["h"][1], ref["h"][1])
    seen = []
    dz2 = L64.backward(wh_t, ref["g"], ref["c"], np.ascontiguousarray(dy.transpose(1, 0, 2)), mask, keep,
                       feedback=lambda t, d: (seen.append(t), np.zeros_like(d))[1], c0=c0)
    assert seen == list(range(T - 1, -1, -1)) and rel(dz2[T - 1], dz[T - 1]) < tol and not np.allclose(dz2[0], dz[0])
