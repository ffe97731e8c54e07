"""float64 restatement of what the two-layer persistent recurrence (csrc/lstm_persist.hip) computes, layer by layer on tests/lstm_float64.py and
on the kernel's own 16-bit operands: the reference of tests/test_gpu_persist_kernels.py.

TEST INFRASTRUCTURE ONLY.  Everything is float64 numpy.  What the kernel hands from one workgroup to another is a 16-bit tile, so each layer's
reference is fed the kernel's stored 16-bit values at exactly those points:
    layer 1 forward    z = xproj1[t] (gate-minor, bias included) + h1[t-1] . Wh1^T          feedback: the kernel's h1[t]
    layer 2 forward    z = bias_p2 + out1[t] . Wx2^T + h2[t-1] . Wh2^T                       out1: the kernel's stored y1 (h1 without a mask);
                                                                                             feedback: the kernel's h2[t]
    layer 2 backward   dh = dh_ext[t] (x mask2 / keep when the mask is folded) + dz2[t+1] . Wh2   feedback: the kernel's dz2[t]
    layer 1 backward   dh = (dz2[t] . Wx2) x mask1 / keep + dz1[t+1] . Wh1                   on the kernel's dz2; feedback: the kernel's dz1[t]
`wx_t2` [4 u2, u1] and `bias_p2` [4 u2] are gate-interleaved (lstm_float64.gate_perm); an error of one layer therefore never leaks into the
reference of the other, and every compared element is one step of arithmetic away from values both sides share."""
import numpy as np

import lstm_float64 as L64


def layer2_xproj(out1, wx_t2, bias_p2):
    """out1 [T, B, u1] -> layer 2's input projection, gate-minor [T, B, u2, 4]."""
    u2 = wx_t2.shape[0] // 4
    perm = L64.gate_perm(u2)
    return np.stack([out1 @ wx_t2[perm[g]].T + bias_p2[perm[g]] for g in range(4)], -1)


def forward(wh_t1, xproj1, h1k, out1k, wh_t2, wx_t2, bias_p2, h2k, state1=(None, None), state2=(None, None)):
    """xproj1 [T, B, u1, 4]; h1k / h2k: the kernel's stored h of either layer; out1k: the kernel's stored output of layer 1 (y1, or h1 without
    a mask); state = (h0, c0), each [B, u] or None.  Returns (ref1, ref2), the dicts of lstm_float64.forward."""
    ref1 = L64.forward(wh_t1, xproj1, lambda t, hv: h1k[t], h0=state1[0], c0=state1[1])
    ref2 = L64.forward(wh_t2, layer2_xproj(out1k, wx_t2, bias_p2), lambda t, hv: h2k[t], h0=state2[0], c0=state2[1])
    return ref1, ref2


def backward(wh_t1, g1k, c1k, dz1k, mask1, wh_t2, wx_t2, g2k, c2k, dz2k, dh_ext, mask2, keep, c0_1=None, c0_2=None):
    """g / c: the kernel's saved activations [T, B, u, 4] and cell states; dz1k / dz2k: the kernel's stored 16-bit dz [T, B, 4u]; dh_ext: what the
    caller hands layer 2; mask2: layer 2's keep mask when the launch folds its dropout backward (None: dh_ext is the gradient of h2).
    Returns (dz1_ref, dz2_ref), gate-interleaved [T, B, 4u]."""
    dz2 = L64.backward(wh_t2, g2k, c2k, dh_ext, mask2, keep, lambda t, dz: dz2k[t], c0=c0_2)
    dh1 = dz2k @ wx_t2                                   # dz2 . wx_p2^T with wx_p2 = wx_t2^T: [T, B, 4 u2] x [4 u2, u1]
    dz1 = L64.backward(wh_t1, g1k, c1k, dh1, mask1, keep, lambda t, dz: dz1k[t], c0=c0_1)
    return dz1, dz2
