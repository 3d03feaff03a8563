"""float64 restatement of the ResGNN training step with the Fourier filter
(lib/graph_conv.py::residual_network :305-330 with ``filter = 'fourier'``,
:83-111), plain and stacked (``_inference`` with stack_num > 1, :272-303).

TEST HELPER ONLY.  It composes oracle.fourier_oracle (the filter and its
autodiff), oracle.model_oracle.loss_and_grad / ema_update and
oracle.cheb_oracle.adam_step; the wiring is model_oracle.forward / backward's
with the filter swapped.  U is always GIVEN: the model's own float32 U cast to
float64, never a recomputed EVD (grid graphs have degenerate eigenvalues, so
two decompositions need not agree on the eigenvectors).

Spectra are kept as fourier_oracle returns them, [N, Fin, M];
``spectrum_nmc`` gives the sample-major [N, M, Fin] of the device path.
"""
from __future__ import annotations

import numpy as np

from oracle import cheb_oracle as O
from oracle import fourier_oracle as FO
from oracle import model_oracle as MO


def r32(a):
    """float32 values held as float64."""
    return np.asarray(a, np.float32).astype(np.float64)


def spectrum_nmc(xhat):
    return np.ascontiguousarray(np.transpose(xhat, (0, 2, 1)))


def filter_forward(x, W, U, residual=None, act="none"):
    """(y = act(fourier(x; W) + residual), xhat [N, Fin, M])."""
    y, xhat = FO.fourier_forward(x, W, U)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return (np.maximum(y, 0.0) if act == "relu" else y), xhat


def filter_backward(dy, y, act, W, U, xhat, mask=None):
    """(dx, dW, dz): dz = dy * [y > 0] for act relu (``mask`` replaces [y > 0]),
    then fourier_oracle.fourier_backward of dz."""
    dy = np.asarray(dy, np.float64)
    if act == "relu":
        dz = dy * ((np.asarray(y) > 0) if mask is None else mask)
    else:
        dz = dy
    dx, dW = FO.fourier_backward(dz, W, U, xhat)
    return dx, dW, dz


def forward(x, Ws, U, R):
    """Ws: [W_init, (W_i0, W_i1) * R, W_N], each [M, Fout, Fin].
    Returns (out, cache); cache[li] = (input, xhat, output, act)."""
    cache = []

    def f(inp, W, res, act):
        out, xhat = filter_forward(inp, W, U, res, act)
        cache.append((inp, xhat, out, act))
        return out

    h = f(np.asarray(x, np.float64), Ws[0], None, "relu")
    li = 1
    for _ in range(R):
        t = f(h, Ws[li], None, "relu")
        h = f(t, Ws[li + 1], h, "relu")
        li += 2
    return f(h, Ws[li], None, "none"), cache


def backward(dout, cache, Ws, U, R, masks=None):
    """The list of dW in the order of Ws.  masks[li] (optional, boolean or None)
    replaces filter li's own ReLU mask [out > 0]."""
    dWs = [None] * len(Ws)

    def b(li, dy):
        _, xhat, out, act = cache[li]
        m = None if masks is None else masks[li]
        dx, dW, dz = filter_backward(dy, out, act, Ws[li], U, xhat, m)
        dWs[li] = dW
        return dx, dz

    last = len(Ws) - 1
    dh, _ = b(last, dout)
    li = last - 2
    for _ in range(R):
        dt, dz1 = b(li + 1, dh)
        dx0, _ = b(li, dt)
        dh = dx0 + dz1
        li -= 2
    b(0, dh)
    return dWs


def loss(x, labels, Ws, U, R):
    return MO.loss_and_grad(forward(x, Ws, U, R)[0], labels)[0]


def _adam(flat_W, flat_g, adam_state, step, lr):
    new_W, new_state = [], []
    for W, g, (m, v) in zip(flat_W, flat_g, adam_state):
        W2, m2, v2 = O.adam_step(W, g, m, v, step, lr=lr)
        new_W.append(W2)
        new_state.append((m2, v2))
    return new_W, new_state


def train_step(x, labels, Ws, U, R, adam_state, step, lr):
    """One step: (loss, dWs, new Ws, new adam_state)."""
    out, cache = forward(x, Ws, U, R)
    l, dout = MO.loss_and_grad(out, labels)
    dWs = backward(dout, cache, Ws, U, R)
    new_W, new_state = _adam(Ws, dWs, adam_state, step, lr)
    return l, dWs, new_W, new_state


# ---- stacked input (lib/graph_conv.py:272-303) ------------------------------------------
def stacked_forward(x, nets, merge_Ws, groups, U, R):
    """X = sum_i relu(net_i(x[..., a_i:b_i])) * w_i; returns (X, [(out_i, cache_i)])."""
    X, caches = None, []
    for (a, b), Ws, w in zip(groups, nets, merge_Ws):
        out, cache = forward(np.asarray(x, np.float64)[..., a:b], Ws, U, R)
        x1 = np.maximum(out, 0)
        X = x1 * w if X is None else X + x1 * w
        caches.append((out, cache))
    return X, caches


def stacked_backward(dX, caches, nets, merge_Ws, U, R, masks=None, out_masks=None):
    """(dWs per network, dw per merge weight).  masks[i][li] / out_masks[i]
    (optional) replace the ReLU masks of network i's filters / of its output."""
    dnets, dws = [], []
    for i, ((out, cache), Ws, w) in enumerate(zip(caches, nets, merge_Ws)):
        dws.append(np.sum(dX * np.maximum(out, 0), axis=0))
        om = (out > 0) if out_masks is None else out_masks[i]
        dnets.append(backward(dX * w * om, cache, Ws, U, R, None if masks is None else masks[i]))
    return dnets, dws


def stacked_flat(nets, merge):
    """The trainer's variable order: net_0 weights, w_0, net_1 weights, w_1, ..."""
    flat = []
    for Ws, w in zip(nets, merge):
        flat += list(Ws) + [w]
    return flat


def stacked_unflat(flat, nets):
    new_nets, new_merge, i = [], [], 0
    for Ws in nets:
        new_nets.append(flat[i:i + len(Ws)])
        new_merge.append(flat[i + len(Ws)])
        i += len(Ws) + 1
    return new_nets, new_merge


def stacked_loss(x, labels, nets, merge_Ws, groups, U, R):
    return MO.loss_and_grad(stacked_forward(x, nets, merge_Ws, groups, U, R)[0], labels)[0]


def stacked_train_step(x, labels, nets, merge_Ws, groups, U, R, adam_state, step, lr):
    """One step; adam_state in stacked_flat's order.  Returns (loss, grads in
    that order, new nets, new merge_Ws, new adam_state)."""
    X, caches = stacked_forward(x, nets, merge_Ws, groups, U, R)
    l, dX = MO.loss_and_grad(X, labels)
    dnets, dws = stacked_backward(dX, caches, nets, merge_Ws, U, R)
    flat_g = stacked_flat(dnets, dws)
    new_flat, new_state = _adam(stacked_flat(nets, merge_Ws), flat_g, adam_state, step, lr)
    new_nets, new_merge = stacked_unflat(new_flat, nets)
    return l, flat_g, new_nets, new_merge, new_state
