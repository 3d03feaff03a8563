"""Float64 reference of ``lib/gconvRNN.py::Model`` (model_type='glstm'), not a
test module: the per-step head (:306-317), the vertex softmax cross-entropy as
the code executes it (:326-332), their backward, and the whole model on top of
oracle/lstm_oracle.py's cell with the standard tanh / sigmoid gates.

  logits[t, n, m] = hd[t, n, m, :] . w + b                  w [H], b scalar
  ce[t, n]        = logsumexp_m logits[t, n, :] - logits[t, n, labels[t, n]]
  loss            = loss_scale * sum_{t, n} ce              loss_scale = 1 / T

``reduce_sum(losses, axis=1)`` on the list of T [N] tensors sums over the batch
and ``reduce_mean`` then averages over time, so the executed loss is
(1/T) sum_t sum_n ce -- ``loss_as_named`` is the batch mean the variable name
promises, kept here only to show the two differ.
"""
import numpy as np

from oracle import lstm_oracle as LO


def head_forward(hd, w, b, labels, loss_scale):
    """hd [T, N, M, H] (already through the dropout mask), labels [T, N].
    Returns (logits [T, N, M], ce [T, N], loss)."""
    hd, w = np.asarray(hd, np.float64), np.asarray(w, np.float64).reshape(-1)
    logits = hd @ w + float(np.asarray(b).reshape(-1)[0])
    mx = logits.max(axis=-1, keepdims=True)
    lse = mx[..., 0] + np.log(np.exp(logits - mx).sum(axis=-1))
    picked = np.take_along_axis(logits, np.asarray(labels)[..., None], axis=-1)[..., 0]
    ce = lse - picked
    return logits, ce, loss_scale * ce.sum()


def head_backward(hd, w, logits, labels, loss_scale):
    """Gradient of head_forward's loss: (dlogit [T, N, M], dhd, dw [H], db)."""
    hd, w = np.asarray(hd, np.float64), np.asarray(w, np.float64).reshape(-1)
    mx = logits.max(axis=-1, keepdims=True)
    e = np.exp(logits - mx)
    p = e / e.sum(axis=-1, keepdims=True)
    onehot = np.zeros_like(p)
    np.put_along_axis(onehot, np.asarray(labels)[..., None], 1.0, axis=-1)
    dlogit = loss_scale * (p - onehot)
    return dlogit, dlogit[..., None] * w, np.einsum("tnm,tnmh->h", dlogit, hd), dlogit.sum()


def pred_out(logits):
    """[T, N, M] -> the reference's pred_out [N, M, T] (:317)."""
    return np.ascontiguousarray(np.moveaxis(logits, 0, 2))


def loss_as_named(ce):
    """What ``loss_batchmean`` would be if axis 1 were time: mean_n sum_t ce."""
    return ce.sum(axis=0).mean()


def model_forward(x, labels, params, lap, K, H):
    """x [N, M, F, T], labels [N, T], params (Wx, Wh, b, w, bh); keep_prob = 1.
    Returns (loss, logits [T, N, M], ce [T, N], state for model_backward)."""
    Wx, Wh, b, w, bh = params
    N, M, F, T = x.shape
    xs = LO.unstack_time(np.asarray(x, np.float64).reshape(N, M, F * T), T)
    hs, _, caches = LO.layer_forward(xs, (Wx, Wh, b), lap, K, H, gates="standard")
    lab = np.asarray(labels).T
    logits, ce, loss = head_forward(hs, w, bh, lab, 1.0 / T)
    return loss, logits, ce, (hs, caches, lab, logits, T)


def model_backward(state, params, lap, K, H):
    """Every gradient of model_forward's loss: dict Wx, Wh, b, w, bh, x ([N, M, F, T])."""
    Wx, Wh, b, w, bh = params
    hs, caches, lab, logits, T = state
    _, dhs, dw, db = head_backward(hs, w, logits, lab, 1.0 / T)
    dxs, _, _, dWx, dWh, dbg = LO.layer_backward(dhs, None, caches, (Wx, Wh, b), lap, K, H,
                                                 gates="standard")
    return dict(Wx=dWx, Wh=dWh, b=dbg, w=dw.reshape(np.shape(w)), bh=np.array([db]),
                x=np.ascontiguousarray(np.moveaxis(dxs, 0, 3)))


def clip_by_norm(g, c):
    """tf.clip_by_norm: g * c / max(||g||, c)."""
    return g * c / max(float(np.sqrt((g * g).sum())), c)


def sgd_steps(x, labels, params, lap, K, H, lr, steps, max_grad_norm=None):
    """``steps`` plain gradient-descent steps; returns (params, losses, last gradients)."""
    names = ("Wx", "Wh", "b", "w", "bh")
    params = [np.array(p, np.float64) for p in params]
    losses, g = [], None
    for _ in range(steps):
        loss, _, _, st = model_forward(x, labels, params, lap, K, H)
        g = model_backward(st, params, lap, K, H)
        if max_grad_norm is not None:
            g = {k: (clip_by_norm(v, max_grad_norm) if k in names else v) for k, v in g.items()}
        params = [p - lr * g[k].reshape(p.shape) for p, k in zip(params, names)]
        losses.append(loss)
    return params, losses, g


def ring_lap(M):
    """L~ of the M-ring's normalised Laplacian rescaled by lmax = 2 (L - I =
    -A/2): (rowptr, col, val) in CSR, float64."""
    rowptr = np.arange(0, 2 * M + 1, 2, dtype=np.int32)
    col = np.empty(2 * M, np.int32)
    for m in range(M):
        col[2 * m:2 * m + 2] = sorted(((m - 1) % M, (m + 1) % M))
    return rowptr, col, np.full(2 * M, -0.5)
