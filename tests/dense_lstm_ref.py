"""Float64 reference of the dense LSTM baseline (not a test module), written from
the reference's text -- lib/gconvRNN.py::Model with model_type='lstm' (:257-262,
:280-285, :299-300, :306-315, :326-332, :381-409) and TF 1.x BasicLSTMCell
(rnn_cell_impl.py: ONE kernel [C + H, 4H], gates i | j | f | o,
c' = c sigmoid(f + forget_bias) + sigmoid(i) tanh(j), h' = tanh(c') sigmoid(o))
-- in plain NumPy.  It shares nothing with the device code.

Parameters travel as the list [weight [H, C], bias [C], kernel [C + H, 4H],
cell bias [4H]]: the reference's creation order.
"""
import numpy as np

NAMES = ("w", "bh", "kernel", "b")


def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


# -- the cell over a sequence, given the input projection ---------------------------
def cell_forward(gx, Wh, b, forget_bias=1.0, order="ijfo"):
    """gx [T, N, 4H] -> (hs, cs [T, N, H], act [T, N, 4H] = i | j | f | o).
    ``order`` names the gate blocks of the columns (the known-answer tests
    permute it)."""
    T, N, G = gx.shape
    H = G // 4
    blk = {g: slice(k * H, (k + 1) * H) for k, g in enumerate(order)}
    h, c = np.zeros((N, H)), np.zeros((N, H))
    hs, cs, act = np.zeros((T, N, H)), np.zeros((T, N, H)), np.zeros((T, N, G))
    for t in range(T):
        a = gx[t] + h @ Wh + b
        i, j = sigmoid(a[:, blk["i"]]), np.tanh(a[:, blk["j"]])
        f, o = sigmoid(a[:, blk["f"]] + forget_bias), sigmoid(a[:, blk["o"]])
        c = c * f + i * j
        h = np.tanh(c) * o
        hs[t], cs[t] = h, c
        act[t] = np.concatenate([i, j, f, o], axis=1)
    return hs, cs, act


def cell_backward(dhs, act, cs, Wh):
    """dpre [T, N, 4H] (columns i | j | f | o) from the output gradients."""
    T, N, H = cs.shape
    dpre = np.zeros((T, N, 4 * H))
    dh_rec, dc = np.zeros((N, H)), np.zeros((N, H))
    for t in range(T - 1, -1, -1):
        i, j, f, o = (act[t][:, k * H:(k + 1) * H] for k in range(4))
        c_prev = cs[t - 1] if t else np.zeros((N, H))
        tc = np.tanh(cs[t])
        dh = dhs[t] + dh_rec
        dc = dc + dh * o * (1 - tc * tc)
        dpre[t] = np.concatenate([dc * j * i * (1 - i), dc * i * (1 - j * j),
                                  dc * c_prev * f * (1 - f), dh * tc * o * (1 - o)], axis=1)
        dc = dc * f
        dh_rec = dpre[t] @ Wh.T
    return dpre


def weight_grads(xs, hs, dpre):
    """(dWx [C, 4H], dWh [H, 4H], db [4H]); dWh is zero for T = 1."""
    T, N, C = xs.shape
    G = dpre.shape[2]
    dWx = xs.reshape(T * N, C).T @ dpre.reshape(T * N, G)
    dWh = hs[:T - 1].reshape(-1, hs.shape[2]).T @ dpre[1:].reshape(-1, G)
    return dWx, dWh, dpre.sum((0, 1))


# -- the loss ------------------------------------------------------------------------
def xent_sum(logits, labels, scale):
    """(scale * sum_rows ce, scale * (softmax - onehot), ce [R]) of logits [R, C]."""
    mx = logits.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(logits - mx).sum(1))
    R = logits.shape[0]
    ce = lse - logits[np.arange(R), labels]
    d = np.exp(logits - lse[:, None])
    d[np.arange(R), labels] -= 1.0
    return scale * ce.sum(), scale * d, ce


# -- the model -----------------------------------------------------------------------
def model_forward(x, labels, params, forget_bias=1.0, mask=None, keep=1.0):
    """x [N, C, T], labels [N, T] -> (loss, logits [T, N, C], state).  ``mask``
    [T, N, H] of 0 / 1: the DropoutWrapper's draw on the OUTPUTS (hd = hs / keep
    * mask); the state path reads the unmasked h."""
    w, bh, kernel, b = params
    N, C, T = x.shape
    xs = np.transpose(np.asarray(x, np.float64), (2, 0, 1))  # unstack axis 2
    gx = xs @ kernel[:C]
    hs, cs, act = cell_forward(gx, kernel[C:], b, forget_bias)
    hd = hs if mask is None else hs / keep * mask
    logits = hd @ w + bh
    lab = np.asarray(labels).T.reshape(-1)
    loss, dlogits, ce = xent_sum(logits.reshape(T * N, C), lab, 1.0 / T)
    return loss, logits, (xs, hs, cs, act, hd, dlogits.reshape(T, N, C), mask, keep, ce.reshape(T, N))


def model_backward(state, params):
    """Every parameter gradient (``NAMES``) and dx [N, C, T]."""
    w, bh, kernel, b = params
    xs, hs, cs, act, hd, dlogits, mask, keep, _ = state
    T, N, C = xs.shape
    H = hs.shape[2]
    dw = hd.reshape(T * N, H).T @ dlogits.reshape(T * N, C)
    dbh = dlogits.sum((0, 1))
    dhd = dlogits @ w.T
    dhs = dhd if mask is None else dhd * mask / keep
    dpre = cell_backward(dhs, act, cs, kernel[C:])
    dWx, dWh, db = weight_grads(xs, hs, dpre)
    dx = np.transpose(dpre @ kernel[:C].T, (1, 2, 0))
    return {"w": dw, "bh": dbh, "kernel": np.concatenate([dWx, dWh], 0), "b": db, "x": dx}


def pred_out(logits):
    """concat(predictions, 1) (:315): [T, N, C] -> [N, T*C], column t*C + c."""
    T, N, C = logits.shape
    return np.transpose(logits, (1, 0, 2)).reshape(N, T * C)


def clip_by_norm(g, clip):
    """tf.clip_by_norm of ONE variable's gradient."""
    return g * clip / max(np.sqrt((g * g).sum()), clip)


def sgd_steps(x, labels, params, lr, steps, clip=None, forget_bias=1.0):
    """``steps`` GradientDescent steps with the per-variable clip (:392-403);
    returns (params, losses, the last gradients before clipping)."""
    params = [p.copy() for p in params]
    losses, g = [], None
    for _ in range(steps):
        loss, _, st = model_forward(x, labels, params, forget_bias)
        g = model_backward(st, params)
        losses.append(loss)
        for p, k in zip(params, NAMES):
            p -= lr * (g[k] if clip is None else clip_by_norm(g[k], clip))
    return params, np.array(losses), g
