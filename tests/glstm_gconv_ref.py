"""float64 restatement of ``GconvModel.inference_glstm_gconv`` (lib/gconv_lstm.py
:374-400; ``inference_glstm_gconv_no_expand`` :402-428 is the same code) with its
MSE loss, one Adam step and ``GraphModel.predict`` (lib/graph_model.py:64-94).

TEST HELPER ONLY.  Composed from what exists: the LSTM layer is
``oracle/lstm_oracle.py`` (cheby_conv) or ``tests/fourier_lstm_ref.py``
(fourier_conv); the head's filters are ``lstm_oracle.cheb_conv64`` /
``cheb_oracle.cheb_backward`` or ``oracle.fourier_oracle``; the head's wiring is
``model_oracle.forward / backward``'s with one difference: conv_init's input
is h_T of the LSTM, so its input gradient is kept and becomes the layer's dhT.

The DropoutWrapper(output_keep_prob) of every layer (lib/gconv_lstm.py:616, :623)
is a GIVEN multiplier b / keep per layer (``drop_mult``: the device mask stream
restated from ops.DROP_WEYL as tests/test_dropout_cpu.py does); the last layer
is read at its last step only, so its multiplier is the [N, M, H] slice at
element offset (T-1) N M H of the layer's stream.

``filt`` = ("fourier_conv", U) or ("cheby_conv", (rowptr, col, val), K).
Parameters: ``layers`` = [(Wx, Wh, b)] per LSTM layer, ``head`` = [W_init,
(W_i0, W_i1) * R, W_out].  The backward is pinned to the forward by central
finite differences (tests/test_glstm_gconv_ref_cpu.py).
"""
from __future__ import annotations

import numpy as np

import fourier_lstm_ref as FR
from cnn_graph_amd.ops import DROP_WEYL
from oracle import cheb_oracle as O
from oracle import fourier_oracle as FO
from oracle import lstm_oracle as LO
from oracle import model_oracle as MO

M64 = (1 << 64) - 1
r32 = FR.r32


# ---- small graphs and seeded parameters -------------------------------------------------
def ring_chords_laplacian(M: int):
    """Normalized Laplacian (float32 CSR, lmax = 2) of a ring of M vertices plus
    the chords i -- i + 3 (irregular weights, so no two rows of L~ agree)."""
    import scipy.sparse
    A = np.zeros((M, M), np.float32)
    for i in range(M):
        for j, w in (((i + 1) % M, 1.0), ((i + 3) % M, 0.5 + 0.25 * (i % 3))):
            if i != j:
                A[i, j] = A[j, i] = max(A[i, j], np.float32(w))
    return scipy.sparse.csr_matrix(O.laplacian(scipy.sparse.csr_matrix(A), normalized=True),
                                   dtype=np.float32)


def cheb_lap(L, lmax=2):
    """(rowptr, col, val) of L~ as the device plan holds it."""
    return O.canonical_csr(O.rescale_L(L, lmax))


def seeded_params(rng, filter, M, F, H, C, K, R, out, layers=1, scale=0.1):
    """(layers, head) drawn as the model initialises them (uniform +-0.1 cells,
    glorot-uniform biases, N(0, 0.1) head -- untruncated: values only), float32
    values held as float64."""
    fourier = filter == "fourier_conv"
    lim = np.sqrt(6.0 / (2 * H))
    ls = []
    for li in range(layers):
        fin = F if li == 0 else H
        wx = (M, 4 * H, fin) if fourier else (K * fin, 4 * H)
        wh = (M, 4 * H, H) if fourier else (K * H, 4 * H)
        ls.append((r32(rng.uniform(-scale, scale, wx)), r32(rng.uniform(-scale, scale, wh)),
                   r32(rng.uniform(-lim, lim, 4 * H))))
    dims = [(H, C)] + [(C, C)] * (2 * R) + [(C, out)]
    head = [r32(0.1 * rng.standard_normal((M, fo, fi) if fourier else (K * fi, fo))) for fi, fo in dims]
    return ls, head


# ---- the dropout mask stream ---------------------------------------------------------
def draws(seed: int, n: int) -> np.ndarray:
    """u in [0, 1) of elements 0..n-1 under seed (tests/test_dropout_cpu.py)."""
    with np.errstate(over="ignore"):
        i = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(seed & M64) + np.uint64(DROP_WEYL) * i
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_bits(seed: int, shape, keep: float, offset: int = 0) -> np.ndarray:
    """b = floor(keep + u) in float32 (0 or 1) of the slice at element ``offset``."""
    n = int(np.prod(shape))
    s = (int(seed) + DROP_WEYL * int(offset)) & M64
    return np.floor(np.float32(keep) + draws(s, n)).reshape(shape)


def drop_mult(seed: int, shape, keep: float, offset: int = 0) -> np.ndarray:
    """The dropout as a float64 multiplier b / keep (keep as the float32 it is)."""
    if keep >= 1.0:
        return np.ones(shape)
    return keep_bits(seed, shape, keep, offset).astype(np.float64) / float(np.float32(keep))


def wrapper_call_seed(wrapper_seed: int, call: int) -> int:
    """DropoutWrapper.next_seed() of its ``call``-th call (1-based)."""
    return (int(wrapper_seed) + 0xD1B54A32D192ED03 * int(call)) & M64


# ---- one filter, either kind -----------------------------------------------------------
def filter_forward(filt, x, W):
    """(y [N, M, Fout], what the backward needs)."""
    if filt[0] == "fourier_conv":
        return FO.fourier_forward(x, W, filt[1])
    A, y = LO.cheb_conv64(x, filt[1], W, filt[2])
    return y, (A, x.shape)


def filter_backward(filt, dy, W, saved):
    """(dx, dW)."""
    if filt[0] == "fourier_conv":
        return FO.fourier_backward(dy, W, filt[1], saved)
    A, (N, M, Fin) = saved
    rowptr, col, val = filt[1]
    return O.cheb_backward(dy, A, W, rowptr, col, val, N, M, Fin, filt[2])


# ---- the LSTM layers ------------------------------------------------------------------
def _layer_forward(filt, xs, P, gates):
    if filt[0] == "fourier_conv":
        return FR.layer_forward(xs, P, filt[1], gates=gates)
    return LO.layer_forward(xs, P, filt[1], filt[2], P[1].shape[1] // 4, gates=gates)


def _layer_backward(filt, dhs, caches, P, gates):
    if filt[0] == "fourier_conv":
        return FR.layer_backward(dhs, None, caches, P, filt[1], gates)
    return LO.layer_backward(dhs, None, caches, P, filt[1], filt[2], P[1].shape[1] // 4, gates)


def max_az(fw, gates):
    """max |a_z| over every layer and step (the tan pole guard).  The Chebyshev
    oracle's caches keep z, not a_z: |a_z| < pi/2 there gives a_z = arctan(z)."""
    if gates != "reference":
        return 0.0
    m = 0.0
    for _, _, caches in fw["layers"]:
        for c in caches:
            az = c["az"] if "az" in c else np.arctan(c["z"])
            m = max(m, float(np.abs(az).max()))
    return m


# ---- the model ------------------------------------------------------------------------
def forward(xs, layers, head, filt, R, gates="reference", mults=None):
    """xs [T, N, M, F].  mults[li]: the multiplier of layer li's wrapper -- [T, N,
    M, H] for a layer below the last, [N, M, H] for the last; None = no dropout.
    Returns (out [N, M, out_features], fw)."""
    inp = np.asarray(xs, np.float64)
    nl = len(layers)
    fwl = []
    for li, P in enumerate(layers):
        hs, cs, caches = _layer_forward(filt, inp, P, gates)
        fwl.append((hs, cs, caches))
        if li < nl - 1:
            inp = hs if mults is None or mults[li] is None else hs * mults[li]
    h = fwl[-1][0][-1]
    if mults is not None and mults[-1] is not None:
        h = h * mults[-1]
    cache = []

    def f(x, W, res, act):
        y, saved = filter_forward(filt, x, W)
        if res is not None:
            y = y + res
        out = np.maximum(y, 0.0) if act else y
        cache.append((saved, out, act))
        return out

    a = f(h, head[0], None, True)                       # conv_init (:384-389)
    li = 1
    for _ in range(R):                                  # residual_layer (:642-658)
        t = f(a, head[li], None, True)
        a = f(t, head[li + 1], a, True)
        li += 2
    out = f(a, head[li], None, False)                   # output_layer (:395-398)
    return out, dict(layers=fwl, head=cache, T=inp.shape[0])


def backward(dout, fw, layers, head, filt, R, gates="reference", mults=None):
    """(dxs [T, N, M, F], [(dWx, dWh, db)] per layer, [dW] of the head)."""
    cache = fw["head"]
    dhead = [None] * len(head)

    def b(li, dy):
        saved, out, act = cache[li]
        dz = dy * (out > 0) if act else np.asarray(dy, np.float64)
        dx, dW = filter_backward(filt, dz, head[li], saved)
        dhead[li] = dW
        return dx, dz

    last = len(head) - 1
    dh, _ = b(last, dout)
    li = last - 2
    for _ in range(R):
        dt, dz1 = b(li + 1, dh)
        dx0, _ = b(li, dt)
        dh = dx0 + dz1
        li -= 2
    dhT, _ = b(0, dh)                                   # conv_init: its dx is the LSTM's dh_T
    if mults is not None and mults[-1] is not None:
        dhT = dhT * mults[-1]
    nl = len(layers)
    dlayers = [None] * nl
    hs_last = fw["layers"][-1][0]
    dhs = np.zeros_like(hs_last)
    dhs[-1] = dhT
    for li in range(nl - 1, -1, -1):
        dxs, _, _, dWx, dWh, db = _layer_backward(filt, dhs, fw["layers"][li][2], layers[li], gates)
        dlayers[li] = (dWx, dWh, db)
        if li > 0:
            dhs = dxs if mults is None or mults[li - 1] is None else dxs * mults[li - 1]
    return dxs, dlayers, dhead


def loss_and_grads(xs, labels, layers, head, filt, R, gates="reference", mults=None):
    """(loss, out, dxs, layer grads, head grads, fw)."""
    out, fw = forward(xs, layers, head, filt, R, gates, mults)
    l, dout = MO.loss_and_grad(out, labels)
    dxs, dl, dh = backward(dout, fw, layers, head, filt, R, gates, mults)
    return l, out, dxs, dl, dh, fw


def flat_params(layers, head):
    """The model's variable order: every layer's Wx, Wh, b, then the head."""
    return [p for P in layers for p in P] + list(head)


def train_step(xs, labels, layers, head, filt, R, gates, mults, adam_state, step, lr, ema):
    """One Adam step: (loss, flat grads, new flat params, new adam_state, new ema)."""
    l, _, _, dl, dh, _ = loss_and_grads(xs, labels, layers, head, filt, R, gates, mults)
    flat_g = flat_params(dl, dh)
    new_p, new_s = [], []
    for p, g, (m, v) in zip(flat_params(layers, head), flat_g, adam_state):
        p2, m2, v2 = O.adam_step(p, g, m, v, step, lr=lr)
        new_p.append(p2)
        new_s.append((m2, v2))
    return l, flat_g, new_p, new_s, MO.ema_update(ema, l)


# ---- GraphModel.predict / evaluate (lib/graph_model.py:64-122) -------------------------------
def predict(forward_fn, data, labels, batch_size):
    """forward_fn(batch [batch_size, M, C]) -> [batch_size, M, out].  The ragged
    last batch is zero-padded (:72-76, :80-81); the loss is the reference's
    ``loss * batch_size / size`` (:92) with ``loss`` the plain sum of the
    per-batch means, padded rows included."""
    data = np.asarray(data, np.float64)
    size = data.shape[0]
    preds, loss = [], 0.0
    for begin in range(0, size, batch_size):
        end = min(begin + batch_size, size)
        batch = np.zeros((batch_size,) + data.shape[1:])
        batch[:end - begin] = data[begin:end]
        p = forward_fn(batch)
        if labels is not None:
            bl = np.zeros((batch_size,) + p.shape[1:])
            bl[:end - begin] = labels[begin:end]
            loss += float(np.mean((bl - p) ** 2))
        preds.append(p[:end - begin])
    preds = np.concatenate(preds)
    return preds if labels is None else (preds, loss * batch_size / size)


def evaluate_mse(labels, preds):
    """:116."""
    return float(np.sum((np.asarray(labels, np.float64) - preds) ** 2) / preds.size)
