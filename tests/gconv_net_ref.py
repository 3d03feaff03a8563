"""float64 restatement of the pure graph-convolution networks of ``GconvModel``
(lib/gconv_lstm.py:297-372) with the MSE loss and one Adam step.

TEST HELPER ONLY.  Written from the reference text; composed from the committed
oracles: each filter is ``lstm_oracle.cheb_conv64`` (cheby_conv in float64) with
``cheb_oracle.cheb_backward``, the loss is ``model_oracle.loss_and_grad``, the
update ``cheb_oracle.adam_step``.

  inference_gconv (:297-314)                  conv_init -> tanh, R residual layers with
                                              tanh (:642-658), output_layer, no activation
  inference_gconv_period_no_expand (:316-333) the same with ReLU
  inference_gconv_period_expand (:335-372)    three branches on the columns
      [0, 2 Tc), [2 Tc, 2 (Tc + Tp)), [2 (Tc + Tp), 2 (Tc + Tp + Tt)): conv_init_j ->
      tanh, residual layers with ReLU, output_layer_j -> ReLU; concat of the three
      [N, M, out] results, one merge_layer filter [3 out -> out]

A network's weights ``Ws`` = [W_init, (W_i0, W_i1) * R, W_out]; the parameters of
``inference_gconv_period_expand`` are the three branches' lists and the merge
weight, flat in that order (``flat``).  TanhGrad and ReluGrad are taken from the
activation's OUTPUT, as TF does.  The backward is pinned to the forward by
central finite differences (tests/test_gconv_net_ref_cpu.py).
"""
from __future__ import annotations

import numpy as np

from oracle import cheb_oracle as O
from oracle import model_oracle as MO
from oracle.lstm_oracle import cheb_conv64  # noqa: F401  (also used by the GPU tests)

SINGLE = {"inference_gconv": ("tanh", "tanh", "none"),
          "inference_gconv_period_no_expand": ("relu", "relu", "none")}
EXPAND = "inference_gconv_period_expand"
EXPAND_ACTS = ("tanh", "relu", "relu")
INFER_FUNCS = tuple(SINGLE) + (EXPAND,)


def r32(a):
    """float32 values held as float64."""
    return np.asarray(a, np.float32).astype(np.float64)


def branch_columns(T):
    """(:340-342): the column range of branch j; the 2 is the reference's."""
    Tc, Tp, Tt = T
    return [(0, 2 * Tc), (2 * Tc, 2 * (Tc + Tp)), (2 * (Tc + Tp), 2 * (Tc + Tp + Tt))]


def variable_names(infer_func, R):
    """tf.get_variable('weights') under the scopes of :297-372 and :642-658, in creation order."""
    def net(j):
        names = [f"conv_init{j}/weights"]
        for i in range(R):
            names += [f"conv_layer_{i}{j}/residual_layer_{i}/sublayer0/weights",
                      f"conv_layer_{i}{j}/residual_layer_{i}/sublayer1/weights"]
        return names + [f"output_layer{j}/weights"]
    if infer_func in SINGLE:
        return net("")
    assert infer_func == EXPAND
    return net("_0") + net("_1") + net("_2") + ["merge_layer/weights"]


def _act(pre, act):
    return np.tanh(pre) if act == "tanh" else np.maximum(pre, 0.0) if act == "relu" else pre


def _dact(dy, out, act):
    """TanhGrad dy (1 - y^2) / ReluGrad dy [y > 0] from the output y."""
    if act == "tanh":
        return dy * (1.0 - out * out)
    return dy * (out > 0) if act == "relu" else np.asarray(dy, np.float64)


# ---- one residual network ------------------------------------------------------------------
def net_forward(x, Ws, lap, K, R, acts):
    """(out, cache); cache[li] = (input, basis, pre-activation, output, act) of filter li."""
    a_init, a_res, a_last = acts
    cache = []

    def f(inp, W, res, act):
        A, y = cheb_conv64(inp, lap, W, K)
        pre = y + res if res is not None else y
        out = _act(pre, act)
        cache.append((inp, A, pre, out, act))
        return out

    h = f(np.asarray(x, np.float64), Ws[0], None, a_init)
    li = 1
    for _ in range(R):                                   # residual_layer (:642-658)
        t = f(h, Ws[li], None, a_res)
        h = f(t, Ws[li + 1], h, a_res)
        li += 2
    return f(h, Ws[li], None, a_last), cache


def net_backward(dout, cache, Ws, lap, K, R):
    """(dx of the network's input, [dW] in the order of Ws)."""
    rowptr, col, val = lap
    dWs = [None] * len(Ws)

    def b(li, dy):
        inp, A, _, out, act = cache[li]
        dz = _dact(dy, out, act)
        N, M, Fin = inp.shape
        dx, dW = O.cheb_backward(dz, A, Ws[li], rowptr, col, val, N, M, Fin, K)
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
    dx, _ = b(0, dh)
    return dx, dWs


# ---- the three networks ------------------------------------------------------------------
def flat(params, infer_func):
    """The variables in creation order."""
    if infer_func in SINGLE:
        return list(params)
    nets, merge = params
    return [w for Ws in nets for w in Ws] + [merge]


def unflat(ws, infer_func):
    ws = list(ws)
    if infer_func in SINGLE:
        return ws
    per = (len(ws) - 1) // 3
    return [ws[j * per:(j + 1) * per] for j in range(3)], ws[-1]


def forward(x, params, infer_func, lap, K, R, T):
    """(out [N, M, out_features], fw)."""
    x = np.asarray(x, np.float64)
    if infer_func in SINGLE:
        out, cache = net_forward(x, params, lap, K, R, SINGLE[infer_func])
        return out, dict(caches=[cache])
    nets, merge = params
    outs, caches = [], []
    for (a, b), Ws in zip(branch_columns(T), nets):
        o, c = net_forward(x[..., a:b], Ws, lap, K, R, EXPAND_ACTS)
        outs.append(o)
        caches.append(c)
    cat = np.concatenate(outs, axis=2)                    # (:365)
    A, out = cheb_conv64(cat, lap, merge, K)              # merge_layer (:366-369)
    return out, dict(caches=caches, cat=cat, A=A)


def backward(dout, fw, params, infer_func, lap, K, R):
    """Gradients in ``params``' structure."""
    if infer_func in SINGLE:
        return net_backward(dout, fw["caches"][0], params, lap, K, R)[1]
    nets, merge = params
    rowptr, col, val = lap
    N, M, Fc = fw["cat"].shape
    dcat, dmerge = O.cheb_backward(np.asarray(dout, np.float64), fw["A"], merge, rowptr, col, val, N, M, Fc, K)
    out_f = Fc // 3
    dnets = [net_backward(dcat[..., j * out_f:(j + 1) * out_f], fw["caches"][j], nets[j], lap, K, R)[1]
             for j in range(3)]
    return dnets, dmerge


def loss(x, labels, params, infer_func, lap, K, R, T):
    return MO.loss_and_grad(forward(x, params, infer_func, lap, K, R, T)[0], labels)[0]


def loss_and_grads(x, labels, params, infer_func, lap, K, R, T):
    """(loss, out, grads, fw)."""
    out, fw = forward(x, params, infer_func, lap, K, R, T)
    l, dout = MO.loss_and_grad(out, labels)
    return l, out, backward(dout, fw, params, infer_func, lap, K, R), fw


def train_step(x, labels, params, infer_func, lap, K, R, T, adam_state, step, lr):
    """One Adam step over the flat variable list: (loss, flat grads, new params, new adam_state)."""
    l, _, grads, _ = loss_and_grads(x, labels, params, infer_func, lap, K, R, T)
    fg = flat(grads, infer_func)
    new_p, new_s = [], []
    for p, g, (m, v) in zip(flat(params, infer_func), fg, adam_state):
        p2, m2, v2 = O.adam_step(p, g, m, v, step, lr=lr)
        new_p.append(p2)
        new_s.append((m2, v2))
    return l, fg, unflat(new_p, infer_func), new_s


def shapes(infer_func, T, H, K, R, out):
    """The variables' shapes in creation order (cheby_conv: [K Fin, Fout], lib/filter.py:64)."""
    def net(fin):
        return [(K * fin, H)] + [(K * H, H)] * (2 * R) + [(K * H, out)]
    if infer_func in SINGLE:
        return net(2 * sum(T))
    return [s for a, b in branch_columns(T) for s in net(b - a)] + [(K * 3 * out, out)]


def seeded_params(rng, infer_func, T, H, K, R, out, scale=0.1):
    """N(0, scale) float32 values (untruncated: values only) in the model's structure."""
    return unflat([r32(scale * rng.standard_normal(s)) for s in shapes(infer_func, T, H, K, R, out)],
                  infer_func)


def relu_margins(fw):
    """min |pre| / max |pre| over every ReLU filter of the last forward (inf: no ReLU)."""
    worst = np.inf
    for cache in fw["caches"]:
        for _, _, pre, _, act in cache:
            if act == "relu":
                worst = min(worst, float(np.abs(pre).min() / np.abs(pre).max()))
    return worst
