"""Float64 restatement of the pooled cgcnn classifier (lib/models.py:24-127 with
the class loss of lib/graph_model.py:249-258): forward, loss, backward and the
Momentum update, for tests/test_cgcnn_ref_cpu.py (which pins the backward to the
forward by finite differences) and the GPU tests of cgcnn.CGCNNModel.

The convolution, its backward and mpool1's forward are oracle.cheb_oracle's, run
in float64; the pool backwards, the fc layers, the loss and Momentum are
restated here.

A network is a dict:
  laps   [(rowptr, col, val)] the CSR of L~ per conv level
  K, p   per conv level;  brelu 'b1relu' | 'b2relu';  pool 'mpool1' | 'apool1'
  nfc    the number of fc layers (the last is ``logits``)
  reg    the regularization factor
Parameters are a list in creation order: per conv level W [Fin K, F] (then the
bias [1, M, F] with b2relu), per fc layer W [Min, Mout] and b [Mout].
"""
import numpy as np

from oracle import cheb_oracle as O


def ring_lap(M, rng=None):
    """A rescaled Laplacian on a ring of M vertices as (rowptr, col, val); with
    ``rng`` the two off-diagonals get independent values, so L~ != L~^T."""
    import scipy.sparse
    i = np.arange(M)
    lo = -0.5 * np.ones(M) if rng is None else -rng.uniform(0.2, 0.8, M)
    hi = -0.5 * np.ones(M) if rng is None else -rng.uniform(0.2, 0.8, M)
    A = scipy.sparse.coo_matrix((np.concatenate([lo, hi]),
                                 (np.concatenate([i, i]), np.concatenate([(i - 1) % M, (i + 1) % M]))),
                                shape=(M, M))
    return O.canonical_csr(A.tocsr())


def conv_forward(x, lap, W, K):
    """(basis [N M, Fin K], y [N, M, F]) in float64, the recurrence in CSR order."""
    rowptr, col, val = lap
    N, M, Fin = x.shape
    Xt = O.chebyshev_basis(rowptr, col, np.asarray(val, np.float64), O.input_layout(np.asarray(x, np.float64)), K)
    A = O.basis_layout(Xt, N, M, Fin, K)
    return A, (A @ W).reshape(N, M, W.shape[1])


def conv_backward(dy, A, W, lap, K, N, M, Fin):
    rowptr, col, val = lap
    return O.cheb_backward(dy, A, W, rowptr, col, np.asarray(val, np.float64), N, M, Fin, K)


def mpool_backward(dy, argmax, M):
    """dy goes to the window's FIRST maximum (argmax: its absolute vertex), 0 elsewhere."""
    N, Mo, F = dy.shape
    dx = np.zeros((N, M, F))
    n, _, f = np.meshgrid(np.arange(N), np.arange(Mo), np.arange(F), indexing="ij")
    dx[n, argmax, f] = dy
    return dx


def apool_forward(x, p):
    N, M, F = x.shape
    return x.reshape(N, M // p, p, F).sum(axis=2) / p


def apool_backward(dy, p):
    return np.repeat(dy, p, axis=1) / p


def top_two_gap(x, p):
    """Per window: (largest - second largest, the largest's magnitude)."""
    N, M, F = x.shape
    s = np.sort(x.reshape(N, M // p, p, F), axis=2)
    return s[:, :, -1, :] - s[:, :, -2, :], np.abs(s[:, :, -1, :])


def softmax_xent(logits, labels):
    """(mean cross-entropy, dlogits = (softmax - onehot) / N), max-subtracted."""
    N = logits.shape[0]
    z = logits - logits.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=1))
    ce = lse - z[np.arange(N), labels]
    d = np.exp(z - lse[:, None])
    d[np.arange(N), labels] -= 1.0
    return ce.mean(), d / N


def split_params(net, params):
    """([(W, b or None)] per conv level, [(W, b)] per fc layer)."""
    it = iter(params)
    convs = [(next(it), next(it) if net["brelu"] == "b2relu" else None) for _ in net["laps"]]
    return convs, [(next(it), next(it)) for _ in range(net["nfc"])]


def regularised(net, params):
    """One bool per parameter: the fc / logits weights and biases."""
    nconv = len(net["laps"]) * (2 if net["brelu"] == "b2relu" else 1)
    return [i >= nconv for i in range(len(params))]


def forward(x, labels, params, net, masks=None):
    """(logits, loss, state).  ``masks``: per hidden fc layer the dropout
    multiplier [N, Mout] (0 or 1 / keep), None for no dropout.  state keeps what
    the backward and the margin checks need."""
    convs, fcs = split_params(net, params)
    st = dict(conv=[], fc=[], pre=[], gaps=[])
    h = np.asarray(x, np.float64)
    if h.ndim == 2:
        h = h[:, :, None]
    for (W, b), lap, K, p in zip(convs, net["laps"], net["K"], net["p"]):
        N, M, Fin = h.shape
        A, y = conv_forward(h, lap, W, K)
        pre = y if b is None else y + b
        a = np.maximum(pre, 0)
        arg = None
        if p > 1:
            if net["pool"] == "mpool1":
                st["gaps"].append(top_two_gap(a, p))
                out, arg = O.mpool1_forward(a, p)
            else:
                out = apool_forward(a, p)
        else:
            out = a
        st["conv"].append(dict(A=A, pre=pre, arg=arg, dims=(N, M, Fin), act=a, out=out))
        st["pre"].append(pre)
        h = out
    h = h.reshape(h.shape[0], -1)
    for j, (W, b) in enumerate(fcs):
        last = j == len(fcs) - 1
        pre = h @ W + b
        rec = dict(x=h, pre=pre, mask=None)
        if last:
            h = pre
        else:
            st["pre"].append(pre)
            h = np.maximum(pre, 0)
            if masks is not None and masks[j] is not None:
                rec["mask"] = np.asarray(masks[j], np.float64)
                h = h * rec["mask"]
        rec["out"] = h
        st["fc"].append(rec)
    ce, dlogits = softmax_xent(h, np.asarray(labels))
    reg = sum(0.5 * (v ** 2).sum() for v, r in zip(params, regularised(net, params)) if r)
    st["dlogits"], st["ce"] = dlogits, ce
    return h, ce + net["reg"] * reg, st


def backward(st, params, net):
    """The gradients of the data term (mean cross-entropy) in parameter order;
    the L2 term's gradient is the update's (``momentum_step``)."""
    convs, fcs = split_params(net, params)
    gfc, gconv = [], []
    dy = st["dlogits"]
    for j in range(len(fcs) - 1, -1, -1):
        rec, (W, _) = st["fc"][j], fcs[j]
        if j < len(fcs) - 1:
            if rec["mask"] is not None:
                dy = dy * rec["mask"]
            dy = dy * (rec["pre"] > 0)
        gfc.append((rec["x"].T @ dy, dy.sum(axis=0)))
        dy = dy @ W.T
    for i in range(len(convs) - 1, -1, -1):
        rec, (W, b) = st["conv"][i], convs[i]
        N, M, Fin = rec["dims"]
        p = net["p"][i]
        dy = dy.reshape(rec["out"].shape)
        if p > 1:
            dy = mpool_backward(dy, rec["arg"], M) if net["pool"] == "mpool1" else apool_backward(dy, p)
        dz = dy * (rec["pre"] > 0)
        dx, dW = conv_backward(dz, rec["A"], W, net["laps"][i], net["K"][i], N, M, Fin)
        gconv.append((dW, None if b is None else dz.sum(axis=0, keepdims=True)))
        dy = dx
    out = []
    for dW, db in reversed(gconv):
        out += [dW] + ([db] if db is not None else [])
    for dW, db in reversed(gfc):
        out += [dW, db]
    return out, dy  # dy: the gradient of the input (finite-difference checks)


def momentum_step(params, grads, accums, lr, momentum, reg, reg_mask, grad_scale=1.0):
    """TF 1.x MomentumOptimizer (no Nesterov) on g = grad * grad_scale + reg * w for
    the regularised variables; returns (params, accums)."""
    new_p, new_a = [], []
    for w, g, a, r in zip(params, grads, accums, reg_mask):
        g = g.reshape(w.shape) * grad_scale + (reg * w if r else 0.0)
        a = momentum * a + g
        new_p.append(w - lr * a)
        new_a.append(a)
    return new_p, new_a


def margins_ok(st, rel=1e-6):
    """Every ReLU pre-activation and every max-pool top-two gap is further than
    ``rel`` of its layer's largest magnitude from zero.  Exact zeros are let
    through where they are deterministic: a pre-activation of exactly 0 (a fake
    vertex of the coarsening: zero input, empty Laplacian row) and a window
    whose two largest are both exactly 0 (post-ReLU; first-max then picks the
    same entry on both sides)."""
    for pre in st["pre"]:
        nz = np.abs(pre[pre != 0])
        if nz.size and nz.min() <= rel * np.abs(pre).max():
            return False
    for gap, top in st["gaps"]:
        tie0 = (gap == 0) & (top == 0)
        if (gap[~tie0] <= rel * top.max()).any():
            return False
    return True


def init_params(rng, net, Fin, F, M_levels, fc_dims):
    """Random float64 parameters of the right shapes (weights N(0, 0.3), biases 0.1 + noise)."""
    params, fi = [], Fin
    for fo, K, M in zip(F, net["K"], M_levels):
        params.append(0.3 * rng.standard_normal((fi * K, fo)))
        if net["brelu"] == "b2relu":
            params.append(0.1 + 0.05 * rng.standard_normal((1, M, fo)))
        fi = fo
    for a, b in zip(fc_dims[:-1], fc_dims[1:]):
        params += [0.3 * rng.standard_normal((a, b)), 0.1 + 0.05 * rng.standard_normal(b)]
    return params
