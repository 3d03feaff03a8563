"""float64 restatement of the closeness / period / trend gconv-LSTM networks
(lib/gconv_lstm.py:431-607) with their MSE loss and one Adam step.

TEST HELPER ONLY.  Composed from tests/glstm_gconv_ref.py: its LSTM layer forward
/ backward, its filter forward / backward, its ``keep_bits`` / ``drop_mult``, its
Adam step and EMA (through the oracles it imports).  What this file adds: the
input split (:472-479, :486-487), the two merges and their backward.

  branches  [[(Wx, Wh, b)] per layer] per branch
  merge     "weights": [(W_b, w_b)] per branch -- y_b = filter(h_b; W_b), out = sum_b
            y_b * w_b with w_b [M, out] broadcast over the batch (:490-497)
            "concat": the head [W_init, (W_i0, W_i1) * R, W_out] on concat_b(h_b)
            (:590-607)
  mults     mults[b][li] as glstm_gconv_ref.forward takes them for one stack
            ([T_b, N, M, H] below the last layer, [N, M, H] for the last); None =
            no dropout

The backward is pinned to the forward by central finite differences
(tests/test_glstm_period_ref_cpu.py).
"""
from __future__ import annotations

import numpy as np

import glstm_gconv_ref as GR
from oracle import cheb_oracle as O
from oracle import model_oracle as MO

r32 = GR.r32


# ---- the input split ------------------------------------------------------------------
def split(x, T, F):
    """x [N, M, C] -> per branch [T_b, N, M, F]: branch b reads the columns
    [F S_b, F (S_b + T_b)), S_b the prefix sum of T; step t, feature f is column
    F S_b + f T_b + t (the reshape to [N, M, F, T_b] and the unstack of axis 3)."""
    x = np.asarray(x)
    N, M, _ = x.shape
    out, s = [], 0
    for t in T:
        cols = x[:, :, F * s:F * (s + t)]
        out.append(np.ascontiguousarray(np.moveaxis(cols.reshape(N, M, F, t), 3, 0)))
        s += t
    return out


def unsplit(dxs, T, F, C):
    """The transpose of ``split``: per-branch [T_b, N, M, F] gradients back into
    [N, M, C] (columns no branch reads stay zero)."""
    _, N, M, _ = dxs[0].shape
    dx = np.zeros((N, M, C))
    s = 0
    for g, t in zip(dxs, T):
        dx[:, :, F * s:F * (s + t)] = np.moveaxis(g, 0, 3).reshape(N, M, F * t)
        s += t
    return dx


# ---- one LSTM stack read at its last step ----------------------------------------------
def stack_forward(filt, xs, layers, gates, mults):
    """(h_T through the last layer's multiplier, what the backward needs)."""
    inp = np.asarray(xs, np.float64)
    fwl = []
    for li, P in enumerate(layers):
        hs, cs, caches = GR._layer_forward(filt, inp, P, gates)
        fwl.append((hs, cs, caches))
        if li < len(layers) - 1:
            inp = hs if mults is None or mults[li] is None else hs * mults[li]
    h = fwl[-1][0][-1]
    if mults is not None and mults[-1] is not None:
        h = h * mults[-1]
    return h, fwl


def stack_backward(filt, dh, fwl, layers, gates, mults):
    """(dxs [T, N, M, F], [(dWx, dWh, db)] per layer) from the gradient of the dropped h_T."""
    if mults is not None and mults[-1] is not None:
        dh = dh * mults[-1]
    dhs = np.zeros_like(fwl[-1][0])
    dhs[-1] = dh
    dl = [None] * len(layers)
    for li in range(len(layers) - 1, -1, -1):
        dxs, _, _, dWx, dWh, db = GR._layer_backward(filt, dhs, fwl[li][2], layers[li], gates)
        dl[li] = (dWx, dWh, db)
        if li > 0:
            dhs = dxs if mults is None or mults[li - 1] is None else dxs * mults[li - 1]
    return dxs, dl


# ---- the networks ----------------------------------------------------------------------
def forward(x, T, F, branches, merge, filt, mode, R=0, gates="reference", mults=None):
    """x [N, M, C].  Returns (out [N, M, out_features], fw)."""
    hs, fws = [], []
    for b, xs in enumerate(split(x, T, F)):
        h, fwl = stack_forward(filt, xs, branches[b], gates, None if mults is None else mults[b])
        hs.append(h)
        fws.append(fwl)
    fw = dict(stacks=fws, C=np.asarray(x).shape[2])
    if mode == "weights":
        out, saved = None, []
        for h, (W, w) in zip(hs, merge):
            y, sv = GR.filter_forward(filt, h, W)
            saved.append((y, sv))
            out = y * w if out is None else out + y * w        # X = x * w; X = X + x * w
        fw["merge"] = saved
        return out, fw
    cache = []

    def f(a, W, res, act):
        y, saved = GR.filter_forward(filt, a, W)
        if res is not None:
            y = y + res
        o = np.maximum(y, 0.0) if act else y
        cache.append((saved, o, act))
        return o

    a = f(np.concatenate(hs, axis=2), merge[0], None, True)    # conv_init on the concat
    li = 1
    for _ in range(R):
        t = f(a, merge[li], None, True)
        a = f(t, merge[li + 1], a, True)
        li += 2
    out = f(a, merge[li], None, False)
    fw["head"] = cache
    fw["H"] = [h.shape[2] for h in hs]
    return out, fw


def backward(dout, fw, T, F, branches, merge, filt, mode, R=0, gates="reference", mults=None):
    """(dx [N, M, C], [[(dWx, dWh, db)] per layer] per branch, the merge's gradients
    in ``merge``'s own structure)."""
    B = len(branches)
    if mode == "weights":
        dmerge, dhs = [], []
        for (y, sv), (W, w) in zip(fw["merge"], merge):
            dw = np.sum(dout * y, axis=0)                      # the broadcast reduction over n
            dh, dW = GR.filter_backward(filt, dout * w, W, sv)
            dmerge.append((dW, dw))
            dhs.append(dh)
    else:
        cache = fw["head"]
        dmerge = [None] * len(merge)

        def b_(li, dy):
            saved, o, act = cache[li]
            dz = dy * (o > 0) if act else np.asarray(dy, np.float64)
            dx, dW = GR.filter_backward(filt, dz, merge[li], saved)
            dmerge[li] = dW
            return dx, dz

        last = len(merge) - 1
        dh, _ = b_(last, dout)
        li = last - 2
        for _ in range(R):
            dt, dz1 = b_(li + 1, dh)
            dx0, _ = b_(li, dt)
            dh = dx0 + dz1
            li -= 2
        da, _ = b_(0, dh)
        edges = np.cumsum([0] + fw["H"])
        dhs = [da[:, :, edges[b]:edges[b + 1]] for b in range(B)]
    dxs, dbr = [], []
    for b in range(B):
        g, dl = stack_backward(filt, dhs[b], fw["stacks"][b], branches[b], gates,
                               None if mults is None else mults[b])
        dxs.append(g)
        dbr.append(dl)
    return unsplit(dxs, T, F, fw["C"]), dbr, dmerge


def loss_and_grads(x, labels, T, F, branches, merge, filt, mode, R=0, gates="reference", mults=None):
    """(loss, out, dx, branch grads, merge grads, fw)."""
    out, fw = forward(x, T, F, branches, merge, filt, mode, R, gates, mults)
    l, dout = MO.loss_and_grad(out, labels)
    dx, dbr, dm = backward(dout, fw, T, F, branches, merge, filt, mode, R, gates, mults)
    return l, out, dx, dbr, dm, fw


def max_az(fw, gates):
    return max(GR.max_az(dict(layers=fwl), gates) for fwl in fw["stacks"])


def flat_params(branches, merge, mode):
    """The model's variable order: per branch every layer's Wx, Wh, b, then (merge
    by weights) the branch's filter weight and merge weight; the head last."""
    out = []
    for b, layers in enumerate(branches):
        out += [p for P in layers for p in P]
        if mode == "weights":
            out += list(merge[b])
    return out + (list(merge) if mode == "concat" else [])


def unflatten(flat, branches, merge, mode):
    """``flat_params``' inverse on a list of the same length."""
    it = iter(flat)
    nb, nm = [], []
    for b, layers in enumerate(branches):
        nb.append([tuple(next(it) for _ in P) for P in layers])
        if mode == "weights":
            nm.append((next(it), next(it)))
    if mode == "concat":
        nm = [next(it) for _ in merge]
    return nb, nm


def train_step(x, labels, T, F, branches, merge, filt, mode, R, gates, mults, adam_state, step, lr, ema):
    """One Adam step: (loss, new branches, new merge, new adam_state, new ema)."""
    l, _, _, dbr, dm, _ = loss_and_grads(x, labels, T, F, branches, merge, filt, mode, R, gates, mults)
    new_p, new_s = [], []
    for p, g, (m, v) in zip(flat_params(branches, merge, mode), flat_params(dbr, dm, mode), adam_state):
        p2, m2, v2 = O.adam_step(p, g, m, v, step, lr=lr)
        new_p.append(p2)
        new_s.append((m2, v2))
    nb, nm = unflatten(new_p, branches, merge, mode)
    return l, nb, nm, new_s, MO.ema_update(ema, l)


def seeded_params(rng, filter, mode, M, F, H, K, R, out, B, layers=1, scale=0.1):
    """(branches, merge) drawn as the model initialises them (values only)."""
    fourier = filter == "fourier_conv"
    branches, merge = [], []
    for _ in range(B):
        ls, head = GR.seeded_params(rng, filter, M, F, H, H, K, 0, out, layers, scale)
        branches.append(ls)
        if mode == "weights":
            W = r32(0.1 * rng.standard_normal((M, out, H) if fourier else (K * H, out)))
            merge.append((W, r32(0.1 * rng.standard_normal((M, out)))))
    if mode == "concat":  # the head's width is num_hidden (:455, :594)
        dims = [(B * H, H)] + [(H, H)] * (2 * R) + [(H, out)]
        merge = [r32(0.1 * rng.standard_normal((M, fo, fi) if fourier else (K * fi, fo))) for fi, fo in dims]
    return branches, merge
