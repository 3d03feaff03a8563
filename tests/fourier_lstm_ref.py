"""Float64 restatement of the gconv-LSTM with the Fourier filter.

TEST HELPER ONLY.  ``lib/gconv_lstm.py::GConvLSTMCell.__call__`` (:183-221) with
``filter_type = "fourier_conv"`` (:59): the eight filters of a cell are
``lib/filter.py::fourier_conv`` (:11-42) on the per-gate variables
``[nNode, feat_out, feat_in]`` (:116-133).  Here the four x- (h-) variables are
concatenated along feat_out in the order z, i, f, o -- Wx [M, 4H, Fin],
Wh [M, 4H, H], b [4H] -- and each side is ONE ``oracle.fourier_oracle``
filter; the gate algebra is ``oracle/lstm_oracle.py``'s (:188-218 of the
reference).  Driven by ``static_rnn`` (:609-627) for the layer, BPTT for the
gradient.  Its backward is pinned to its forward by central finite differences
(tests/test_fourier_lstm_cpu.py).
"""
from __future__ import annotations

import numpy as np

from oracle import fourier_oracle as FO


def r32(a):
    """What a float32 kernel input is, as float64."""
    return np.asarray(a, np.float32).astype(np.float64)


def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def gate_update(a, c, gates="reference"):
    """The gate algebra (lib/gconv_lstm.py:188-218) on the pre-activations
    a [..., 4H] (z, i, f, o along the last axis) and the state c [..., H].
    Returns (c', h', dict of z, i, f, o, az)."""
    H = a.shape[-1] // 4
    az, ai, af, ao = (a[..., q * H:(q + 1) * H] for q in range(4))
    z = np.tan(az) if gates == "reference" else np.tanh(az)       # (:188)
    i, f = _sigmoid(ai), _sigmoid(af)                             # (:195, :202)
    o = np.tanh(ao) if gates == "reference" else _sigmoid(ao)     # (:209)
    cn = f * c + i * z                                            # (:215)
    hn = o * np.tanh(cn)                                          # (:218)
    return cn, hn, dict(z=z, i=i, f=f, o=o, az=az)


def cell_forward(x, c, h, Wx, Wh, b, U, gates="reference"):
    """One step (lib/gconv_lstm.py:183-221).  Returns (c', h', cache); the
    cache holds ``az`` (the z pre-activation, for the tan pole guard)."""
    gx, xhat = FO.fourier_forward(x, Wx, U)
    gh, hhat = FO.fourier_forward(h, Wh, U)
    a = gx + gh + np.asarray(b, np.float64)                       # (:186-187 ...)
    c = np.asarray(c, np.float64)
    cn, hn, g = gate_update(a, c, gates)
    cache = dict(c=c, cn=cn, xhat=xhat, hhat=hhat, **g)
    return cn, hn, cache


def cell_backward(dh, dc, cache, Wx, Wh, U, gates="reference"):
    """Gradient of cell_forward: (dx, dc_prev, dh_prev, dWx, dWh, db)."""
    z, i, f, o, c, cn = (cache[k] for k in ("z", "i", "f", "o", "c", "cn"))
    tc = np.tanh(cn)
    dcn = dh * o * (1 - tc * tc) + dc
    d_o = dh * tc
    d_z, d_i, d_f = dcn * i, dcn * z, dcn * c
    daz = d_z * (1 + z * z) if gates == "reference" else d_z * (1 - z * z)
    dai, daf = d_i * i * (1 - i), d_f * f * (1 - f)
    dao = d_o * (1 - o * o) if gates == "reference" else d_o * o * (1 - o)
    dpre = np.concatenate([daz, dai, daf, dao], axis=-1)          # [N, M, 4H]
    dx, dWx = FO.fourier_backward(dpre, Wx, U, cache["xhat"])
    dh_prev, dWh = FO.fourier_backward(dpre, Wh, U, cache["hhat"])
    db = dpre.reshape(-1, dpre.shape[-1]).sum(axis=0)
    return dx, dcn * f, dh_prev, dWx, dWh, db


def layer_forward(xs, params, U, c0=None, h0=None, gates="reference"):
    """static_rnn of one cell over xs [T, N, M, Fin] (zero state when None).
    Returns (hs, cs, caches)."""
    Wx, Wh, b = params
    T, N, M, _ = xs.shape
    H = Wh.shape[2]
    c = np.zeros((N, M, H)) if c0 is None else np.asarray(c0, np.float64)
    h = np.zeros((N, M, H)) if h0 is None else np.asarray(h0, np.float64)
    hs, cs, caches = [], [], []
    for t in range(T):
        c, h, cache = cell_forward(xs[t], c, h, Wx, Wh, b, U, gates)
        hs.append(h)
        cs.append(c)
        caches.append(cache)
    return np.stack(hs), np.stack(cs), caches


def layer_backward(dhs, dcT, caches, params, U, gates="reference", dhT=None):
    """BPTT of layer_forward.  dhs [T, N, M, H] = gradient of the outputs, dcT /
    dhT = gradient of the final state (None = 0).
    Returns (dxs, dc0, dh0, dWx, dWh, db)."""
    Wx, Wh, _ = params
    T = len(caches)
    dh_rec = np.zeros_like(dhs[0], dtype=np.float64) if dhT is None else np.asarray(dhT, np.float64)
    dc = np.zeros_like(dhs[0], dtype=np.float64) if dcT is None else np.asarray(dcT, np.float64)
    dWx, dWh, db = np.zeros(Wx.shape), np.zeros(Wh.shape), np.zeros(Wh.shape[1])
    dxs = [None] * T
    for t in range(T - 1, -1, -1):
        dx, dc, dh_rec, gWx, gWh, gb = cell_backward(dhs[t] + dh_rec, dc, caches[t], Wx, Wh, U, gates)
        dxs[t] = dx
        dWx += gWx
        dWh += gWh
        db += gb
    return np.stack(dxs), dc, dh_rec, dWx, dWh, db


def max_az(caches):
    """max |a_z| over a run: z = tan(a_z) has its first pole at pi/2."""
    return max(float(np.abs(c["az"]).max()) for c in caches)
