"""The pure graph-convolution networks of ``GconvModel`` (lib/gconv_lstm.py
:297-372) -- the baselines nips2016/gconvTest.py:93-96 lists next to the
gconv-LSTM variants -- trained as ``GraphModel`` trains them:

  inference_gconv (:297-314)
      conv_init -> tanh, conv_layer_num residual layers with tanh
      (tanh(filter(tanh(filter(x))) + x), :642-658), output_layer, no activation
  inference_gconv_period_no_expand (:316-333)
      the same with ReLU
  inference_gconv_period_expand (:335-372)
      three branches on the closeness / period / trend columns [0, 2 Tc),
      [2 Tc, 2 (Tc + Tp)), [2 (Tc + Tp), 2 (Tc + Tp + Tt)) (the 2 is the
      reference's): conv_init_j -> tanh, residual layers with ReLU,
      output_layer_j -> ReLU; the three [N, M, out] results concatenated and
      passed through ONE merge_layer filter [3 out -> out]

Every network is ``model._ResNet``'s schedule of C-ABI launches with the
activations as arguments; tanh runs in the Chebyshev kernels' y store
(CG_ACT_TANH).  The branches' columns come from cg_slice_channels, the concat and
its split are cg_concat_drop_forward / cg_concat_drop_backward with keep = 1,
the merge filter is cg_cheb_forward_layout / cg_cheb_backward_layout with dx.
Loss, exchange, update, predict, evaluate and fit are ``FlatTrainer``'s: one flat
parameter buffer, one loss launch, one all-reduce when world > 1, one optimizer
launch.  No torch compute op runs in the step.

Variables (names and creation order the reference's, truncated_normal(0, 0.1)
from one generator in that order, lib/filter.py:39, :63): ``conv_init/weights``,
``conv_layer_{i}/residual_layer_{i}/sublayer{0,1}/weights``, ``output_layer/
weights``; with the branches ``conv_init_{j}``, ``conv_layer_{i}_{j}/...``,
``output_layer_{j}`` per branch j, then ``merge_layer/weights``.

``filter="fourier_conv"`` runs ``inference_gconv_period_no_expand`` (ReLU
everywhere: ``model._FourierResNet``); the other two need tanh, which the
Fourier transforms' store does not have.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .graph_conv import truncated_normal_
from .model import _ChannelSplit, _ChebFilter, _net_class, head_names
from .trainer import FlatTrainer, is_fourier_conv

# infer_func -> (after conv_init, inside the residual layers, after the last filter)
SINGLE = {"inference_gconv": ("tanh", "tanh", "none"),
          "inference_gconv_period_no_expand": ("relu", "relu", "none")}
EXPAND = "inference_gconv_period_expand"
EXPAND_ACTS = ("tanh", "relu", "relu")
INFER_FUNCS = tuple(SINGLE) + (EXPAND,)
FLOWS = 2  # channels per time step: hard-coded at lib/gconv_lstm.py:340-342


def branch_columns(T):
    """The [c0, c1) column ranges of the closeness / period / trend branches (:340-342)."""
    T = _check_T(T)
    edges = [FLOWS * sum(T[:j]) for j in range(len(T) + 1)]
    return list(zip(edges[:-1], edges[1:]))


def variable_names(infer_func: str, conv_layer_num: int):
    """The reference's variable names in creation order."""
    if infer_func not in INFER_FUNCS:
        raise ValueError(f"infer_func must be one of {INFER_FUNCS}, got {infer_func!r}")
    if infer_func in SINGLE:
        return head_names(conv_layer_num)
    return [n for j in range(3) for n in head_names(conv_layer_num, f"_{j}")] + ["merge_layer/weights"]


def _check_T(T):
    try:
        T = tuple(int(t) for t in T)
    except TypeError:
        T = ()
    if len(T) != 3 or min(T) < 1:
        raise ValueError(f"T must be (Tc, Tp, Tt), three positive step counts, got {T!r}")
    return T


class GConvNetModel(FlatTrainer):
    """The graph-convolution networks on device; ``infer_func`` selects the
    network by the reference's name (``INFER_FUNCS``).  T = (Tc, Tp, Tt): the
    steps of the closeness, period and trend windows; the input is [N, M, C]
    with C = 2 (Tc + Tp + Tt).  The two single networks run on all columns of x
    whatever T is (:297-333): ``in_features`` gives them another C."""

    def __init__(self, L, N: int, T=(3, 3, 3), num_hidden: int = 64, K: int = 2,
                 conv_layer_num: int = 4, out_features: int = 2, filter: str = "cheby_conv",
                 infer_func: str = "inference_gconv", optimizer: str = "adam",
                 learning_rate: float = 1e-3, decay_rate: float = 0.95, decay_steps: int | None = None,
                 lmax: float = 2, device=None, seed: int = 2017, comm=None,
                 in_features: int | None = None):
        if infer_func not in INFER_FUNCS:
            raise ValueError(f"infer_func must be one of {INFER_FUNCS}, got {infer_func!r}")
        fourier = is_fourier_conv(filter)
        if fourier and (infer_func == EXPAND or "tanh" in SINGLE[infer_func]):
            raise NotImplementedError(
                f"{infer_func} with filter='fourier_conv': the Fourier store has no tanh (cg_fres_* take "
                "none / relu); only inference_gconv_period_no_expand runs on the Fourier filter")
        self.T = _check_T(T)
        self.infer_func, self.filter = infer_func, filter
        self.N, self.H, self.K = int(N), int(num_hidden), int(K)
        self.R, self.Fout = int(conv_layer_num), int(out_features)
        self.C = FLOWS * sum(self.T)
        if in_features is not None and int(in_features) != self.C:
            if infer_func == EXPAND or int(in_features) < 1:
                raise ValueError(f"in_features = {in_features}: {EXPAND} reads the {self.C} columns that T "
                                 "names; the single networks take any positive count")
            self.C = int(in_features)
        self.columns = branch_columns(self.T)
        M, H, K, R, Fout = int(L.shape[0]), self.H, self.K, self.R, self.Fout
        net = _net_class(fourier)
        expand = infer_func == EXPAND
        if expand:
            total = sum(sum(net.sizes(b - a, H, K, M, R, Fout)) for a, b in self.columns)
            total += 3 * Fout * K * Fout
        else:
            total = sum(net.sizes(self.C, H, K, M, R, Fout))
        super().__init__(total, (self.N, M, Fout), optimizer, learning_rate, decay_rate, decay_steps,
                         device, comm)
        self._set_graph(L, fourier, lmax)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        names = variable_names(infer_func, R)
        per = 2 * R + 2  # filters per network
        f32 = dict(device=self.device, dtype=torch.float32)
        if not expand:
            self.nets = [net(self, "", self.C, H, K, R, Fout, gen, names=names, acts=SINGLE[infer_func])]
        else:
            self.nets = [net(self, "", b - a, H, K, R, Fout, gen, input_grad=False,
                             names=names[j * per:(j + 1) * per], acts=EXPAND_ACTS)
                         for j, (a, b) in enumerate(self.columns)]
            self.merge_W, self.merge_dW = self.carve((3 * Fout * K, Fout), names[-1])
            truncated_normal_(self.merge_W, 0.1, gen)
            Nb, Fc = self.N, 3 * Fout
            self.split = _ChannelSplit(self, self.C, self.columns)
            self.x_b = self.split.bufs
            self.cat = torch.empty((Nb, self.M, Fc), **f32)
            self.dcat = torch.empty((Nb, self.M, Fc), **f32)
            self.d_b = [torch.empty((Nb, self.M, Fout), **f32) for _ in range(3)]
            self.out = torch.empty((Nb, self.M, Fout), **f32)
            # merge_layer: ONE filter [3 out -> out] with dx, its basis in the rows layout
            self.merge = _ChebFilter(self, Fc, Fout, K, "none", self.merge_W, self.merge_dW, self.out,
                                     layout="rows")
            # the seams' host arrays of sizes / pointers / (unused) seeds, built once
            self._cat_H = (ctypes.c_int32 * 3)(Fout, Fout, Fout)
            self._cat_seed = (ctypes.c_uint64 * 3)(0, 0, 0)
            self._cat_in = (ctypes.c_void_p * 3)(*[n.out[-1].data_ptr() for n in self.nets])
            self._cat_d = (ctypes.c_void_p * 3)(*[d.data_ptr() for d in self.d_b])
        self._carved()
        self.W, self.dW = self._tensors, self._grads
        self._alloc_ws(self.nets + ([self.merge] if expand else []))
        h = _lib.lib()
        self._cat_f, self._cat_b = h.cg_concat_drop_forward, h.cg_concat_drop_backward

    def forward(self, x, stream=None):
        """The network's output [N, M, out_features]."""
        s = self._stream(stream)
        if tuple(x.shape) != (self.N, self.M, self.C) or not x.is_cuda:
            raise ValueError(f"x must be a cuda tensor of shape {(self.N, self.M, self.C)}")
        x = x.contiguous()
        if self.infer_func != EXPAND:
            return self.nets[0].forward(x, s)
        for net, xi in zip(self.nets, self.split.slices(x, s)):
            net.forward(xi, s)
        _lib.check("cg_concat_drop_forward",
                   self._cat_f(3, self.N, self.M, self._cat_H, self._cat_in, ctypes.c_float(1.0),
                               self._cat_seed, self.cat.data_ptr(), s))
        return self.merge.forward(self.cat, None, s)

    def backward(self, dout, stream=None):
        """Every dW of the last forward from d(out) [N, M, out_features]."""
        s = self._stream(stream)
        dout = dout.contiguous()
        if self.infer_func != EXPAND:
            return self.nets[0].backward(dout, s)
        self.merge.backward(dout, None, self.dcat, False, s)
        _lib.check("cg_concat_drop_backward",
                   self._cat_b(3, self.N, self.M, self._cat_H, self.dcat.data_ptr(), ctypes.c_float(1.0),
                               self._cat_seed, self._cat_d, s))
        for net, d in zip(self.nets, self.d_b):
            net.backward(d, s)
