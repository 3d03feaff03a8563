"""The reference's ResGNN training step on device: ``GraphConv.residual_network``
(lib/graph_conv.py:234-330, ``model_name == 'ResGNN'``) + MSE loss
(lib/graph_model.py:246-275) + Adam with staircase exponential decay
(lib/graph_model.py:277-310), as ONE explicit schedule of C-ABI launches:

  conv_init    a   = relu(cheb(x; W_init))                       cg_cheb_forward_ex
  layer i      t   = relu(cheb(h; W_i0))                          (ReLU in the y store)
               h'  = relu(cheb(t; W_i1) + h)                      (residual + ReLU in the y store)
  convN        out = cheb(h; W_N)
  loss         mean((labels - out)^2), dout = 2 (out - labels) / n, and the
               loss moving average (lib/graph_model.py:265-273)    cg_mse_loss_ema
  (filters whose forward and backward both run the sample-major streaming
  path with Fin % 16 == 0 -- the hidden layers at the humanflow shape -- keep
  their basis in the planes layout, cg_cheb_forward_layout(CG_BASIS_PLANES):
  each Chebyshev step writes its own plane, no rows-layout assembly pass)
  backward     cg_cheb_backward_ex per filter in reverse: ReLU mask from the
               saved outputs, the residual branch's gradient dz1 doubles as the
               buffer the sublayer-0 input gradient is ACCUMULATED into
               (dx_accumulate), so dh_in = dx(f0) + dz1 needs no extra pass
  exchange     one all-reduce of the flat gradient buffer (RcclComm, N > 1)
  update       ONE cg_adam_update over the flat parameter buffer (grad / world)

Loss, exchange, update, the flat buffers and predict / evaluate are
``trainer.FlatTrainer``'s, shared with the gconv-LSTM models: every weight is a
view into one flat fp32 buffer (and so is every gradient), so the optimizer and
the data-parallel exchange are one launch each.  No PyTorch compute op runs in
the step: torch only owns the buffers.
Weights: ``truncated_normal(0, 0.1)`` per ``tf.get_variable('weights')``
(lib/graph_model.py:326-333) in the reference's scope order.

``StackedResGNN`` is ``_inference`` with ``stack_num > 1`` (lib/graph_conv.py:
272-303, the ``_STACK_NUM = 2`` driver nips2016/humanflow-ln-period-shortlong.py
:171): the input's channel groups (``x[..., 0:12]`` and ``x[..., 12:16]``) run
through separate residual networks, merged as ``X = sum_i relu(net_i) * w_i``
with ``w_i [M, 2]`` -- same flat-buffer schedule, one Adam, one all-reduce.

``filter="fourier"`` (``params['filter'] = 'fourier'``, the configuration of the
reference's published humanflow-ln-period runs; lib/graph_conv.py:83-111) runs
the same schedule with every filter on the MFMA transforms (cg_fres_forward /
cg_fres_backward): weights ``[M, Fout, Fin]``, the saved tensor of a filter is
its spectrum xhat, U = ``graph.fourier(L)`` prepared once; ``K`` is accepted
and ignored as at lib/graph_conv.py:103, and no Chebyshev plan is built.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from . import filter as _filter
from . import ops
from .graph_conv import truncated_normal_
from .plan import plan_for
from .trainer import FlatTrainer


ACTS = ("relu", "relu", "none")  # residual_network: after conv_init, in the layers, after convN


def _chain(scope, Fin, F, R, Fout_last, acts=ACTS):
    """(name, Fin, Fout, act) of a residual network's filters in the reference's call order.
    ``acts``: the activation after conv_init, inside the residual layers, after the last filter."""
    a_init, a_res, a_last = acts
    layers = [(f"{scope}conv_init/weights", Fin, F, a_init)]
    for i in range(R):
        layers.append((f"{scope}residual_layer_{i}/sublayer0/weights", F, F, a_res))
        layers.append((f"{scope}residual_layer_{i}/sublayer1/weights", F, F, a_res))
    layers.append((f"{scope}convN/weights", F, Fout_last, a_last))
    return layers


class _ResNet:
    """One ``residual_network`` (lib/graph_conv.py:305-330): conv_init, R
    residual layers of two filters each, convN, on the Chebyshev filter.  Its
    weights and gradients are the next views the owner's ``carve`` hands out,
    drawn ``truncated_normal(0, 0.1)`` from ``gen`` in creation order.

    What a net reads from its ``owner`` (a FlatTrainer), and nothing else: the
    batch and graph sizes ``N`` and ``M``, ``device``, the Chebyshev ``plan`` (the
    prepared basis ``gft`` for the Fourier net), the flat buffers through
    ``carve``, and the workspace ``ws`` / ``ws_n`` at call time.

    ``input_grad``: the input is an activation, not data (the network sits
    behind an LSTM, lib/gconv_lstm.py:382-389): conv_init's backward also
    computes dx into ``dx_in`` [N, M, Fin].  ``names`` replaces the variable
    names (same order).  ``acts``: the three activations of ``_chain`` (the
    gconv networks of lib/gconv_lstm.py:297-372 use tanh, and end a branch in ReLU)."""

    def __init__(self, owner, scope: str, Fin: int, nfilter: int, K: int, R: int, Fout_last: int, gen,
                 input_grad: bool = False, names=None, acts=ACTS):
        self.o = owner
        N, M = owner.N, owner.M
        self.Fin, self.K, self.R = Fin, K, R
        self.layers = layers = _chain(scope, Fin, nfilter, R, Fout_last, acts)
        self.names = list(names) if names is not None else [name for name, *_ in layers]
        if len(self.names) != len(layers):
            raise ValueError(f"{len(layers)} filters, {len(self.names)} names")
        self.W, self.dW = [], []
        for name, (_, fi, fo, _) in zip(self.names, layers):
            w, dw = owner.carve(self._wshape(fi, fo, K, M), name)
            truncated_normal_(w, 0.1, gen)
            self.W.append(w)
            self.dW.append(dw)
        f32 = dict(device=owner.device, dtype=torch.float32)
        self.input_grad = bool(input_grad)
        self.dx_in = torch.empty((N, M, Fin), **f32) if input_grad else None
        # activations saved by the forward, gradient work buffers
        self.out = [torch.empty((N, M, fo), **f32) for _, _, fo, _ in layers]
        self.g = [torch.empty((N, M, nfilter), **f32) for _ in range(3)]
        # a last filter with an activation: its dz, of the output's width
        self.dz_last = torch.empty((N, M, Fout_last), **f32) if layers[-1][3] != "none" else None
        self._setup(f32)

    @staticmethod
    def _wshape(fi, fo, K, M):
        return (fi * K, fo)

    @classmethod
    def sizes(cls, Fin, F, K, M, R, Fout_last):
        """Parameter counts of the filters, in creation order."""
        return [math.prod(cls._wshape(fi, fo, K, M)) for _, fi, fo, _ in _chain("", Fin, F, R, Fout_last)]

    def _setup(self, f32):
        """The filter's saved tensors and C entry points: the Chebyshev bases, in
        the planes layout where it applies, else rows."""
        o, N, M, K = self.o, self.o.N, self.o.M, self.K
        self.layout = ["planes" if o.plan.basis_elems(N, fi, K, fo, "planes") else "rows"
                       for _, fi, fo, _ in self.layers]
        self.basis = [torch.empty((K, N * M, fi) if lay == "planes" else (N * M, fi * K), **f32)
                      for (_, fi, _, _), lay in zip(self.layers, self.layout)]
        h = _lib.lib()
        self._fwd, self._bwd = h.cg_cheb_forward_layout, h.cg_cheb_backward_layout

    def ws_bytes(self):
        o = self.o
        return max(max(o.plan.workspace_bytes(o.N, fi, self.K, fo)) for _, fi, fo, _ in self.layers)

    def _f(self, li, x, res, s):
        o = self.o
        _, fi, fo, act = self.layers[li]
        st = self._fwd(o.plan.handle, o.N, fi, self.K, fo, x.data_ptr(), self.W[li].data_ptr(),
                       res.data_ptr() if res is not None else None, ops.ACTS[act],
                       _lib.BASIS_LAYOUTS[self.layout[li]], self.basis[li].data_ptr(),
                       self.out[li].data_ptr(), o.ws.data_ptr(), o.ws_n, s)
        _lib.check("cg_cheb_forward_layout", st)
        return self.out[li]

    def _b(self, li, dy, dz, dx, dx_acc, s):
        o = self.o
        _, fi, fo, act = self.layers[li]
        st = self._bwd(o.plan.handle, o.N, fi, self.K, fo, dy.data_ptr(), self.out[li].data_ptr(),
                       ops.ACTS[act], _lib.BASIS_LAYOUTS[self.layout[li]], self.basis[li].data_ptr(),
                       self.W[li].data_ptr(), dx.data_ptr() if dx is not None else None, int(dx_acc),
                       self.dW[li].data_ptr(), dz.data_ptr() if dz is not None else None,
                       o.ws.data_ptr(), o.ws_n, s)
        _lib.check("cg_cheb_backward_layout", st)

    def forward(self, x, s):
        h = self._f(0, x, None, s)
        li = 1
        for _ in range(self.R):
            t = self._f(li, h, None, s)
            h = self._f(li + 1, t, h, s)
            li += 2
        return self._f(li, h, None, s)

    def backward(self, dout, s):
        """Every dW of this network from d(out); the input gets no gradient (data)
        unless ``input_grad``: then ``dx_in`` receives it."""
        last = len(self.layers) - 1
        bufs = self.g
        dh = bufs[0]
        self._b(last, dout, self.dz_last, dh, False, s)    # convN: dh = dL/dh
        cur = 0  # bufs[cur] is dh
        li = last - 2
        for _ in range(self.R):
            dz1 = bufs[(cur + 1) % 3]
            dt = bufs[(cur + 2) % 3]
            self._b(li + 1, dh, dz1, dt, False, s)         # sublayer1: dz1 = dh*[h'>0] (= d residual)
            self._b(li, dt, dh, dz1, True, s)              # sublayer0: dz1 += dx  (dh buffer as dz0)
            dh, cur = dz1, (cur + 1) % 3
            li -= 2
        # conv_init (no dx when x is data)
        self._b(0, dh, bufs[(cur + 1) % 3], self.dx_in, False, s)


class _FourierResNet(_ResNet):
    """The same network with the Fourier filter: _ResNet's forward / backward
    schedule over cg_fres_forward / cg_fres_backward.  Weights [M, Fout, Fin]
    (lib/graph_conv.py:105); the forward saves each filter's spectrum xhat; ``K``
    is ignored.

    ``drop`` = (keep_prob, seed) or None: conv_init reads its input through a
    dropout mask folded into the transforms (cg_fres_forward_drop /
    cg_fres_backward_drop; needs ``input_grad``)."""

    drop = None

    @staticmethod
    def _wshape(fi, fo, K, M):
        return (M, fo, fi)

    def _setup(self, f32):
        self.xhat = [torch.empty((self.o.N, self.o.M, fi), **f32) for _, fi, _, _ in self.layers]
        h = _lib.lib()
        self._fwd, self._bwd = h.cg_fres_forward, h.cg_fres_backward
        self._fwd_drop, self._bwd_drop = h.cg_fres_forward_drop, h.cg_fres_backward_drop

    def ws_bytes(self):
        o = self.o
        return max(max(ops.fres_workspace_bytes(o.N, o.M, fi, fo)) for _, fi, fo, _ in self.layers)

    def _f(self, li, x, res, s):
        o = self.o
        _, fi, fo, act = self.layers[li]
        # conv_init alone reads through the mask: (keep_prob, seed) go in after x
        fn, drop = (self._fwd_drop, self.drop) if li == 0 and self.drop is not None else (self._fwd, ())
        st = fn(o.N, o.M, fi, fo, o.gft.data_ptr(), o.gft.numel(), self.W[li].data_ptr(), x.data_ptr(),
                *drop, res.data_ptr() if res is not None else None, ops.ACTS[act],
                self.xhat[li].data_ptr(), self.out[li].data_ptr(), o.ws.data_ptr(), o.ws_n, s)
        _lib.check(fn.__name__, st)
        return self.out[li]

    def _b(self, li, dy, dz, dx, dx_acc, s):
        o = self.o
        _, fi, fo, act = self.layers[li]
        grads = (dz.data_ptr() if dz is not None else None, dx.data_ptr() if dx is not None else None)
        if li == 0 and self.drop is not None:  # (keep_prob, seed, dz, dx): dx =, never +=
            fn, grads = self._bwd_drop, (*self.drop, *grads)
        else:
            fn, grads = self._bwd, (*grads, int(dx_acc))
        st = fn(o.N, o.M, fi, fo, o.gft.data_ptr(), o.gft.numel(), self.W[li].data_ptr(),
                self.xhat[li].data_ptr(), dy.data_ptr(), self.out[li].data_ptr(), ops.ACTS[act],
                *grads, self.dW[li].data_ptr(), o.ws.data_ptr(), o.ws_n, s)
        _lib.check(fn.__name__, st)


FILTERS = ("chebyshev5", "fourier")


def _net_class(filter):
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
    return _FourierResNet if filter == "fourier" else _ResNet


class _ResModel(FlatTrainer):
    """What ResGNN and StackedResGNN share: the graph (a Chebyshev plan, or U
    prepared once for the transforms) and the flat Adam trainer over ``total``
    parameters."""

    def __init__(self, L, N, nfilter, K, nres_layer_count, Fout_last, learning_rate, decay_rate,
                 decay_steps, device, comm, lmax, filter, total):
        super().__init__(total, (int(N), int(L.shape[0]), int(Fout_last)), "adam", learning_rate,
                         decay_rate, decay_steps, device, comm)
        self.filter = filter
        if filter == "fourier":  # no Chebyshev plan: U, prepared once for the transforms
            self.plan = None
            self.M = int(L.shape[0])
            self.U = _filter.fourier_basis(L, self.device)
            self.gft = ops.gft_prepare(self.U)
        else:
            dev_index = self.device.index if self.device.index is not None else 0
            self.plan = plan_for(L, lmax=lmax, device=dev_index)
            self.M = self.plan.M
        self.N, self.nfilter, self.K = int(N), int(nfilter), int(K)
        self.R, self.Fout_last = int(nres_layer_count), int(Fout_last)

    def _make_net(self, scope, Fin, gen):
        return _net_class(self.filter)(self, scope, Fin, self.nfilter, self.K, self.R, self.Fout_last, gen)


class ResGNN(_ResModel):
    """ResGNN on one graph level (the fork's active model uses ``L[0]`` everywhere)."""

    def __init__(self, L, N: int, Fin: int, nfilter: int, K: int, nres_layer_count: int,
                 Fout_last: int = 2, learning_rate: float = 1e-3, decay_rate: float = 0.95,
                 decay_steps: int | None = None, device=None, seed: int = 2017, comm=None,
                 lmax: float = 2, filter: str = "chebyshev5"):
        """filter: "chebyshev5" or "fourier" (K is then ignored, lib/graph_conv.py:103)."""
        total = sum(_net_class(filter).sizes(Fin, nfilter, K, L.shape[0], nres_layer_count, Fout_last))
        super().__init__(L, N, nfilter, K, nres_layer_count, Fout_last, learning_rate, decay_rate,
                         decay_steps, device, comm, lmax, filter, total)
        self.Fin = int(Fin)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        self.net = self._make_net("", self.Fin, gen)
        self._carved()
        self.layers = self.net.layers
        self.W, self.dW = self.net.W, self.net.dW
        # the forward's saved tensors: the Chebyshev bases, or the spectra xhat
        self.basis, self.out = getattr(self.net, "basis", None), self.net.out
        self._alloc_ws([self.net])

    def forward(self, x, stream=None):
        """residual_network (lib/graph_conv.py:305-330): returns the logits [N, M, Fout_last]."""
        s = self._stream(stream)
        if tuple(x.shape) != (self.N, self.M, self.Fin) or not x.is_cuda:
            raise ValueError(f"x must be a cuda tensor of shape {(self.N, self.M, self.Fin)}")
        return self.net.forward(x.contiguous(), s)

    def train_step(self, x, labels, stream=None):
        """One optimizer step (lib/graph_model.py:277-310); returns the device loss [1]."""
        s = self._stream(stream)
        out = self.forward(x, s)
        self._loss(out, labels, s)
        self.net.backward(self.dout, s)
        self._exchange_and_update(s)
        return self.loss


class StackedResGNN(_ResModel):
    """``GraphConv._inference`` with ``stack_num > 1`` (lib/graph_conv.py:272-303).

    ``groups`` are the channel ranges of the input fed to each residual
    network; the reference hard-codes ``x_arr[0:12]`` and ``x_arr[12:16]``
    (:284-285) for its 16-channel (8 periods x 2 flows) humanflow input.
    Variable order (= initialisation order): for each i, the network
    ``final_merge/VC_i/...`` then the merge weight ``final_merge/W_i/weights``
    [M, Fout_last]."""

    def __init__(self, L, N: int, C: int, nfilter: int, K: int, nres_layer_count: int,
                 groups=((0, 12), (12, 16)), Fout_last: int = 2, learning_rate: float = 1e-3,
                 decay_rate: float = 0.95, decay_steps: int | None = None, device=None,
                 seed: int = 2017, comm=None, lmax: float = 2, filter: str = "chebyshev5"):
        """filter: "chebyshev5" or "fourier" (K is then ignored, lib/graph_conv.py:103)."""
        net = _net_class(filter)
        groups = [(int(a), int(b)) for a, b in groups]
        if len(groups) < 1 or any(not (0 <= a < b <= C) for a, b in groups):
            raise ValueError(f"bad channel groups {groups} for C={C}")
        self.C, self.groups = int(C), groups
        M = L.shape[0]
        total = sum(sum(net.sizes(b - a, nfilter, K, M, nres_layer_count, Fout_last)) + M * Fout_last
                    for a, b in groups)
        super().__init__(L, N, nfilter, K, nres_layer_count, Fout_last, learning_rate, decay_rate,
                         decay_steps, device, comm, lmax, filter, total)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        f32 = dict(device=self.device, dtype=torch.float32)
        self.nets, self.merge_W, self.merge_dW = [], [], []
        for i, (a, b) in enumerate(groups):
            self.nets.append(self._make_net(f"final_merge/VC_{i}/", b - a, gen))
            w, dw = self.carve((self.M, self.Fout_last), f"final_merge/W_{i}/weights")
            truncated_normal_(w, 0.1, gen)
            self.merge_W.append(w)
            self.merge_dW.append(dw)
        self._carved()
        self.W, self.dW = self._tensors, self._grads
        self.x_groups = [torch.empty((self.N, self.M, b - a), **f32) if (a, b) != (0, self.C) else None
                         for a, b in groups]
        self.X = torch.empty((self.N, self.M, self.Fout_last), **f32)
        self.d_net = torch.empty((self.N, self.M, self.Fout_last), **f32)
        self._alloc_ws(self.nets)
        h = _lib.lib()
        self._slice, self._merge_f, self._merge_b = (h.cg_slice_channels, h.cg_stack_merge_forward,
                                                     h.cg_stack_merge_backward)

    def forward(self, x, stream=None):
        """_inference (lib/graph_conv.py:274-303): returns X [N, M, Fout_last]."""
        s = self._stream(stream)
        if tuple(x.shape) != (self.N, self.M, self.C) or not x.is_cuda:
            raise ValueError(f"x must be a cuda tensor of shape {(self.N, self.M, self.C)}")
        x = x.contiguous()
        N, M, F = self.N, self.M, self.Fout_last
        for i, ((a, b), net) in enumerate(zip(self.groups, self.nets)):
            xi = x
            if self.x_groups[i] is not None:
                xi = self.x_groups[i]
                _lib.check("cg_slice_channels",
                           self._slice(x.data_ptr(), N * M, self.C, a, b, xi.data_ptr(), s))
            out = net.forward(xi, s)
            _lib.check("cg_stack_merge_forward",
                       self._merge_f(N, M, F, out.data_ptr(), self.merge_W[i].data_ptr(), int(i > 0),
                                     self.X.data_ptr(), s))
        return self.X

    def train_step(self, x, labels, stream=None):
        """One optimizer step over every network and merge weight; returns the device loss [1]."""
        s = self._stream(stream)
        X = self.forward(x, s)
        self._loss(X, labels, s)
        N, M, F = self.N, self.M, self.Fout_last
        for i, net in enumerate(self.nets):
            out = net.out[-1]
            _lib.check("cg_stack_merge_backward",
                       self._merge_b(N, M, F, self.dout.data_ptr(), out.data_ptr(),
                                     self.merge_W[i].data_ptr(), self.d_net.data_ptr(),
                                     self.merge_dW[i].data_ptr(), s))
            net.backward(self.d_net, s)
        self._exchange_and_update(s)
        return self.loss
