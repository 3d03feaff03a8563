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
from . import ops
from .graph_conv import truncated_normal_
from .trainer import FlatTrainer, is_fourier


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


def head_names(conv_layer_num: int, suffix: str = ""):
    """The variable names of a gconv network of lib/gconv_lstm.py (:297-400, :431-607)
    in creation order: conv_init, the residual layers, output_layer; ``suffix``
    (``_{j}``) marks branch j's scopes."""
    names = [f"conv_init{suffix}/weights"]
    for i in range(conv_layer_num):
        names += [f"conv_layer_{i}{suffix}/residual_layer_{i}/sublayer{k}/weights" for k in (0, 1)]
    return names + [f"output_layer{suffix}/weights"]


class _ChebFilter:
    """ONE Chebyshev filter of a device model: its forward and backward C-ABI
    calls and the basis saved between them -- in the planes layout where it
    applies, else rows (``layout`` overrides the choice).  ``W``, ``dW`` and ``out``
    are the caller's; the plan and the workspace are the ``owner``'s (a FlatTrainer),
    unless ``plan`` (with its vertex count ``M``) names this filter's own graph:
    a level of the cgcnn pyramid."""

    def __init__(self, owner, fi, fo, K, act, W, dW, out, layout=None, plan=None, M=None):
        N = owner.N
        plan = owner.plan if plan is None else plan
        M = owner.M if M is None else int(M)
        self.o, self.W, self.dW, self.out, self.plan = owner, W, dW, out, plan
        self.dims, self.act = (plan.handle, N, fi, K, fo), ops.ACTS[act]
        if layout is None:
            layout = "planes" if plan.basis_elems(N, fi, K, fo, "planes") else "rows"
        self.layout, self._layout = layout, _lib.BASIS_LAYOUTS[layout]
        self.basis = torch.empty((K, N * M, fi) if layout == "planes" else (N * M, fi * K),
                                 device=owner.device, dtype=torch.float32)
        h = _lib.lib()
        self._fwd, self._bwd = h.cg_cheb_forward_layout, h.cg_cheb_backward_layout

    wshape = staticmethod(lambda fi, fo, K, M: (fi * K, fo))

    def ws_bytes(self):
        return max(self.plan.workspace_bytes(*self.dims[1:]))

    def forward(self, x, res, s):
        """out = act(filter(x; W) + res)."""
        o = self.o
        st = self._fwd(*self.dims, x.data_ptr(), self.W.data_ptr(),
                       res.data_ptr() if res is not None else None, self.act, self._layout,
                       self.basis.data_ptr(), self.out.data_ptr(), o.ws.data_ptr(), o.ws_n, s)
        _lib.check("cg_cheb_forward_layout", st)
        return self.out

    def backward(self, dy, dz, dx, dx_acc, s):
        """dW, and where given dz (= dy through the activation) and dx (+= with ``dx_acc``)."""
        o = self.o
        st = self._bwd(*self.dims, dy.data_ptr(), self.out.data_ptr(), self.act, self._layout,
                       self.basis.data_ptr(), self.W.data_ptr(), dx.data_ptr() if dx is not None else None,
                       int(dx_acc), self.dW.data_ptr(), dz.data_ptr() if dz is not None else None,
                       o.ws.data_ptr(), o.ws_n, s)
        _lib.check("cg_cheb_backward_layout", st)


class _FourierFilter:
    """The same unit on the MFMA transforms (cg_fres_forward / cg_fres_backward):
    weights [M, Fout, Fin] (lib/graph_conv.py:105), the saved tensor is the
    spectrum xhat, the owner's prepared basis ``gft`` is read at call time; ``K``
    is ignored.

    ``drop`` = (keep_prob, seed) or None: the filter reads its input through a
    dropout mask folded into the transforms (cg_fres_forward_drop /
    cg_fres_backward_drop; its dx is then written, never accumulated)."""

    drop = None

    def __init__(self, owner, fi, fo, K, act, W, dW, out, layout=None):
        self.o, self.W, self.dW, self.out = owner, W, dW, out
        self.dims, self.act = (owner.N, owner.M, fi, fo), ops.ACTS[act]
        self.xhat = torch.empty((owner.N, owner.M, fi), device=owner.device, dtype=torch.float32)
        h = _lib.lib()
        self._fwd, self._bwd = h.cg_fres_forward, h.cg_fres_backward
        self._fwd_drop, self._bwd_drop = h.cg_fres_forward_drop, h.cg_fres_backward_drop

    wshape = staticmethod(lambda fi, fo, K, M: (M, fo, fi))

    def ws_bytes(self):
        return max(ops.fres_workspace_bytes(*self.dims))

    def forward(self, x, res, s):
        o = self.o
        # through the mask: (keep_prob, seed) go in after x
        fn, drop = (self._fwd_drop, self.drop) if self.drop is not None else (self._fwd, ())
        st = fn(*self.dims, o.gft.data_ptr(), o.gft.numel(), self.W.data_ptr(), x.data_ptr(), *drop,
                res.data_ptr() if res is not None else None, self.act, self.xhat.data_ptr(),
                self.out.data_ptr(), o.ws.data_ptr(), o.ws_n, s)
        _lib.check(fn.__name__, st)
        return self.out

    def backward(self, dy, dz, dx, dx_acc, s):
        o = self.o
        grads = (dz.data_ptr() if dz is not None else None, dx.data_ptr() if dx is not None else None)
        if self.drop is not None:  # (keep_prob, seed, dz, dx): dx =, never +=
            fn, grads = self._bwd_drop, (*self.drop, *grads)
        else:
            fn, grads = self._bwd, (*grads, int(dx_acc))
        st = fn(*self.dims, o.gft.data_ptr(), o.gft.numel(), self.W.data_ptr(), self.xhat.data_ptr(),
                dy.data_ptr(), self.out.data_ptr(), self.act, *grads, self.dW.data_ptr(),
                o.ws.data_ptr(), o.ws_n, s)
        _lib.check(fn.__name__, st)


class _ResNet:
    """One ``residual_network`` (lib/graph_conv.py:305-330): conv_init, R
    residual layers of two filters each, convN: ``filters``, one ``_ChebFilter``
    each.  Its weights and gradients are the next views the owner's ``carve``
    hands out, drawn ``truncated_normal(0, 0.1)`` from ``gen`` in creation order.

    What a net and its filters read from the ``owner`` (a FlatTrainer), and
    nothing else: the batch and graph sizes ``N`` and ``M``, ``device``, the
    Chebyshev ``plan`` (the prepared basis ``gft`` for the Fourier net), the flat
    buffers through ``carve``, and the workspace ``ws`` / ``ws_n`` at call time.

    ``input_grad``: the input is an activation, not data (the network sits
    behind an LSTM, lib/gconv_lstm.py:382-389): conv_init's backward also
    computes dx into ``dx_in`` [N, M, Fin].  ``names`` replaces the variable
    names (same order).  ``acts``: the three activations of ``_chain`` (the
    gconv networks of lib/gconv_lstm.py:297-372 use tanh, and end a branch in ReLU)."""

    Filter = _ChebFilter

    def __init__(self, owner, scope: str, Fin: int, nfilter: int, K: int, R: int, Fout_last: int, gen,
                 input_grad: bool = False, names=None, acts=ACTS):
        self.o = owner
        N, M = owner.N, owner.M
        self.Fin, self.K, self.R = Fin, K, R
        self.layers = layers = _chain(scope, Fin, nfilter, R, Fout_last, acts)
        self.names = list(names) if names is not None else [name for name, *_ in layers]
        if len(self.names) != len(layers):
            raise ValueError(f"{len(layers)} filters, {len(self.names)} names")
        f32 = dict(device=owner.device, dtype=torch.float32)
        self.W, self.dW, self.out, self.filters = [], [], [], []
        for name, (_, fi, fo, act) in zip(self.names, layers):
            w, dw = owner.carve(self.Filter.wshape(fi, fo, K, M), name)
            truncated_normal_(w, 0.1, gen)
            self.W.append(w)
            self.dW.append(dw)
            self.out.append(torch.empty((N, M, fo), **f32))  # saved by the forward
            self.filters.append(self.Filter(owner, fi, fo, K, act, w, dw, self.out[-1]))
        self.input_grad = bool(input_grad)
        self.dx_in = torch.empty((N, M, Fin), **f32) if input_grad else None
        # gradient work buffers
        self.g = [torch.empty((N, M, nfilter), **f32) for _ in range(3)]
        # a last filter with an activation: its dz, of the output's width
        self.dz_last = torch.empty((N, M, Fout_last), **f32) if layers[-1][3] != "none" else None

    # the filters' saved tensors: the Chebyshev bases and their layouts
    layout = property(lambda self: [f.layout for f in self.filters])
    basis = property(lambda self: [f.basis for f in self.filters])

    @classmethod
    def sizes(cls, Fin, F, K, M, R, Fout_last):
        """Parameter counts of the filters, in creation order."""
        return [math.prod(cls.Filter.wshape(fi, fo, K, M))
                for _, fi, fo, _ in _chain("", Fin, F, R, Fout_last)]

    def ws_bytes(self):
        return max(f.ws_bytes() for f in self.filters)

    def _f(self, li, x, res, s):
        return self.filters[li].forward(x, res, s)

    def _b(self, li, dy, dz, dx, dx_acc, s):
        self.filters[li].backward(dy, dz, dx, dx_acc, s)

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
    schedule over ``_FourierFilter``s; the forward saves each filter's spectrum
    xhat.  ``filters[0].drop`` folds a dropout mask into conv_init's transforms
    (needs ``input_grad``)."""

    Filter = _FourierFilter
    layout = basis = None
    xhat = property(lambda self: [f.xhat for f in self.filters])


def _net_class(fourier: bool):
    return _FourierResNet if fourier else _ResNet


class _ChannelSplit:
    """The channel ranges [a, b) of an input [N, M, C] as contiguous tensors: one
    pre-allocated buffer (``bufs``) and one cg_slice_channels launch per range; a
    range that is all of x is x itself (buffer None, no launch)."""

    def __init__(self, owner, C, ranges):
        N, M = owner.N, owner.M
        self.rows, self.C, self.ranges = N * M, int(C), list(ranges)
        self.bufs = [torch.empty((N, M, b - a), device=owner.device, dtype=torch.float32)
                     if (a, b) != (0, self.C) else None for a, b in self.ranges]
        self._slice = _lib.lib().cg_slice_channels

    def slices(self, x, s):
        """Yields the ranges of x in turn.  A range's launch is enqueued when it is
        drawn: a loop that draws one slice per pass keeps slice and consumer in order."""
        for (a, b), buf in zip(self.ranges, self.bufs):
            if buf is not None:
                _lib.check("cg_slice_channels",
                           self._slice(x.data_ptr(), self.rows, self.C, a, b, buf.data_ptr(), s))
            yield x if buf is None else buf


class LSTMHead:
    """The LSTM -> head seam, a mixin for a FlatTrainer whose LSTM layers (autograd,
    carved first) feed a residual gconv network (``head``: a ``_ResNet`` with
    ``input_grad``, the explicit schedule)."""

    head = _head_in = None

    def _make_head(self, fourier, Fin, width, R, Fout, gen):
        # truncated_normal(0, 0.1) on the flat views (lib/filter.py:39, :63), after the cells' draws
        self.lstm_grad = self.grad[:self._off]  # what autograd accumulates into
        self.head = _net_class(fourier)(self, "", Fin, width, self.K, R, Fout, gen, input_grad=True,
                                        names=head_names(R))
        self.head_W, self.head_dW = self.head.W, self.head.dW
        self._alloc_ws([self.head])

    def _head_forward(self, a, s):
        """The head's output on ``a``, the end of the autograd part."""
        self._head_in = a
        return self.head.forward(a.detach().contiguous(), s)

    def _head_backward(self, dout, s):
        """The LSTM part of the bucket zeroed, the head's explicit schedule (its dW
        written into the bucket), then conv_init's dx into autograd, whose layers
        accumulate into the bucket."""
        self.lstm_grad.zero_()
        self.head.backward(dout.contiguous(), s)
        a, self._head_in = self._head_in, None
        if a is not None and a.requires_grad:
            a.backward(self.head.dx_in)


class _ResModel(FlatTrainer):
    """What ResGNN and StackedResGNN share: the graph (``_set_graph``) and the
    flat Adam trainer over ``total`` parameters."""

    def __init__(self, L, N, nfilter, K, nres_layer_count, Fout_last, learning_rate, decay_rate,
                 decay_steps, device, comm, lmax, filter, total):
        super().__init__(total, (int(N), int(L.shape[0]), int(Fout_last)), "adam", learning_rate,
                         decay_rate, decay_steps, device, comm)
        self.filter = filter
        self._set_graph(L, filter == "fourier", lmax)
        self.N, self.nfilter, self.K = int(N), int(nfilter), int(K)
        self.R, self.Fout_last = int(nres_layer_count), int(Fout_last)

    def _make_net(self, scope, Fin, gen):
        net = _net_class(self.filter == "fourier")
        return net(self, scope, Fin, self.nfilter, self.K, self.R, self.Fout_last, gen)


class ResGNN(_ResModel):
    """ResGNN on one graph level (the fork's active model uses ``L[0]`` everywhere)."""

    def __init__(self, L, N: int, Fin: int, nfilter: int, K: int, nres_layer_count: int,
                 Fout_last: int = 2, learning_rate: float = 1e-3, decay_rate: float = 0.95,
                 decay_steps: int | None = None, device=None, seed: int = 2017, comm=None,
                 lmax: float = 2, filter: str = "chebyshev5"):
        """filter: "chebyshev5" or "fourier" (K is then ignored, lib/graph_conv.py:103)."""
        net = _net_class(is_fourier(filter))
        total = sum(net.sizes(Fin, nfilter, K, L.shape[0], nres_layer_count, Fout_last))
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

    def backward(self, dout, stream=None):
        """Every dW of the last forward from d(out)."""
        self.net.backward(dout, self._stream(stream))


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
        net = _net_class(is_fourier(filter))
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
        self.split = _ChannelSplit(self, self.C, groups)
        self.X = torch.empty((self.N, self.M, self.Fout_last), **f32)
        self.d_net = torch.empty((self.N, self.M, self.Fout_last), **f32)
        self._alloc_ws(self.nets)
        h = _lib.lib()
        self._merge_f, self._merge_b = h.cg_stack_merge_forward, h.cg_stack_merge_backward

    def forward(self, x, stream=None):
        """_inference (lib/graph_conv.py:274-303): returns X [N, M, Fout_last]."""
        s = self._stream(stream)
        if tuple(x.shape) != (self.N, self.M, self.C) or not x.is_cuda:
            raise ValueError(f"x must be a cuda tensor of shape {(self.N, self.M, self.C)}")
        x = x.contiguous()
        N, M, F = self.N, self.M, self.Fout_last
        for i, (net, xi) in enumerate(zip(self.nets, self.split.slices(x, s))):
            out = net.forward(xi, s)
            _lib.check("cg_stack_merge_forward",
                       self._merge_f(N, M, F, out.data_ptr(), self.merge_W[i].data_ptr(), int(i > 0),
                                     self.X.data_ptr(), s))
        return self.X

    def backward(self, dout, stream=None):
        """Every network's and merge weight's gradient of the last forward from d(X)."""
        s = self._stream(stream)
        N, M, F = self.N, self.M, self.Fout_last
        for i, net in enumerate(self.nets):
            _lib.check("cg_stack_merge_backward",
                       self._merge_b(N, M, F, dout.data_ptr(), net.out[-1].data_ptr(),
                                     self.merge_W[i].data_ptr(), self.d_net.data_ptr(),
                                     self.merge_dW[i].data_ptr(), s))
            net.backward(self.d_net, s)
