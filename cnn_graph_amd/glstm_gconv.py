"""``GconvModel.inference_glstm_gconv`` (lib/gconv_lstm.py:374-400; the driver's
``inference_glstm_gconv_no_expand``, :402-428, is the same code line for line)
trained as ``GraphModel`` trains it -- the model nips2016/gconvTest.py runs:

  x [N, M, F*T]  --unstack time (:375-379)-->  T x [N, M, F]
  glstm_layer    layer_count GConvLSTMCells under static_rnn, each in a
                 DropoutWrapper(keep_prob) (:609-627); the last step's output
  conv_init      a   = relu(filter(h_T; W_init [H -> C]))              (:384-389)
  conv_layer_i   t   = relu(filter(a; W_i0)); a = relu(filter(t; W_i1) + a)
                 (residual_layer, :642-658), conv_layer_num times
  output_layer   out = filter(a; W_out [C -> out_features]), no activation (:395-398)
  loss / update  GLSTMModel's: cg_mse_loss_ema, ONE all-reduce of the flat
                 gradient bucket when world > 1, ONE optimizer launch

``filter`` names the reference's ``lib/filter.py`` function for the cells AND
the head.  The head's weights are created as filter.py creates them:
``tf.truncated_normal_initializer(0, 0.1)`` -- lib/filter.py:39-40 for
fourier_conv ([M, Fout, Fin]), :63-64 for cheby_conv ([K*Fin, Fout]).

The LSTM layers run as ``GLSTMModel``'s do (autograd over the layer
functions); the head is ``model._ResNet`` / ``_FourierResNet`` -- the explicit
C-ABI schedule of ResGNN -- with ``input_grad``: conv_init's backward also
computes dx, and that dx is the last LSTM layer's dh_T.

The seam (h_T -> dropout -> conv_init).  ``seam="unfused"``: ``ops.dropout`` on
h_T (the slice at element offset (T-1) N M H of the layer's mask stream), then
the plain filter calls.  ``seam="fused"`` (fourier_conv only): the mask is
folded into conv_init's transforms, cg_fres_forward_drop / cg_fres_backward_drop
-- the same bits, two passes over h_T and two launches fewer.  The Chebyshev
head is always unfused.  ``seam="auto"`` is the measured-faster one at the
driver's shape ("The LSTM -> head seam").
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from . import evaluate as _ev
from . import ops
from .gconv_lstm import (DropoutWrapper, GConvLSTMCell, _exchange_and_update, dropout_seed, layer,
                         unstack_time)
from .model import _FourierResNet, _ResNet

# what "auto" resolves to for the Fourier head (DESIGN.md has the measurement)
AUTO_SEAM = "fused"


class GLSTMGconvModel:
    """inference_glstm_gconv on device.  Every parameter -- each layer's Wx, Wh,
    b, then conv_init, the residual layers and output_layer -- is a view into one
    flat fp32 buffer, every gradient a view into one flat bucket."""

    OPTIMIZERS = ("adam", "sgd", "rmsprop")

    def __init__(self, L, N: int, T: int, feat_in: int, num_hidden: int = 128,
                 num_hidden_conv: int = 32, K: int = 2, layer_count: int = 1, conv_layer_num: int = 1,
                 out_features: int = 2, keep_prob: float = 0.8, filter: str = "cheby_conv",
                 seam: str = "auto", optimizer: str = "adam", learning_rate: float = 1e-3,
                 decay_rate: float = 0.95, decay_steps: int | None = None, lmax: float = 2,
                 gates: str = "reference", device=None, seed: int = 2017, comm=None):
        if optimizer not in self.OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {self.OPTIMIZERS}")
        if filter not in ("cheby_conv", "fourier_conv"):
            raise ValueError("filter must be 'cheby_conv' or 'fourier_conv'")
        if seam not in ("auto", "fused", "unfused"):
            raise ValueError("seam must be 'auto', 'fused' or 'unfused'")
        if not 0.0 < float(keep_prob) <= 1.0:
            raise ValueError(f"keep_prob must be in (0, 1], got {keep_prob}")
        fourier = filter == "fourier_conv"
        if seam == "fused" and not fourier:
            raise ValueError("seam='fused' folds the mask into the Fourier transforms; the "
                             "Chebyshev head is 'unfused'")
        self.filter = filter
        self.seam = (AUTO_SEAM if fourier else "unfused") if seam == "auto" else seam
        self.device = torch.device(device if device is not None else "cuda")
        self.N, self.T, self.F, self.H, self.K = int(N), int(T), int(feat_in), int(num_hidden), int(K)
        # the head's _ResNet reads these from its owner
        self.nfilter, self.R, self.Fout_last = int(num_hidden_conv), int(conv_layer_num), int(out_features)
        self.Fout = self.Fout_last
        self.keep_prob = float(keep_prob)
        self.optimizer, self.lr = optimizer, learning_rate
        self.decay_rate, self.decay_steps = decay_rate, decay_steps
        self.comm = comm
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        cells = []
        for li in range(int(layer_count)):
            fin = self.F if li == 0 else self.H
            cells.append(GConvLSTMCell(self.H, laplacian=L, lmax=lmax, K=self.K, feat_in=fin,
                                       gates=gates, device=self.device, generator=gen,
                                       filter_type=filter))
        self.M = M = cells[0]._nNode
        self.plan = None if fourier else cells[0].plan
        self.U = cells[0].U if fourier else None
        H, C, R = self.H, self.nfilter, self.R
        head_sizes = _FourierResNet.sizes(H, C, M, R, self.Fout) if fourier else \
            _ResNet.sizes(H, C, self.K, R, self.Fout)
        lstm_total = sum(c.Wx.numel() + c.Wh.numel() + c.b.numel() for c in cells)
        total = lstm_total + sum(head_sizes)
        f32 = dict(device=self.device, dtype=torch.float32)
        self.flat = torch.empty(total, **f32)
        self.grad = torch.zeros(total, **f32)
        self.names, self.params = [], []
        off = 0

        def bind(t_init, name):
            nonlocal off
            n = t_init.numel()
            view = self.flat[off:off + n].view_as(t_init)
            view.copy_(t_init)
            p = torch.nn.Parameter(view)   # aliases the flat buffer
            p.grad = self.grad[off:off + n].view_as(t_init)
            off += n
            self.names.append(name)
            self.params.append(p)
            return p

        scope = "gconv_lstm_layer/rnn/multi_rnn_cell/cell_{}/"
        for li, c in enumerate(cells):
            with torch.no_grad():
                c.Wx = bind(c.Wx.detach(), scope.format(li) + "Wx")
                c.Wh = bind(c.Wh.detach(), scope.format(li) + "Wh")
                c.b = bind(c.b.detach(), scope.format(li) + "b")
        assert off == lstm_total
        self.lstm_grad = self.grad[:lstm_total]  # what autograd accumulates into
        self.cells = cells
        head_names = ["conv_init/weights"]
        for i in range(R):
            head_names += [f"conv_layer_{i}/residual_layer_{i}/sublayer{j}/weights" for j in (0, 1)]
        head_names.append("output_layer/weights")
        h = _lib.lib()
        if fourier:
            self.gft = cells[0].gft_basis if cells[0].gft_basis is not None else ops.gft_prepare(self.U)
            self._fwd, self._bwd = h.cg_fres_forward, h.cg_fres_backward
            net = _FourierResNet
        else:
            self._fwd, self._bwd = h.cg_cheb_forward_layout, h.cg_cheb_backward_layout
            net = _ResNet
        # truncated_normal(0, 0.1) on the flat views (lib/filter.py:39, :63), after the cells' draws
        self.head = net(self, "", H, off, gen, input_grad=True, names=head_names)
        assert self.head.end == total
        self.names += self.head.names
        self.head_W, self.head_dW = self.head.W, self.head.dW
        self.ws_n = self.head.ws_bytes()
        self.ws = torch.empty(max(self.ws_n, 1), device=self.device, dtype=torch.uint8)
        # each wrapper's mask stream from (model seed, rank, layer), as GLSTMModel
        rank = int(getattr(comm, "rank", 0)) if comm is not None else 0
        self.wrapped = [DropoutWrapper(c, keep_prob, seed=dropout_seed(seed, rank, li))
                        if keep_prob < 1.0 else c for li, c in enumerate(cells)]
        # optimizer slots (TF 1.x: Adam m, v zeros; RMSProp ms ONES, mom zeros)
        self.s1 = (torch.ones if optimizer == "rmsprop" else torch.zeros)(total, **f32)
        self.s2 = torch.zeros(total, **f32)
        self.loss = torch.empty((1,), **f32)
        self.ema = torch.zeros((3,), **f32)  # ExponentialMovingAverage(0.9) of the loss
        self.dout = torch.empty((self.N, M, self.Fout), **f32)
        nb = ctypes.c_size_t()
        _lib.call("cg_mse_loss_workspace_bytes", self.N * M * self.Fout, ctypes.byref(nb))
        self.mws = torch.empty(max(nb.value, 1), device=self.device, dtype=torch.uint8)
        self.mws_n = nb.value
        self.step_count = 0
        self._h = None

    @property
    def world(self):
        return self.comm.world if self.comm is not None else 1

    @property
    def loss_average(self):
        return self.ema[1:2]

    def parameters(self):
        return dict(zip(self.names, self.params + self.head_W))

    def gradients(self):
        return dict(zip(self.names, [p.grad for p in self.params] + self.head_dW))

    def learning_rate(self, step):
        """tf.train.exponential_decay(lr, global_step, decay_steps, decay_rate, staircase=True)."""
        if self.decay_rate == 1 or not self.decay_steps:
            return self.lr
        return self.lr * self.decay_rate ** math.floor(step / self.decay_steps)

    def _stream(self, stream):
        return stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream

    def forward(self, x, stream=None, dropout: bool = True):
        """The output layer's [N, M, out_features] (a buffer the next forward
        overwrites).  x: [N, M, F*T] as the reference feeds it, or [T, N, M, F].
        ``dropout=False`` runs every layer unwrapped.  ``backward`` continues
        from the state this call leaves."""
        s = self._stream(stream)
        xs = unstack_time(x, self.T) if x.dim() == 3 else x.contiguous()
        if tuple(xs.shape) != (self.T, self.N, self.M, self.F) or not xs.is_cuda:
            raise ValueError(f"x must be a cuda tensor of [N, M, F*T] = {(self.N, self.M, self.F * self.T)}")
        last = len(self.cells) - 1
        for li in range(last):
            cell = self.wrapped[li] if dropout else self.cells[li]
            xs, _ = layer(cell, xs, final_c=False)
        # the last layer runs unwrapped and is read at its last step only
        _, st = layer(self.cells[last], xs, final_c=False)
        h = hd = st.h
        w = self.wrapped[last]
        self.head.drop = None
        if dropout and isinstance(w, DropoutWrapper):
            # the last-step slice of the layer's mask: element offset (T-1) N M H
            seed, off = w.next_seed(), (self.T - 1) * h.numel()
            if self.seam == "fused":
                self.head.drop = (w.output_keep_prob, (seed + ops.DROP_WEYL * off) & ((1 << 64) - 1))
            else:
                hd = ops.dropout(h, w.output_keep_prob, seed, offset=off)
        self._h = hd  # what conv_init read (through the mask when fused)
        return self.head.forward(hd.detach().contiguous(), s)

    def backward(self, dout, stream=None):
        """Every gradient of the last forward from d(out) [N, M, out_features]: the
        head's explicit schedule (its dW written into the bucket), conv_init's
        dx -- already through the mask when the seam is fused -- as dh_T of the
        LSTM, whose layers accumulate into the (zeroed) bucket through autograd;
        an input that requires grad gets its ``.grad``."""
        s = self._stream(stream)
        self.lstm_grad.zero_()
        self.head.backward(dout.contiguous(), s)
        if self._h is not None and self._h.requires_grad:
            self._h.backward(self.head.dx_in)
        self._h = None

    def train_step(self, x, labels, stream=None):
        """One optimizer step; returns the device loss [1] (this rank's batch)."""
        s = self._stream(stream)
        out = self.forward(x, stream)
        labels = labels.contiguous()
        if labels.numel() != out.numel():
            raise ValueError("labels must match the logits' shape")
        _lib.call("cg_mse_loss_ema", out.data_ptr(), labels.data_ptr(), out.numel(),
                  self.loss.data_ptr(), self.dout.data_ptr(), self.ema.data_ptr(),
                  ctypes.c_float(0.9), self.mws.data_ptr(), self.mws_n, s)
        self.backward(self.dout, stream)
        _exchange_and_update(self, s)
        return self.loss

    def predict(self, data, labels=None, reference_dropout: bool = False):
        """GraphModel.predict (lib/graph_model.py:64-94; evaluate.predict has the
        padding and the ``loss * batch_size / size`` quirk, padded rows
        included): data [size, M, F*T] -> predictions [size, M, out_features],
        with labels also the loss.  Parameters, optimizer slots, the loss
        average and the step count are untouched.

        Dropout at evaluation: the reference's DropoutWrapper(0.8) inside
        glstm_layer (lib/gconv_lstm.py:616, :623) is a constant of the graph, so
        the reference ALSO drops when it evaluates.  The default here is no
        dropout (deterministic predictions); ``reference_dropout=True`` applies
        the wrappers' masks as a training forward does (and advances their
        mask streams)."""
        return _ev.predict(lambda b: self.forward(b, dropout=reference_dropout), self.N, self.device,
                           data, labels)

    def evaluate(self, data, labels, reference_dropout: bool = False):
        """GraphModel.evaluate (lib/graph_model.py:96-122):
        (string, mse, 0, loss, predictions)."""
        return _ev.evaluate(lambda d, l: self.predict(d, l, reference_dropout), data, labels)
