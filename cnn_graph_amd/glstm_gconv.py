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
  loss / update  FlatTrainer's: cg_mse_loss_ema, ONE all-reduce of the flat
                 gradient bucket when world > 1, ONE optimizer launch

``filter`` names the reference's ``lib/filter.py`` function for the cells AND
the head.  The head's weights are created as filter.py creates them:
``tf.truncated_normal_initializer(0, 0.1)`` -- lib/filter.py:39-40 for
fourier_conv ([M, Fout, Fin]), :63-64 for cheby_conv ([K*Fin, Fout]).

The LSTM layers are ``gconv_lstm.LSTMStackTrainer``'s, shared with ``GLSTMModel``
(autograd over the layer functions, ``lstm_to_hT``); the head is
``model._ResNet`` / ``_FourierResNet`` -- the explicit C-ABI schedule of
ResGNN -- with ``input_grad``: conv_init's backward also computes dx, and that
dx is the last LSTM layer's dh_T.

The seam (h_T -> dropout -> conv_init).  ``seam="unfused"``: ``ops.dropout`` on
h_T (the slice at element offset (T-1) N M H of the layer's mask stream), then
the plain filter calls.  ``seam="fused"`` (fourier_conv only): the mask is
folded into conv_init's transforms, cg_fres_forward_drop / cg_fres_backward_drop
-- the same bits, two passes over h_T and two launches fewer.  The Chebyshev
head is always unfused.  ``seam="auto"`` is the measured-faster one at the
driver's shape ("The LSTM -> head seam").
"""
from __future__ import annotations

import torch

from . import ops
from .gconv_lstm import LSTMStackTrainer, lstm_to_hT
from .model import _FourierResNet, _ResNet

# what "auto" resolves to for the Fourier head (DESIGN.md has the measurement)
AUTO_SEAM = "fused"


class GLSTMGconvModel(LSTMStackTrainer):
    """inference_glstm_gconv on device.  Every parameter -- each layer's Wx, Wh,
    b, then conv_init, the residual layers and output_layer -- is a view into one
    flat fp32 buffer, every gradient a view into one flat bucket."""

    def __init__(self, L, N: int, T: int, feat_in: int, num_hidden: int = 128,
                 num_hidden_conv: int = 32, K: int = 2, layer_count: int = 1, conv_layer_num: int = 1,
                 out_features: int = 2, keep_prob: float = 0.8, filter: str = "cheby_conv",
                 seam: str = "auto", optimizer: str = "adam", learning_rate: float = 1e-3,
                 decay_rate: float = 0.95, decay_steps: int | None = None, lmax: float = 2,
                 gates: str = "reference", device=None, seed: int = 2017, comm=None):
        if seam not in ("auto", "fused", "unfused"):
            raise ValueError("seam must be 'auto', 'fused' or 'unfused'")
        if not 0.0 < float(keep_prob) <= 1.0:
            raise ValueError(f"keep_prob must be in (0, 1], got {keep_prob}")
        fourier = filter == "fourier_conv"
        if seam == "fused" and not fourier:
            raise ValueError("seam='fused' folds the mask into the Fourier transforms; the "
                             "Chebyshev head is 'unfused'")
        self.seam = (AUTO_SEAM if fourier else "unfused") if seam == "auto" else seam
        self.keep_prob = float(keep_prob)
        H, C, R, Fout = int(num_hidden), int(num_hidden_conv), int(conv_layer_num), int(out_features)
        self.R = R
        net = _FourierResNet if fourier else _ResNet
        super().__init__(L, N, T, feat_in, num_hidden, K, layer_count, out_features, keep_prob, filter,
                         sum(net.sizes(H, C, int(K), int(L.shape[0]), R, Fout)), optimizer,
                         learning_rate, decay_rate, decay_steps, lmax, gates, device, seed, comm)
        self.lstm_grad = self.grad[:self._off]  # what autograd accumulates into
        head_names = ["conv_init/weights"]
        for i in range(R):
            head_names += [f"conv_layer_{i}/residual_layer_{i}/sublayer{j}/weights" for j in (0, 1)]
        head_names.append("output_layer/weights")
        if fourier:
            c0 = self.cells[0]
            self.gft = c0.gft_basis if c0.gft_basis is not None else ops.gft_prepare(self.U)
        # truncated_normal(0, 0.1) on the flat views (lib/filter.py:39, :63), after the cells' draws
        self.head = net(self, "", H, C, self.K, R, Fout, self._gen, input_grad=True, names=head_names)
        self._carved()
        self.head_W, self.head_dW = self.head.W, self.head.dW
        self._alloc_ws([self.head])
        self._h = None

    def forward(self, x, stream=None, dropout: bool = True):
        """The output layer's [N, M, out_features] (a buffer the next forward
        overwrites).  x: [N, M, F*T] as the reference feeds it, or [T, N, M, F].
        ``dropout=False`` runs every layer unwrapped.  ``backward`` continues
        from the state this call leaves."""
        s = self._stream(stream)
        xs = self._steps(x)
        if tuple(xs.shape) != (self.T, self.N, self.M, self.F) or not xs.is_cuda:
            raise ValueError(f"x must be a cuda tensor of [N, M, F*T] = {(self.N, self.M, self.F * self.T)}")
        h, mask = lstm_to_hT(self.cells, self.wrapped, xs, dropout)
        self.head.drop = None
        if mask is not None:
            keep, seed, off = mask
            if self.seam == "fused":
                self.head.drop = (keep, (seed + ops.DROP_WEYL * off) & ((1 << 64) - 1))
            else:
                h = ops.dropout(h, keep, seed, offset=off)
        self._h = h  # what conv_init read (through the mask when fused)
        return self.head.forward(h.detach().contiguous(), s)

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
        self._loss(out, labels, s)
        self.backward(self.dout, stream)
        self._exchange_and_update(s)
        return self.loss
