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

from . import ops
from .gconv_lstm import LSTMStackTrainer, lstm_to_hT
from .model import LSTMHead, _net_class
from .trainer import check_keep_prob, check_seam

# what "auto" resolves to for the Fourier head (DESIGN.md has the measurement)
AUTO_SEAM = "fused"


class GLSTMGconvModel(LSTMHead, LSTMStackTrainer):
    """inference_glstm_gconv on device.  Every parameter -- each layer's Wx, Wh,
    b, then conv_init, the residual layers and output_layer -- is a view into one
    flat fp32 buffer, every gradient a view into one flat bucket."""

    def __init__(self, L, N: int, T: int, feat_in: int, num_hidden: int = 128,
                 num_hidden_conv: int = 32, K: int = 2, layer_count: int = 1, conv_layer_num: int = 1,
                 out_features: int = 2, keep_prob: float = 0.8, filter: str = "cheby_conv",
                 seam: str = "auto", optimizer: str = "adam", learning_rate: float = 1e-3,
                 decay_rate: float = 0.95, decay_steps: int | None = None, lmax: float = 2,
                 gates: str = "reference", device=None, seed: int = 2017, comm=None):
        check_seam(seam)
        self.keep_prob = check_keep_prob(keep_prob)
        fourier = filter == "fourier_conv"
        if seam == "fused" and not fourier:
            raise ValueError("seam='fused' folds the mask into the Fourier transforms; the "
                             "Chebyshev head is 'unfused'")
        self.seam = (AUTO_SEAM if fourier else "unfused") if seam == "auto" else seam
        H, C, R, Fout = int(num_hidden), int(num_hidden_conv), int(conv_layer_num), int(out_features)
        self.R = R
        super().__init__(L, N, T, feat_in, num_hidden, K, layer_count, out_features, keep_prob, filter,
                         sum(_net_class(fourier).sizes(H, C, int(K), int(L.shape[0]), R, Fout)), optimizer,
                         learning_rate, decay_rate, decay_steps, lmax, gates, device, seed, comm, head=True)
        self._make_head(fourier, H, C, R, Fout, self._gen)
        self._carved()

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
        drop = None
        if mask is not None:
            keep, seed, off = mask
            if self.seam == "fused":  # conv_init reads h_T through the mask
                drop = (keep, (seed + ops.DROP_WEYL * off) & ((1 << 64) - 1))
            else:
                h = ops.dropout(h, keep, seed, offset=off)
        self.head.filters[0].drop = drop
        return self._head_forward(h, s)

    def backward(self, dout, stream=None):
        """Every gradient of the last forward from d(out) [N, M, out_features]: the
        head's explicit schedule (its dW written into the bucket), conv_init's
        dx -- already through the mask when the seam is fused -- as dh_T of the
        LSTM, whose layers accumulate into the (zeroed) bucket through autograd;
        an input that requires grad gets its ``.grad``."""
        self._head_backward(dout, self._stream(stream))
