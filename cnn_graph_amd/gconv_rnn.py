"""``lib/gconvRNN.py::Model`` with ``model_type='glstm'``: the structured-sequence
gconv-LSTM that predicts at EVERY time step and is trained with a softmax
cross-entropy over the vertices ("which vertex comes next").

  x [N, M, feat_in, T]  --unstack axis 3 (:264-267)-->  T x [N, M, feat_in]
  cell      ONE gconvLSTMCell (tanh / sigmoid gates, cheby_conv) in a
            DropoutWrapper(output_keep_prob=0.8) under static_rnn (:287-300)
  head      per step reshape(h_t, [-1, H]) @ weight + bias, reshaped to
            [-1, M, 1] and concatenated to pred_out [N, M, T] (:306-317)
  labels    [N, T] int64, one target vertex per step (:271-274)
  loss      sparse_softmax_cross_entropy_with_logits per step (:328-330), then
            reduce_sum(list of T [N] tensors, axis=1) -- a sum over the BATCH --
            and reduce_mean over time (:331-332): loss = (1/T) sum_t sum_n ce.
            That is what the code executes, whatever ``loss_batchmean`` says.
  optim     sgd / adam / rmsprop at a constant learning rate; max_grad_norm
            clips per variable with tf.clip_by_norm + tf.check_numerics
            (:381-409)

Two quirks of the reference, restated here:
  * the head weight is declared [num_hidden * num_kernel, feat_out] (:292), which
    only multiplies the [.., num_hidden] outputs for num_kernel = 1, and the
    reshape to [-1, M, 1] (:311) only makes sense for feat_out = 1.  Here the
    head is ``w`` [H, 1] and ``b`` [1] for every K.
  * the scalar bias shifts every vertex's logit alike, so the softmax does not
    see it and its exact gradient is 0.  ``db`` is still the plain sum of
    dlogit -- rounding noise, as it is in TF.

On device the head, the loss and their gradients are ONE pass over the layer's
[T, N, M, H] output (``ops.seq_xent_call`` -> cg_seq_xent_head; DESIGN.md, "The
per-step softmax head").  ``seam`` says where the DropoutWrapper's mask is
applied: "unfused" runs ``layer(wrapped, xs)`` (ops.dropout, a read and a write
of hs, and its backward) and the head with keep = 1; "fused" runs the cell
unwrapped and hands (keep, seed) to the head, which masks the values it loads
and the gradient it stores -- the same bits.  "auto" is ``AUTO_SEAM``.

Data parallel: the loss is a SUM over the batch, so the ranks' gradients add:
one all-reduce(sum) of the bucket and grad_scale = 1 (not 1/world).  The clip
runs on the exchanged gradient, before the update.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .gconv_lstm import LSTMStackTrainer, layer
from .trainer import FlatTrainer, check_keep_prob, check_seam

# what seam="auto" resolves to ("The per-step softmax head": the rule
# and the measurement)
AUTO_SEAM = "fused"


class GConvRNNModel(LSTMStackTrainer):
    """gconvRNN.Model(model_type='glstm') on device.  Parameters, in the flat
    buffer's order: the cell's Wx [K*feat_in, 4H], Wh [K*H, 4H], b [4H]
    (uniform(-0.1, 0.1), :145-161; glorot-uniform biases), then the head's
    ``w`` [H, 1] and ``b`` [1] (random_normal(0, 1), :291-293)."""

    def __init__(self, L, N: int, T: int, feat_in: int, num_hidden: int = 32, K: int = 3,
                 keep_prob: float = 0.8, seam: str = "auto", optimizer: str = "sgd",
                 learning_rate: float = 1e-3, max_grad_norm: float | None = None, lmax: float = 2,
                 filter: str = "cheby_conv", layer_count: int = 1, hconv: str = "auto", device=None,
                 seed: int = 2017, comm=None):
        self.seam = AUTO_SEAM if check_seam(seam) == "auto" else seam
        self.keep_prob = check_keep_prob(keep_prob)
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm must be positive (or None)")
        H = int(num_hidden)
        # constant learning rate: decay_rate = 1 (the reference's optimizers take a float)
        super().__init__(L, N, T, feat_in, H, K, layer_count, 1, keep_prob, filter, H + 1, optimizer,
                         learning_rate, 1, None, lmax, "standard", device, seed, comm, hconv=hconv)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        f32 = dict(device=self.device, dtype=torch.float32)
        w0 = torch.empty((H, 1), **f32).normal_(0.0, 1.0, generator=self._gen)
        b0 = torch.empty((1,), **f32).normal_(0.0, 1.0, generator=self._gen)
        self.w, self.dw = self.carve((H, 1), "gconv_model/weight", init=w0)
        self.b, self.db = self.carve((1,), "gconv_model/bias", init=b0)
        self._carved()
        self.loss_scale = 1.0 / self.T
        self.xws, _ = ops._workspace("cg_seq_xent_workspace_bytes", self.T, self.N, self.M, H,
                                     device=self.device)
        self._no_labels = torch.zeros((self.T, self.N), device=self.device, dtype=torch.int32)

    # -- FlatTrainer's hooks -------------------------------------------------------
    def _grad_scale(self, world):
        return 1.0  # the loss sums over the batch: the ranks' gradients add

    def _after_exchange(self, s):
        if self.max_grad_norm is not None:  # per variable, then check_numerics (:392-402)
            ops.clip_by_norm_(self._grads, self.max_grad_norm, check_numerics=True)

    # -- pieces ----------------------------------------------------------------------
    def _steps(self, x):
        """[N, M, feat_in, T] (or its [N, M, feat_in*T] view) -> [T, N, M, feat_in]."""
        if x.dim() == 4:
            x = x.reshape(x.shape[0], x.shape[1], -1)
        if tuple(x.shape) != (self.N, self.M, self.F * self.T) or not x.is_cuda:
            raise ValueError(f"x must be a cuda tensor of [N, M, feat_in, T] = "
                             f"{(self.N, self.M, self.F, self.T)}")
        return super()._steps(x)

    def _labels(self, labels):
        """[N, T] target vertices -> the head's [T, N] int32 device tensor."""
        if isinstance(labels, torch.Tensor) and labels.is_cuda:
            lab = labels.t()
        else:
            lab = np.asarray(labels.numpy() if isinstance(labels, torch.Tensor) else labels).T
        if tuple(lab.shape) != (self.T, self.N):
            raise ValueError(f"labels must be [N, T] = {(self.N, self.T)}")
        return ops.seq_xent_labels(lab, self.M, self.device)

    def _sequence(self, xs, dropout: bool):
        """The last layer's outputs hs [T, N, M, H] and the (keep, seed) still to
        be applied to them by the head (None: nothing left to apply)."""
        last = len(self.cells) - 1
        for li in range(last):
            xs, _ = layer(self.wrapped[li] if dropout else self.cells[li], xs, final_c=False)
        w = self.wrapped[last]
        if not dropout or w is self.cells[last]:
            return layer(self.cells[last], xs, final_c=False)[0], None
        if self.seam == "fused":
            return layer(self.cells[last], xs, final_c=False)[0], (w.output_keep_prob, w.next_seed())
        return layer(w, xs, final_c=False)[0], None

    def _head(self, hs, lab, mask, need_grad: bool, want_logits: bool):
        keep, seed = mask if mask is not None else (1.0, 0)
        return ops.seq_xent_call(hs.detach(), self.w.detach(), self.b.detach(), lab, keep, seed,
                                 self.loss_scale, need_grad=need_grad, want_logits=want_logits,
                                 ws=self.xws, out_dw=self.dw.view(-1) if need_grad else None,
                                 out_db=self.db if need_grad else None)

    # -- the reference's three entry points -----------------------------------------------
    def forward(self, x, dropout: bool = True):
        """pred_out [N, M, T] (:317).  ``dropout=False`` runs the cell unwrapped."""
        with torch.no_grad():
            hs, mask = self._sequence(self._steps(x), dropout)
            return self._head(hs, self._no_labels, mask, False, True).logits

    def train_step(self, x, labels, stream=None, with_output: bool = False):
        """``train`` (:361-369): one optimizer step; returns the device loss [1]
        of this rank's batch (and pred_out with ``with_output``).  Its own step, not
        FlatTrainer's: the loss is the per-step softmax head's, not ``_loss``."""
        s = self._stream(stream)
        lab = self._labels(labels)
        self.grad.zero_()
        hs, mask = self._sequence(self._steps(x), True)
        r = self._head(hs, lab, mask, True, with_output)
        hs.backward(r.dhs)  # the cells' gradients accumulate into the bucket
        self._exchange_and_update(s)
        self.loss = r.loss
        return (r.loss, r.logits) if with_output else r.loss

    def test_step(self, x, labels, with_output: bool = False):
        """``test`` (:371-377): the loss without an update.  The DropoutWrapper is
        a constant of the reference's graph, so it drops here too (and the mask
        stream advances); no parameter, optimizer slot or step count changes."""
        lab = self._labels(labels)
        with torch.no_grad():
            hs, mask = self._sequence(self._steps(x), True)
            r = self._head(hs, lab, mask, False, with_output)
        return (r.loss, r.logits) if with_output else r.loss

    def predict(self, data, reference_dropout: bool = False):
        """pred_out over data [size, M, feat_in, T] in batches of N, the last one
        zero-padded and its padded rows dropped: [size, M, T].  Deterministic
        (no dropout) unless ``reference_dropout``."""
        return FlatTrainer.predict(self, data, None, dropout=reference_dropout)

    def evaluate(self, data, labels, reference_dropout: bool = False):
        raise NotImplementedError("gconvRNN.Model has no evaluate; use test_step for the loss")
