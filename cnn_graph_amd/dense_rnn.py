"""``lib/gconvRNN.py::Model`` with ``model_type='lstm'``: the dense LSTM baseline
the reference's sequence experiments compare the graph LSTM against.  Every
time step is a flat ``[N, num_node]`` vector and every step predicts a class in
``[0, num_node)``.

  x [N, num_node, T]  --unstack axis 2 (:259-262)-->  T x [N, num_node]
  head      'weight' [H, C] and 'bias' [C], C = num_node, random_normal(0, 1),
            tf.Variables made BEFORE static_rnn first calls the cell (:282-285):
            they come first in the variable list
  cell      ONE BasicLSTMCell(num_hidden, forget_bias=1.0) (:281) in a
            DropoutWrapper(output_keep_prob=0.8) under static_rnn from the zero
            state (:299-300, ``dtype`` only)
  outputs   per step reshape(h_t, [-1, H]) @ weight + bias (:308-309);
            pred_out = concat(predictions, 1): [N, T*C], column t*C + c (:315)
            -- NOT the glstm branch's [N, M, T]
  labels    [N, T] int64, one class per step (:271-274)
  loss      sparse_softmax_cross_entropy_with_logits per step (:328-330),
            reduce_sum(axis=1) over the BATCH and reduce_mean over time
            (:331-332): loss = (1/T) sum_t sum_n ce
  optim     sgd / adam / rmsprop at a constant learning rate; max_grad_norm clips
            per variable with tf.clip_by_norm + tf.check_numerics (:381-409)

TensorFlow is not vendored with the reference, so the cell is restated from
TF 1.x ``rnn_cell_impl.py`` (BasicLSTMCell), as SURVEY section 8c allows:
  * ONE ``kernel`` [C + H, 4H] (glorot-uniform over that shape, the
    variable-scope default) and ``bias`` [4H] (zeros);
    gates = concat([x, h], 1) @ kernel + bias, split into i | j | f | o
  * c' = c * sigmoid(f + forget_bias) + sigmoid(i) * tanh(j);
    h' = tanh(c') * sigmoid(o)
Here the kernel is carved as one variable and Wx (its first C rows) and Wh (the
remaining H rows) are views: tf.clip_by_norm is per variable (:397-403), so the
clip norm is over the whole kernel.

On device: gx of all steps is one cg_gemm_f32; the recurrence is
``ops.dense_lstm_seq`` (``path``: "seq" = cg_dlstm_seq_forward / _backward, one
launch a direction; "steps" = the per-step composition of cg_gemm_f32 and
cg_lstm_cell_*; "auto" = ``AUTO_PATH``, DESIGN.md "The dense LSTM baseline");
the DropoutWrapper masks the OUTPUTS only (cg_dropout_forward / _backward on hs
[T, N, H]; the state path reads the unmasked h); the head is cg_gemm_f32 +
cg_bias_act_forward(CG_ACT_NONE); the loss is cg_class_xent_sum with
loss_scale = 1/T.

Data parallel: the loss is a SUM over the batch, so the ranks' gradients add:
one all-reduce(sum) of the bucket and grad_scale = 1.  The clip runs on the
exchanged gradient, before the update.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops
from .trainer import FlatTrainer, check_keep_prob

# what path="auto" resolves to ("The dense LSTM baseline": the rule and
# the measurement)
AUTO_PATH = "seq"


class LSTMRNNModel(FlatTrainer):
    """gconvRNN.Model(model_type='lstm') on device.  Parameters, in the flat
    buffer's (the reference's creation) order: the head's ``weight`` [H, C] and
    ``bias`` [C], then the cell's ``kernel`` [C + H, 4H] and ``bias`` [4H]."""

    def __init__(self, N: int, T: int, num_node: int, num_hidden: int = 32, keep_prob: float = 0.8,
                 optimizer: str = "sgd", learning_rate: float = 1e-3,
                 max_grad_norm: float | None = None, forget_bias: float = 1.0, device=None,
                 seed: int = 2017, comm=None, path: str = "auto"):
        self.N, self.T, self.C, self.H = int(N), int(T), int(num_node), int(num_hidden)
        N, T, C, H = self.N, self.T, self.C, self.H
        if min(N, T, C, H) < 1:
            raise ValueError("N, T, num_node and num_hidden must be positive")
        self.keep_prob = check_keep_prob(keep_prob)
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm must be positive (or None)")
        if path not in ("auto",) + ops.DENSE_LSTM_PATHS:
            raise ValueError(f"path must be 'auto' or one of {ops.DENSE_LSTM_PATHS}")
        self.path = AUTO_PATH if path == "auto" else path
        if self.path == "seq" and not ops.dense_lstm_supported(H):
            # a missing kernel is an error, not a quiet change of path
            raise ValueError(f"path 'seq' needs num_hidden % 16 == 0 and 16 <= num_hidden <= 128, got {H}")
        self.forget_bias = float(forget_bias)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # constant learning rate: decay_rate = 1 (the reference's optimizers take a float)
        super().__init__(H * C + C + (C + H) * 4 * H + 4 * H, (N, T * C), optimizer, learning_rate, 1,
                         None, device, comm)
        f32 = dict(device=self.device, dtype=torch.float32)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        self.w, self.dw = self.carve((H, C), "gconv_model/weight")
        self.b, self.db = self.carve((C,), "gconv_model/bias")
        self.w.normal_(0.0, 1.0, generator=gen)
        self.b.normal_(0.0, 1.0, generator=gen)
        lim = math.sqrt(6.0 / ((C + H) + 4 * H))
        k0 = torch.empty((C + H, 4 * H), **f32).uniform_(-lim, lim, generator=gen)
        self.kernel, self.dkernel = self.carve((C + H, 4 * H), "gconv_model/rnn/basic_lstm_cell/kernel",
                                               init=k0)
        self.cell_bias, self.dcell_bias = self.carve((4 * H,), "gconv_model/rnn/basic_lstm_cell/bias",
                                                     init=torch.zeros((4 * H,), **f32))
        self._carved()
        self.loss_scale = 1.0 / T
        self.xws, _ = ops._workspace("cg_class_xent_workspace_bytes", T * N, C, 0, device=self.device)
        self._no_labels = torch.zeros((T * N,), device=self.device, dtype=torch.int32)
        self._drop_seed = int(seed) & ((1 << 64) - 1)
        self._drop_calls = 0
        self.last_drop_seed = None  # the seed of the last mask drawn (None: none yet)

    # -- FlatTrainer's hooks -------------------------------------------------------
    def _grad_scale(self, world):
        return 1.0  # the loss sums over the batch: the ranks' gradients add

    def _after_exchange(self, s):
        if self.max_grad_norm is not None:  # per variable, then check_numerics (:392-402)
            ops.clip_by_norm_(self._grads, self.max_grad_norm, check_numerics=True)

    # -- pieces ----------------------------------------------------------------------
    @property
    def Wx(self):
        return self.kernel[:self.C]

    @property
    def Wh(self):
        return self.kernel[self.C:]

    def _steps(self, x):
        """rnn_input [N, C, T] -> the step-major rows [T*N, C] (tf.unstack on axis 2)."""
        if tuple(x.shape) != (self.N, self.C, self.T) or not x.is_cuda:
            raise ValueError(f"x must be a cuda tensor of [N, num_node, T] = {(self.N, self.C, self.T)}")
        return x.to(torch.float32).permute(2, 0, 1).contiguous().view(self.T * self.N, self.C)

    def _labels(self, labels):
        """[N, T] classes -> the loss's step-major int32 device tensor [T*N]."""
        if isinstance(labels, torch.Tensor) and labels.is_cuda:
            lab = labels.t()
        else:
            lab = np.asarray(labels.numpy() if isinstance(labels, torch.Tensor) else labels).T
        if tuple(lab.shape) != (self.T, self.N):
            raise ValueError(f"labels must be [N, T] = {(self.N, self.T)}")
        return ops.class_labels(lab.reshape(-1), self.C, self.device)

    def _next_seed(self) -> int:
        self._drop_calls += 1
        self.last_drop_seed = (self._drop_seed + 0xD1B54A32D192ED03 * self._drop_calls) & ((1 << 64) - 1)
        return self.last_drop_seed

    def _sequence(self, xs, dropout: bool):
        """The wrapped cell's outputs hd [T*N, H] (the mask on the outputs only)."""
        hs = ops.dense_lstm_seq(xs, self.kernel, self.cell_bias, self.T, self.N, self.forget_bias,
                                self.path)
        if dropout and self.keep_prob < 1.0:
            hs = ops.dropout(hs, self.keep_prob, self._next_seed())
        return hs.view(self.T * self.N, self.H)

    def _logits(self, hd):
        return ops.bias_act(ops.gemm(hd, self.w), self.b, "none")

    def _pred_out(self, logits):
        """[T*N, C] step-major -> concat(predictions, 1): [N, T*C] (:315)."""
        return logits.view(self.T, self.N, self.C).permute(1, 0, 2).reshape(self.N, self.T * self.C)

    # -- the reference's entry points ------------------------------------------------
    def forward(self, x, dropout: bool = True):
        """pred_out [N, T*C] (:315).  ``dropout=False`` runs the cell unwrapped."""
        with torch.no_grad():
            return self._pred_out(self._logits(self._sequence(self._steps(x), dropout)))

    def train_step(self, x, labels, stream=None, with_output: bool = False):
        """``train`` (:361-369): one optimizer step; returns the device loss [1]
        of this rank's batch (and pred_out with ``with_output``)."""
        s = self._stream(stream)
        lab = self._labels(labels)
        self.grad.zero_()
        hd = self._sequence(self._steps(x), True)
        with torch.no_grad():
            h2 = hd.detach()
            logits = self._logits(h2)
            r = ops.class_xent_sum(logits, lab, self.loss_scale, ws=self.xws,
                                   out_dlogits=self.dout.view(self.T * self.N, self.C))
            ops.gemm(h2, r.dlogits, trans_a=True, out=self.dw)
            ops.bias_grad(r.dlogits, out=self.db)
            dhd = ops.gemm(r.dlogits, self.w, trans_b=True)
        hd.backward(dhd)  # the cell's gradients accumulate into the bucket
        self._exchange_and_update(s)
        self.loss = r.loss
        return (r.loss, self._pred_out(logits)) if with_output else r.loss

    def test_step(self, x, labels, with_output: bool = False):
        """``test`` (:371-377): the loss without an update.  The DropoutWrapper is
        a constant of the reference's graph, so it drops here too (and the mask
        stream advances); no parameter, optimizer slot or step count changes."""
        lab = self._labels(labels)
        with torch.no_grad():
            logits = self._logits(self._sequence(self._steps(x), True))
            r = ops.class_xent_sum(logits, lab, self.loss_scale, need_grad=False, ws=self.xws)
        return (r.loss, self._pred_out(logits)) if with_output else r.loss

    def predict(self, data, reference_dropout: bool = False):
        """pred_out over data [size, num_node, T] in batches of N, the last one
        zero-padded and its padded rows dropped: [size, T*C].  Deterministic (no
        dropout) unless ``reference_dropout``."""
        return FlatTrainer.predict(self, data, None, dropout=reference_dropout)

    def evaluate(self, data, labels, reference_dropout: bool = False):
        raise NotImplementedError("gconvRNN.Model has no evaluate; use test_step for the loss")
