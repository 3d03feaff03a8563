"""``FlatTrainer``: what the seven device models (``ResGNN``, ``StackedResGNN``,
``GLSTMModel``, ``GLSTMGconvModel``, ``GLSTMPeriodModel``, ``GConvRNNModel``,
``GConvNetModel``) share around their forward and backward passes
(lib/graph_model.py:246-310; sgd / rmsprop of lib/gconvRNN.py:381-389).

  buffers   every parameter is a view into ONE flat fp32 buffer (``flat``),
            every gradient a view into ONE flat bucket (``grad``); the optimizer
            slots ``s1`` / ``s2`` have the same size.  ``carve`` hands the views
            out in creation order and records their names.
  graph     ``_set_graph`` / ``_graph_from_cell``: a Chebyshev ``plan``, or ``U`` and
            its prepared transform ``gft``; ``is_fourier`` / ``is_fourier_conv``
            validate the two filter vocabularies
  step      ``train_step``: forward, loss, backward, exchange, update
  loss      mean((labels - out)^2), dout and the loss moving average
            (lib/graph_model.py:265-273)                       cg_mse_loss_ema
  exchange  ONE all-reduce(sum) of the bucket when ``comm.world`` > 1
  update    ONE optimizer launch over ``flat``, grad_scale = 1/world
            (``_grad_scale``), at the staircase exponentially decayed learning
            rate; ``_after_exchange`` runs between exchange and update
  predict / evaluate  GraphModel's (lib/graph_model.py:64-122) through evaluate.py;
            ``DropoutEval`` adds ``reference_dropout`` for the models with wrappers
  fit       GraphModel.fit (lib/graph_model.py:124-197): the dataset lives on the
            device, ``fit_schedule`` restates the reference's index deque on the
            host, and each step is ONE cg_batch_gather plus ``train_step``

A model derives from it, allocates with ``FlatTrainer.__init__``, carves its
parameters, calls ``_carved()`` and implements two hooks:

  forward(x, stream=None, ...)   the output [N, M, Fout]; keeps what backward needs
  backward(dout, stream)         every gradient of the last forward into the bucket,
                                 zeroing first the part autograd ACCUMULATES into

and, where the defaults do not fit, ``_grad_scale`` and ``_after_exchange``
(``GConvRNNModel``, which also has a ``train_step`` of its own: its loss is not
the mean squared error).  ``comm`` is any object with ``allreduce_sum_(tensor,
stream)`` and ``world`` (``dist.RcclComm`` on RCCL, ``dist.TorchComm`` on a
process group).
"""
from __future__ import annotations

import ctypes
import math
import time

import numpy as np
import torch

from . import _lib
from . import evaluate as _ev
from . import filter as _filter
from . import ops
from .plan import plan_for

OPTIMIZERS = ("adam", "sgd", "rmsprop")
FILTERS = ("chebyshev5", "fourier")  # lib/graph_conv.py's names: ResGNN, StackedResGNN


def is_fourier(filter) -> bool:
    """Validates a ``FILTERS`` name; True for the Fourier filter."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
    return filter == "fourier"


def is_fourier_conv(filter) -> bool:
    """Validates one of lib/filter.py's names; True for the Fourier filter."""
    if filter not in ("cheby_conv", "fourier_conv"):
        raise ValueError("filter must be 'cheby_conv' or 'fourier_conv'")
    return filter == "fourier_conv"


def check_keep_prob(keep_prob, name: str = "keep_prob") -> float:
    if not 0.0 < float(keep_prob) <= 1.0:
        raise ValueError(f"{name} must be in (0, 1], got {keep_prob}")
    return float(keep_prob)


def check_seam(seam) -> str:
    if seam not in ("auto", "fused", "unfused"):
        raise ValueError("seam must be 'auto', 'fused' or 'unfused'")
    return seam


def fit_schedule(S: int, batch: int, num_steps: int, rng=None) -> np.ndarray:
    """The sample indices of ``num_steps`` batches of ``batch`` out of ``S``
    samples, int32 [num_steps, batch], drawn as GraphModel.fit draws them
    (lib/graph_model.py:139-147): a queue that is refilled with
    ``permutation(S)`` whenever fewer than ``batch`` indices are left, and a batch
    is its first ``batch`` entries.  Leftovers carry into the next epoch, so a
    batch that straddles a refill can hold one sample twice (the reference's
    behaviour, kept).

    ``rng``: a ``numpy.random.RandomState``; an int seed (``RandomState(seed)``);
    or None for the global ``numpy.random`` state, which is what the reference
    draws from -- after ``numpy.random.seed(k)`` the batches are the
    reference's, in its order."""
    S, batch, num_steps = int(S), int(batch), int(num_steps)
    if batch < 1 or num_steps < 0:
        raise ValueError(f"fit_schedule: batch = {batch}, num_steps = {num_steps}")
    if S < batch:
        raise ValueError(f"fit_schedule: {S} samples cannot fill a batch of {batch} (one refill per "
                         "batch: the reference's popleft raises IndexError here)")
    if rng is None:
        rng = np.random
    elif not isinstance(rng, np.random.RandomState):
        rng = np.random.RandomState(rng)
    out = np.empty((num_steps, batch), np.int32)
    left = np.empty((0,), np.int64)  # the deque, front first
    for step in range(num_steps):
        if left.size < batch:
            left = np.concatenate([left, rng.permutation(S)])
        out[step], left = left[:batch], left[batch:]
    return out


class FlatTrainer:
    def __init__(self, total: int, out_shape, optimizer: str, learning_rate, decay_rate, decay_steps,
                 device, comm):
        """total: the parameter count; out_shape: (N, M, Fout) of the model's output."""
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}")
        self.device = torch.device(device if device is not None else "cuda")
        self.optimizer, self.lr = optimizer, learning_rate
        self.decay_rate, self.decay_steps = decay_rate, decay_steps
        self.comm = comm
        f32 = dict(device=self.device, dtype=torch.float32)
        self.flat = torch.empty(total, **f32)
        self.grad = torch.zeros(total, **f32)
        # optimizer slots (TF 1.x: Adam m, v zeros; RMSProp ms ONES, mom zeros)
        self.s1 = (torch.ones if optimizer == "rmsprop" else torch.zeros)(total, **f32)
        self.s2 = torch.zeros(total, **f32)
        self.loss = torch.empty((1,), **f32)
        # {biased, average, local_step} of ExponentialMovingAverage(0.9) of the loss
        self.ema = torch.zeros((3,), **f32)
        self.dout = torch.empty(tuple(out_shape), **f32)
        self.mws, self.mws_n = ops._workspace("cg_mse_loss_workspace_bytes", math.prod(out_shape),
                                              device=self.device)
        self.step_count = 0
        # names / tensors / gradient views in carving order; ``params``: the
        # autograd-owned ones (torch.nn.Parameter, .grad = the bucket view)
        self.names, self.params = [], []
        self._tensors, self._grads, self._off = [], [], 0
        h = _lib.lib()  # the step's C entry points, looked up once
        self._mse = h.cg_mse_loss_ema
        self._update = {"adam": h.cg_adam_update, "sgd": h.cg_sgd_update,
                        "rmsprop": h.cg_rmsprop_update}[optimizer]

    # -- carving ------------------------------------------------------------------
    def carve(self, shape, name: str, init=None):
        """The next (parameter view, gradient view) of ``shape`` in the flat
        buffers.  With ``init`` (the LSTM cells, autograd-owned): ``init`` is
        copied in and the first is a ``torch.nn.Parameter`` aliasing ``flat``
        whose ``.grad`` is the bucket view."""
        n = math.prod(shape)
        w = self.flat[self._off:self._off + n].view(shape)
        g = self.grad[self._off:self._off + n].view(shape)
        if init is not None:
            with torch.no_grad():
                w.copy_(init)
            w = torch.nn.Parameter(w)
            w.grad = g
            self.params.append(w)
        self._off += n
        self.names.append(name)
        self._tensors.append(w)
        self._grads.append(g)
        return w, g

    def align(self, floats: int = 4):
        """Advance the carving offset to the next multiple of ``floats`` (a view
        a kernel reads as float4 must start 16-byte aligned).  The skipped
        entries belong to no parameter: they are zero with a zero gradient, and
        no optimizer moves such an entry."""
        pad = -self._off % floats
        self.flat[self._off:self._off + pad].zero_()
        self._off += pad

    def _carved(self):
        assert self._off == self.flat.numel(), (self._off, self.flat.numel())

    # -- the graph ------------------------------------------------------------------
    def _set_graph(self, L, fourier: bool, lmax):
        """``M`` and a Chebyshev ``plan``, or -- no plan -- ``U`` and ``gft``, U prepared once."""
        self.plan = self.U = self.gft = None
        if fourier:
            self.M = int(L.shape[0])
            self.U = _filter.fourier_basis(L, self.device)
            self.gft = ops.gft_prepare(self.U)
        else:
            dev_index = self.device.index if self.device.index is not None else 0
            self.plan = plan_for(L, lmax=lmax, device=dev_index)
            self.M = self.plan.M

    def _graph_from_cell(self, cell, gft: bool = False):
        """The same from a model's first LSTM cell.  ``gft``: a residual head will
        read the prepared transform -- the fused cell's own, else prepared here."""
        fourier = cell.filter_type == "fourier_conv"
        self.M = cell._nNode
        self.plan = None if fourier else cell.plan
        self.U = cell.U if fourier else None
        self.gft = None
        if fourier and gft:
            self.gft = cell.gft_basis if cell.gft_basis is not None else ops.gft_prepare(self.U)

    def _alloc_ws(self, nets):
        # one workspace serves every forward and backward call of the nets (stream
        # order: a call's workspace is dead once the call has executed)
        self.ws_n = max(n.ws_bytes() for n in nets)
        self.ws = torch.empty(max(self.ws_n, 1), device=self.device, dtype=torch.uint8)

    def parameters(self):
        return dict(zip(self.names, self._tensors))

    def gradients(self):
        return dict(zip(self.names, (g if t.grad is None else t.grad
                                     for t, g in zip(self._tensors, self._grads))))

    # -- the step's shared pieces -----------------------------------------------------
    @property
    def world(self):
        return self.comm.world if self.comm is not None else 1

    @property
    def loss_average(self):
        """The loss moving average (lib/graph_model.py:271-273), a device scalar."""
        return self.ema[1:2]

    def learning_rate(self, step):
        """tf.train.exponential_decay(lr, global_step, decay_steps, decay_rate, staircase=True)."""
        if self.decay_rate == 1 or not self.decay_steps:
            return self.lr
        return self.lr * self.decay_rate ** math.floor(step / self.decay_steps)

    def _stream(self, stream):
        return stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream

    def _loss(self, out, labels, s):
        """loss, dout and the moving average from the logits; ``self.dout`` feeds the backward."""
        n = out.numel()
        labels = labels.contiguous()
        if labels.numel() != n:
            raise ValueError("labels must match the logits' shape")
        _lib.check("cg_mse_loss_ema", self._mse(out.data_ptr(), labels.data_ptr(), n,
                                                self.loss.data_ptr(), self.dout.data_ptr(),
                                                self.ema.data_ptr(), ctypes.c_float(0.9),
                                                self.mws.data_ptr(), self.mws_n, s))

    # two hooks of the step's tail; the defaults are the mean-loss models'
    def _grad_scale(self, world: int) -> float:
        """What the optimizer multiplies the exchanged (summed) bucket by: 1/world
        for a loss that is a mean over the batch."""
        return 1.0 / world

    def _after_exchange(self, s):
        """Called between the all-reduce and the optimizer launch (gradient clipping)."""

    def _exchange_and_update(self, s):
        """The tail of a step: every autograd-owned .grad still inside the bucket,
        ONE all-reduce when world > 1, ONE optimizer launch with grad_scale = 1/world."""
        lo = self.grad.data_ptr()
        for p in self.params:  # autograd accumulated into the flat bucket in place
            if p.grad is None or not lo <= p.grad.data_ptr() < lo + 4 * self.grad.numel():
                raise RuntimeError("a parameter's .grad left the flat gradient bucket")
        world = self.world
        if world > 1:
            self.comm.allreduce_sum_(self.grad, s)
        self._after_exchange(s)
        self.step_count += 1
        self._optimizer_launch(self.learning_rate(self.step_count - 1), self._grad_scale(world), s)

    def _optimizer_launch(self, lr: float, scale: float, s):
        """The ONE update launch over ``flat`` (a hook: ``CGCNNModel`` runs Momentum
        with its L2 term here)."""
        f = ctypes.c_float
        flat, grad, n = self.flat.data_ptr(), self.grad.data_ptr(), self.flat.numel()
        lr, scale = f(lr), f(scale)
        if self.optimizer == "adam":
            st = self._update(flat, grad, self.s1.data_ptr(), self.s2.data_ptr(), n, lr, f(0.9),
                              f(0.999), f(1e-8), self.step_count, scale, s)
        elif self.optimizer == "sgd":
            st = self._update(flat, grad, n, lr, scale, s)
        else:
            st = self._update(flat, grad, self.s1.data_ptr(), self.s2.data_ptr(), n, lr, f(0.9),
                              f(0.0), f(1e-10), scale, s)
        _lib.check(f"cg_{self.optimizer}_update", st)

    def train_step(self, x, labels, stream=None):
        """One optimizer step (lib/graph_model.py:277-310) on this rank's batch;
        returns the device loss [1]."""
        s = self._stream(stream)
        out = self.forward(x, stream=s)
        self._loss(out, labels, s)
        self.backward(self.dout, s)
        self._exchange_and_update(s)
        return self.loss

    # -- inference ------------------------------------------------------------------
    def predict(self, data, labels=None, **forward_kw):
        """GraphModel.predict (lib/graph_model.py:64-94): predictions [size, M,
        Fout] over batches of N, the last one zero-padded; with labels also the
        reference's ``loss * batch_size / size`` (evaluate.predict has the quirk,
        padded rows included).  ``forward_kw`` goes to the model's ``forward``.
        No parameter, optimizer slot, loss average or step count changes."""
        fwd = (lambda b: self.forward(b, **forward_kw)) if forward_kw else self.forward
        return _ev.predict(fwd, self.N, self.device, data, labels)

    def evaluate(self, data, labels, **forward_kw):
        """GraphModel.evaluate (:96-122): (string, mse, 0, loss, predictions)."""
        return _ev.evaluate(lambda d, l: FlatTrainer.predict(self, d, l, **forward_kw), data, labels)

    # -- training loop --------------------------------------------------------------
    # two hooks of ``fit``; the defaults are the regression models' (labels [S, M, Fout])
    def _fit_set(self, name, d, l):
        """One of fit's two (data, labels) pairs on the device, validated.  The
        labels are rows of 4-byte words that cg_batch_gather copies unchanged and
        that ``evaluate`` accepts."""
        _, M, Fout = (int(v) for v in self.dout.shape)
        f32 = dict(device=self.device, dtype=torch.float32)
        d = torch.as_tensor(d).to(**f32).contiguous()
        l = torch.as_tensor(l).to(**f32).contiguous()
        if d.dim() != 3 or int(d.shape[1]) != M:
            raise ValueError(f"fit: {name}_data must be [samples, M = {M}, channels], got {tuple(d.shape)}")
        if int(l.shape[0]) != int(d.shape[0]):
            raise ValueError(f"fit: {name} data and labels differ in their number of samples")
        if l.numel() != int(d.shape[0]) * M * Fout:
            raise ValueError(f"fit: {name}_labels must hold [samples, {M}, {Fout}] values")
        return d, l

    def _fit_label_batch(self):
        """The buffer a step's labels are gathered into, as ``train_step`` takes them."""
        return torch.empty(tuple(self.dout.shape), device=self.device, dtype=torch.float32)

    def fit(self, train_data, train_labels, val_data, val_labels, num_epochs=20, eval_frequency=200,
            rng=None, verbose=True, stream=None, rank=None):
        """GraphModel.fit (lib/graph_model.py:124-197): ``int(num_epochs * S / B)``
        optimizer steps over shuffled batches (``fit_schedule``), ``evaluate`` on the
        validation set every ``eval_frequency`` steps and after the last one.
        Returns ``(accuracies, losses, t_step)``: evaluate's mse and loss at each
        evaluation, and the wall time per step, evaluations included (:196).

        The four arrays are moved to the device as fp32 once (data [S, M, C],
        labels with S * M * Fout elements); a dataset that does not fit in device
        memory next to the model is out of scope.  The whole index schedule is
        uploaded once as well, so a step is ONE cg_batch_gather into two buffers
        allocated here and then ``train_step`` on them, in stream order: no host
        synchronisation between evaluations and no torch indexing.  ``stream`` is
        ``train_step``'s.

        Data parallel (``comm.world`` > 1): B = N * world is the global batch,
        every rank builds the same schedule and rank r trains on its columns
        [r N, (r + 1) N) -- ``dist.shard``'s split.  ``rank`` defaults to the
        launcher's (``dist.env_rank_world``); ``rng`` must be a seed or a
        RandomState that is the same on every rank, so None is refused.

        ``verbose`` prints the reference's progress lines (:169-175, :192); the
        learning rate shown is the one the last step applied.  Checkpoints are
        not written."""
        N = int(self.dout.shape[0])
        world = self.world
        if world > 1 and rng is None:
            raise ValueError("fit: rng=None draws from this process's global numpy state; with "
                             f"world = {world} every rank must draw the same permutations: pass a seed")
        if rank is None:
            rank = 0
            if self.comm is not None:
                from . import dist
                rank = dist.env_rank_world()[0]
        if not 0 <= int(rank) < world:
            raise ValueError(f"fit: rank {rank} outside [0, {world})")
        f32 = dict(device=self.device, dtype=torch.float32)
        (data, labels), (val_data, val_labels) = (
            self._fit_set(name, d, l)
            for name, d, l in (("train", train_data, train_labels), ("val", val_data, val_labels)))
        S, B = int(data.shape[0]), N * world
        num_steps = int(num_epochs * S / B)
        sched = fit_schedule(S, B, num_steps, rng)  # refuses S < B
        if num_steps < 1:
            raise ValueError(f"fit: num_epochs = {num_epochs} over {S} samples is less than one batch of {B}")
        row, lrow = data.numel() // S, labels.numel() // S
        labels = labels.view(S, lrow)
        idx = torch.from_numpy(sched).to(self.device)
        x_b = torch.empty((N,) + tuple(data.shape[1:]), **f32)
        y_b = self._fit_label_batch()
        s = self._stream(stream)
        gather = _lib.lib().cg_batch_gather
        dp, lp, xp, yp = data.data_ptr(), labels.data_ptr(), x_b.data_ptr(), y_b.data_ptr()
        ip = idx.data_ptr() + 4 * int(rank) * N  # this rank's columns of step 0
        accuracies, losses = [], []
        t_process, t_wall = time.process_time(), time.time()
        for step in range(1, num_steps + 1):
            _lib.check("cg_batch_gather", gather(dp, lp, ip + 4 * B * (step - 1), N, S, row, lrow, xp, yp, s))
            self.train_step(x_b, y_b, stream)
            if step % eval_frequency == 0 or step == num_steps:
                string, mse, _, loss, _ = self.evaluate(val_data, val_labels)
                accuracies.append(mse)
                losses.append(loss)
                if verbose:
                    print("step {} / {} (epoch {:.2f} / {}):".format(step, num_steps, step * B / S, num_epochs))
                    print("  learning_rate = {:.2e}, loss_average = {:.2e}".format(
                        self.learning_rate(self.step_count - 1), float(self.loss_average)))
                    print("  validation {}".format(string))
                    print("  time: {:.0f}s (wall {:.0f}s)".format(time.process_time() - t_process,
                                                                 time.time() - t_wall))
        torch.cuda.synchronize(self.device)
        if verbose:
            print("validation accuracy: peak = {:.2f}, mean = {:.2f}".format(max(accuracies),
                                                                            np.mean(accuracies[-10:])))
        return accuracies, losses, (time.time() - t_wall) / num_steps


class DropoutEval:
    """``predict`` / ``evaluate`` of a model whose ``forward`` takes ``dropout``
    (DropoutWrappers inside); goes in front of FlatTrainer in the bases."""

    def predict(self, data, labels=None, reference_dropout: bool = False):
        """``FlatTrainer.predict``.  Dropout at evaluation: the reference's DropoutWrapper(0.8) is a constant
        of its graph, so the reference ALSO drops when it evaluates.  The
        default here is no dropout (deterministic predictions);
        ``reference_dropout=True`` applies the wrappers' masks as a training
        forward does (and advances their mask streams)."""
        return super().predict(data, labels, dropout=reference_dropout)

    def evaluate(self, data, labels, reference_dropout: bool = False):
        """``FlatTrainer.evaluate``; ``reference_dropout`` as in ``predict``."""
        return super().evaluate(data, labels, dropout=reference_dropout)
