"""``CGCNNModel``: the pooled cgcnn classifier of the reference's notebooks
(``models.cgcnn(L, F, K, p, M, ...)``, lib/models.py:24-127, usage.ipynb) trained
on device: ``GraphConv.cgcnn_inference``'s network, the class loss the fork left
in comments (lib/graph_model.py:249-258), its L2 term (lib/graph_conv.py:174,
:198, :223-224) and ``tf.train.MomentumOptimizer`` (lib/graph_model.py:287-291),
as ONE explicit schedule of C-ABI launches on ``FlatTrainer``'s flat buffers.  No
torch compute op runs in the step: torch only owns the buffers.

  conv{i}   y = relu(cheb(x; W_i)) on level i's own plan      cg_cheb_forward_layout
            (b1relu: the ReLU in the y store; b2relu: y = cheb(x), then
            z = relu(y + b_i), b_i [1, M_i, F_i]               cg_bias_act_forward)
            x' = pool(y, p_i)             cg_maxpool_forward / cg_avgpool_forward
            (p_i == 1: no launch)
  flatten   a view [N, M_last F_last]
  fc{i}     y = relu(x W + b)                     cg_gemm_f32, cg_bias_act_forward
            training: x' = dropout(y, keep)       cg_dropout_forward (keep == 1: no launch)
  logits    x W + b                               cg_gemm_f32, cg_bias_act_forward
  loss      mean_n ce(logits_n, label_n) + regularization * sum 1/2 ||v||^2 over
            the fc / logits weights and biases, dlogits, the loss moving
            average                                              cg_class_xent_ema
  backward  logits, fc{i}: db and dz = dy * [y > 0]             cg_bias_act_backward
            dW = x^T dz, dx = dz W^T (no dx into data)          cg_gemm_f32 (twice)
            the dropout mask regenerated from its seed          cg_dropout_backward
            conv{i}: pool backward writes the gradient      cg_maxpool_backward /
            that the filter's backward masks with the saved y   cg_avgpool_backward
            (b2relu: cg_bias_act_backward masks it and sums db),
            then dW and dx (conv1: x is data, no dx)          cg_cheb_backward_layout
  exchange  ONE all-reduce(sum) of the flat gradient bucket when world > 1
  update    accum = momentum accum + g, w -= lr accum, with g = grad / world +
            regularization * w on the regularised variables      cg_momentum_update
            (momentum == 0 and regularization == 0:              cg_sgd_update)

C-ABI calls per step, with G conv levels of which P pool (p_i > 1), H hidden fc
layers, and d = 1 with dropout < 1 else 0, b = 1 with b2relu else 0:
  forward G (1 + b) + P + 2 (H + 1) + d H,  loss 1,
  backward 3 (H + 1) - [G == 0] + d H + P + G (1 + b),  update 1.
usage.ipynb's network (G = P = 2, H = 1, b1relu, dropout 0.5): 9 + 1 + 11 + 1 = 22.

Variables, in creation order (= initialisation order, one generator):
conv{i}/weights [Fin K, F], conv{i}/bias [1, M_i, F_i] (b2relu only), fc{i}/weights,
fc{i}/bias, logits/weights, logits/bias; weights truncated_normal(0, 0.1), biases
0.1.  The regularised variables are the fc / logits ones: ONE contiguous range
[reg_begin, total) of the flat buffer, which the loss and the update take as a
pair of integers.

Labels are class ids.  ``fit`` keeps them on the device as int32 and
cg_batch_gather carries them as they are: it copies 4-byte words and never
does arithmetic on them, so an int32 row passes through the fp32 entry
bit for bit (a row of an index outside the dataset is 0 = class 0).

Data parallel: the loss is a mean over the rank's batch, grad_scale = 1 / world;
the L2 term enters once, in the update after the exchange, and once in every
rank's reported loss.  Dropout draws one mask stream per fc layer from (seed,
rank, layer), advanced every training forward (``gconv_lstm.dropout_seed``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import ops
from .graph_conv import GraphConv, truncated_normal_
from .model import _ChebFilter
from .plan import plan_for
from .trainer import FlatTrainer, check_keep_prob

FILTERS = ("chebyshev5", "chebyshev2")  # one HIP path (graph_conv.GraphConv.chebyshev2)
BRELUS = ("b1relu", "b2relu")
POOLS = ("mpool1", "apool1")
_STREAM_STEP = 0xD1B54A32D192ED03  # a mask stream's per-call increment (DropoutWrapper's)


def weighted_f1(labels, predictions) -> float:
    """sklearn.metrics.f1_score(labels, predictions, average='weighted') from the
    confusion matrix: the classes' F1 = 2 tp / (2 tp + fp + fn) (0 where that is
    0 / 0) averaged with the classes' supports as weights."""
    y = np.asarray(labels).astype(np.int64).ravel()
    q = np.asarray(predictions).astype(np.int64).ravel()
    if y.shape != q.shape or y.size == 0:
        raise ValueError("labels and predictions must be equally long and not empty")
    C = int(max(y.max(), q.max())) + 1
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (y, q), 1)
    tp = np.diag(conf).astype(np.float64)
    support, predicted = conf.sum(axis=1), conf.sum(axis=0)
    den = (support + predicted).astype(np.float64)  # 2 tp + fn + fp
    f1 = np.divide(2 * tp, den, out=np.zeros(C), where=den > 0)
    return float((f1 * support).sum() / support.sum())


class _Level:
    """One conv level: its filter on its own plan, the b2relu bias, the pool, and
    the buffers its forward saves and its backward writes."""


class CGCNNModel(FlatTrainer):
    def __init__(self, L, N: int, F, K, p, M, Fin: int = 1, filter: str = "chebyshev5",
                 brelu: str = "b1relu", pool: str = "mpool1", regularization: float = 0,
                 dropout: float = 1, learning_rate: float = 0.1, decay_rate: float = 0.95,
                 decay_steps: int | None = None, momentum: float = 0.9, device=None,
                 seed: int = 2017, comm=None):
        """L: the graph Laplacians of the coarsening pyramid, finest first; N: the
        batch size; F, K, p: the conv levels' widths, polynomial orders and pooling
        sizes (powers of 2); M: the fc layers' widths, M[-1] the number of classes;
        Fin: the input's features per vertex.  ``filter`` 'chebyshev5' or
        'chebyshev2' (the Fourier classifier is not built), ``brelu`` 'b1relu' or
        'b2relu', ``pool`` 'mpool1' or 'apool1'.  ``dropout`` is the fc layers'
        keep-probability in (0, 1]."""
        if filter not in FILTERS:
            raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
        if brelu not in BRELUS:
            raise ValueError(f"brelu must be one of {BRELUS}, got {brelu!r}")
        if pool not in POOLS:
            raise ValueError(f"pool must be one of {POOLS}, got {pool!r}")
        F, K, p, M = ([int(v) for v in t] for t in (F, K, p, M))
        if not (len(F) == len(K) == len(p)):
            raise ValueError("need len(F) == len(K) == len(p) (lib/models.py:72)")
        if len(M) < 1 or min(F + K + M + [int(N), int(Fin)]) < 1:
            raise ValueError("N, Fin and every entry of F, K, M must be >= 1, and M not empty")
        if len(L) < 1:
            raise ValueError("need at least one graph level")
        Ls = GraphConv.select_laplacians(L, p)  # refuses too few levels, p not a power of 2
        self.keep = check_keep_prob(dropout, "dropout")
        if not float(momentum) >= 0.0 or not float(regularization) >= 0.0:
            raise ValueError("momentum and regularization must be >= 0")
        Mv = [int(l.shape[0]) for l in Ls]
        M0 = Mv[0] if Mv else int(L[0].shape[0])
        for i, (m, pp) in enumerate(zip(Mv, p)):
            if m % pp or (i + 1 < len(Mv) and Mv[i + 1] != m // pp):
                raise ValueError(f"level {i}: {m} vertices pooled by {pp} do not give the next "
                                 "level's graph")
        G, b2 = len(F), brelu == "b2relu"
        fins = [int(Fin)] + F[:-1]
        flat_w = Mv[-1] // p[-1] * F[-1] if G else M0 * int(Fin)
        fc_in = [flat_w] + M[:-1]
        conv_total = sum(fi * k * fo + (m * fo if b2 else 0) for fi, k, fo, m in zip(fins, K, F, Mv))
        total = conv_total + sum(a * b + b for a, b in zip(fc_in, M))
        super().__init__(total, (int(N), M[-1]), "sgd", learning_rate, decay_rate, decay_steps,
                         device, comm)
        self.N, self.Fin, self.M0, self.C = int(N), int(Fin), M0, M[-1]
        self.F, self.K, self.p, self.Mfc = F, K, p, M
        self.filter, self.brelu, self.pool = filter, brelu, pool
        self.regularization, self.momentum = float(regularization), float(momentum)
        self.reg_begin, self.reg_n = conv_total, total - conv_total
        self.accum = self.s1  # the Momentum slot, zeros
        self.plan = self.M = None  # every level has its own
        N = self.N
        f32 = dict(device=self.device, dtype=torch.float32)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        dev_index = self.device.index if self.device.index is not None else 0
        h = _lib.lib()

        def weights(shape, name):
            w, g = self.carve(shape, name)
            truncated_normal_(w, 0.1, gen)
            return w, g

        def bias(shape, name):
            w, g = self.carve(shape, name)
            with torch.no_grad():
                w.fill_(0.1)
            return w, g

        ws_n = [1]
        self.levels = []
        for i in range(G):
            lv = _Level()
            fi, fo, k, m, pp = fins[i], F[i], K[i], Mv[i], p[i]
            lv.M, lv.F, lv.p = m, fo, pp
            lv.W, lv.dW = weights((fi * k, fo), f"conv{i + 1}/weights")
            lv.b = lv.db = lv.z = None
            if b2:
                lv.b, lv.db = bias((1, m, fo), f"conv{i + 1}/bias")
                lv.z = torch.empty((N, m, fo), **f32)
                ws_n.append(ops._ws_bytes("cg_bias_act_workspace_bytes", N * m * fo, m * fo)[0])
            lv.y = torch.empty((N, m, fo), **f32)  # the filter's output, saved
            lv.filt = _ChebFilter(self, fi, fo, k, "none" if b2 else "relu", lv.W, lv.dW, lv.y,
                                  plan=plan_for(Ls[i], lmax=2, device=dev_index), M=m)
            ws_n.append(lv.filt.ws_bytes())
            lv.pooled = torch.empty((N, m // pp, fo), **f32) if pp > 1 else None
            lv.argmax = (torch.empty((N, m // pp, fo), device=self.device, dtype=torch.int32)
                         if pp > 1 and pool == "mpool1" else None)
            lv.dpool = torch.empty((N, m, fo), **f32) if pp > 1 else None  # d(act output)
            lv.dz = torch.empty((N, m, fo), **f32)                          # through the ReLU
            lv.dx = torch.empty((N, m, fi), **f32) if i > 0 else None       # conv1 reads data
            self.levels.append(lv)
        self._Ls = Ls  # the plan cache is keyed by these objects
        self.fcs = []
        for j, (a, b) in enumerate(zip(fc_in, M)):
            fc = _Level()
            last = j == len(M) - 1
            scope = "logits" if last else f"fc{j + 1}"
            fc.Min, fc.Mout, fc.relu = a, b, not last
            fc.W, fc.dW = weights((a, b), f"{scope}/weights")
            fc.b, fc.db = bias((b,), f"{scope}/bias")
            fc.y = torch.empty((N, b), **f32)
            fc.drop = torch.empty((N, b), **f32) if self.keep < 1.0 and not last else None
            fc.dz = torch.empty((N, b), **f32) if not last else None  # logits: dz is dlogits
            fc.ddrop = torch.empty((N, b), **f32) if fc.drop is not None else None
            fc.dx = torch.empty((N, a), **f32) if (j > 0 or G > 0) else None
            fc.x = None
            ws_n.append(ops._ws_bytes("cg_bias_act_workspace_bytes", N * b, b)[0])
            self.fcs.append(fc)
        self._carved()
        self.ws_n = max(ws_n)
        self.ws = torch.empty(self.ws_n, device=self.device, dtype=torch.uint8)
        self.xws, self.xws_n = ops._workspace("cg_class_xent_workspace_bytes", N, self.C, self.reg_n,
                                              device=self.device)
        self.status = torch.zeros((1,), device=self.device, dtype=torch.int32)
        # one mask stream per hidden fc layer, from (seed, rank, layer)
        from .gconv_lstm import dropout_seed
        rank = int(getattr(comm, "rank", 0)) if comm is not None else 0
        self._drop_base = [dropout_seed(seed, rank, j) for j in range(len(M) - 1)]
        self._drop_calls = 0
        self.drop_seeds = [0] * (len(M) - 1)  # the seeds of the last training forward
        self._dropped = False
        self._xent, self._mom = h.cg_class_xent_ema, h.cg_momentum_update
        self._gemm, self._ba_f, self._ba_b = h.cg_gemm_f32, h.cg_bias_act_forward, h.cg_bias_act_backward
        self._drop_f, self._drop_b = h.cg_dropout_forward, h.cg_dropout_backward
        self._pool_f = h.cg_maxpool_forward if pool == "mpool1" else h.cg_avgpool_forward
        self._pool_b = h.cg_maxpool_backward if pool == "mpool1" else h.cg_avgpool_backward

    # -- forward --------------------------------------------------------------------
    def forward(self, x, stream=None, dropout: bool = True):
        """The logits [N, C] of x [N, M0, Fin] (or [N, M0] with Fin == 1), already in
        the coarsening order (``ops.perm_data``).  ``dropout``: a training forward
        -- the fc layers' masks are applied (keep < 1) and their streams advance."""
        s = self._stream(stream)
        N = self.N
        if x.dim() == 2 and self.Fin == 1:
            x = x.unsqueeze(2)
        if tuple(x.shape) != (N, self.M0, self.Fin) or not x.is_cuda or x.dtype != torch.float32:
            raise ValueError(f"x must be a cuda fp32 tensor of shape {(N, self.M0, self.Fin)}")
        x = x.contiguous()
        relu, none = _lib.CG_ACT_RELU, _lib.CG_ACT_NONE
        mpool = self.pool == "mpool1"
        for lv in self.levels:
            a = lv.filt.forward(x, None, s)
            if lv.b is not None:
                n = lv.z.numel()
                _lib.check("cg_bias_act_forward",
                           self._ba_f(n, lv.M * lv.F, a.data_ptr(), lv.b.data_ptr(), relu,
                                      lv.z.data_ptr(), s))
                a = lv.z
            if lv.p > 1:
                args = (a.data_ptr(), N, lv.M, lv.F, lv.p, lv.pooled.data_ptr())
                if mpool:
                    args += (lv.argmax.data_ptr(),)
                _lib.check("cg_pool_forward", self._pool_f(*args, s))
                a = lv.pooled
            x = a
        drop = self._dropped = bool(dropout) and self.keep < 1.0
        if drop:
            self.drop_seeds = [(b + _STREAM_STEP * self._drop_calls) & ((1 << 64) - 1)
                               for b in self._drop_base]
            self._drop_calls += 1
        for j, fc in enumerate(self.fcs):
            fc.x = x  # [N, Min] (a conv level's buffer read flat)
            yp = fc.y.data_ptr()
            _lib.check("cg_gemm_f32", self._gemm(0, 0, N, fc.Mout, fc.Min, x.data_ptr(), fc.Min,
                                                 fc.W.data_ptr(), fc.Mout, yp, fc.Mout, s))
            _lib.check("cg_bias_act_forward",
                       self._ba_f(N * fc.Mout, fc.Mout, yp, fc.b.data_ptr(), relu if fc.relu else none,
                                  yp, s))
            x = fc.y
            if drop and fc.drop is not None:
                _lib.check("cg_dropout_forward",
                           self._drop_f(yp, N * fc.Mout, ctypes.c_float(self.keep), self.drop_seeds[j],
                                        fc.drop.data_ptr(), s))
                x = fc.drop
        return x

    # -- loss -------------------------------------------------------------------------
    def _labels(self, labels):
        if isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32:
            labels = labels.contiguous()
        else:
            labels = ops.class_labels(labels, self.C, self.device)
        if labels.numel() != self.N:
            raise ValueError(f"labels must be [{self.N}] class ids")
        return labels

    def _loss(self, out, labels, s, train: bool = True, pred=None, correct=None):
        """loss (L2 term included), and for a training step dlogits into ``dout``
        and the loss moving average; ``status`` keeps the first out-of-range row + 1."""
        labels = self._labels(labels)
        st = self._xent(out.data_ptr(), labels.data_ptr(), self.N, self.C, self.flat.data_ptr(),
                        self.reg_begin, self.reg_n, ctypes.c_float(self.regularization),
                        self.loss.data_ptr(), self.dout.data_ptr() if train else None,
                        self.ema.data_ptr() if train else None, ctypes.c_float(0.9),
                        ops._p(pred), ops._p(correct), self.status.data_ptr(),
                        self.xws.data_ptr(), self.xws_n, s)
        _lib.check("cg_class_xent_ema", st)

    # -- backward -----------------------------------------------------------------------
    def backward(self, dout, stream=None):
        """Every gradient of the last forward from d(logits) [N, C]; each view of the
        bucket is written, none accumulated into."""
        s = self._stream(stream)
        N = self.N
        relu, none = _lib.CG_ACT_RELU, _lib.CG_ACT_NONE
        dy = dout
        for j in range(len(self.fcs) - 1, -1, -1):
            fc = self.fcs[j]
            if self._dropped and fc.drop is not None:
                _lib.check("cg_dropout_backward",
                           self._drop_b(dy.data_ptr(), N * fc.Mout, ctypes.c_float(self.keep),
                                        self.drop_seeds[j], fc.ddrop.data_ptr(), s))
                dy = fc.ddrop
            dz = fc.dz if fc.relu else dy  # no activation: dz = dy, in place
            _lib.check("cg_bias_act_backward",
                       self._ba_b(N * fc.Mout, fc.Mout, dy.data_ptr(), fc.y.data_ptr(),
                                  relu if fc.relu else none, dz.data_ptr(), fc.db.data_ptr(), 0,
                                  self.ws.data_ptr(), self.ws_n, s))
            # dW [Min, Mout] = x^T dz;  dx [N, Min] = dz W^T
            _lib.check("cg_gemm_f32", self._gemm(1, 0, fc.Min, fc.Mout, N, fc.x.data_ptr(), fc.Min,
                                                 dz.data_ptr(), fc.Mout, fc.dW.data_ptr(), fc.Mout, s))
            if fc.dx is not None:
                _lib.check("cg_gemm_f32", self._gemm(0, 1, N, fc.Min, fc.Mout, dz.data_ptr(), fc.Mout,
                                                     fc.W.data_ptr(), fc.Mout, fc.dx.data_ptr(),
                                                     fc.Min, s))
            dy = fc.dx
        mpool = self.pool == "mpool1"
        for lv in reversed(self.levels):
            if lv.p > 1:
                args = (dy.data_ptr(),) + ((lv.argmax.data_ptr(),) if mpool else ())
                _lib.check("cg_pool_backward",
                           self._pool_b(*args, N, lv.M, lv.F, lv.p, lv.dpool.data_ptr(), s))
                dy = lv.dpool
            if lv.b is not None:  # b2relu: mask and db here, the filter has no activation
                n = lv.z.numel()
                _lib.check("cg_bias_act_backward",
                           self._ba_b(n, lv.M * lv.F, dy.data_ptr(), lv.z.data_ptr(), relu,
                                      lv.dz.data_ptr(), lv.db.data_ptr(), 0, self.ws.data_ptr(),
                                      self.ws_n, s))
                lv.filt.backward(lv.dz, None, lv.dx, False, s)
            else:
                lv.filt.backward(dy, lv.dz, lv.dx, False, s)
            dy = lv.dx

    def _optimizer_launch(self, lr: float, scale: float, s):
        if self.momentum == 0.0 and (self.regularization == 0.0 or self.reg_n == 0):
            return super()._optimizer_launch(lr, scale, s)  # cg_sgd_update
        f = ctypes.c_float
        st = self._mom(self.flat.data_ptr(), self.grad.data_ptr(),
                       self.accum.data_ptr() if self.momentum != 0.0 else None, self.flat.numel(),
                       f(lr), f(self.momentum), f(scale), f(self.regularization), self.reg_begin,
                       self.reg_n, s)
        _lib.check("cg_momentum_update", st)

    def train_step(self, x, labels, stream=None):
        """One optimizer step on this rank's batch x [N, M0, Fin] with class ids
        ``labels`` [N] (an int32 device tensor, or host integers, which are
        validated against [0, C) and uploaded); returns the device loss [1]."""
        return super().train_step(x, labels, stream)

    # -- inference ----------------------------------------------------------------------
    def predict(self, data, labels=None):
        """lib/models.py's predict for the classifier: the predicted class of every
        sample, int64 [size] on the host, over batches of N with the last one
        zero-padded; with ``labels`` also ``loss * batch_size / size`` where loss
        is the plain sum of the batches' losses (L2 term included, the padded
        rows labelled 0: the reference's quirk, as ``evaluate.predict`` keeps it).
        No dropout; no parameter, slot, moving average or step count changes."""
        f32 = dict(device=self.device, dtype=torch.float32)
        data = torch.as_tensor(data).to(**f32)
        if data.dim() == 2:
            data = data.unsqueeze(2)
        size, N = int(data.shape[0]), self.N
        if labels is not None:
            labels = ops.class_labels(labels, self.C, self.device)
            if int(labels.shape[0]) != size:
                raise ValueError("data and labels differ in their number of samples")
        preds = torch.empty((size,), device=self.device, dtype=torch.int32)
        pb = torch.empty((N,), device=self.device, dtype=torch.int32)
        zeros = torch.zeros((N,), device=self.device, dtype=torch.int32)
        s = self._stream(None)
        loss = 0.0
        with torch.no_grad():
            for begin in range(0, size, N):
                end = min(begin + N, size)
                batch, bl = data[begin:end], None if labels is None else labels[begin:end]
                if end - begin < N:
                    batch = torch.zeros((N,) + tuple(data.shape[1:]), **f32)
                    batch[:end - begin] = data[begin:end]
                    if labels is not None:
                        bl = torch.zeros((N,), device=self.device, dtype=torch.int32)
                        bl[:end - begin] = labels[begin:end]
                out = self.forward(batch.contiguous(), dropout=False)
                self._loss(out, bl if bl is not None else zeros, s, train=False, pred=pb)
                if labels is not None:
                    loss += float(self.loss)
                preds[begin:end] = pb[:end - begin]
        preds = preds.cpu().numpy().astype(np.int64)
        return preds if labels is None else (preds, loss * N / size)

    def evaluate(self, data, labels):
        """lib/models.py's evaluate: (string, accuracy %, weighted-F1 %, loss,
        predictions); F1 from the confusion matrix on the host (``weighted_f1``)."""
        preds, loss = self.predict(data, labels)
        lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64)
        ncorrect = int((preds == lab).sum())
        accuracy = 100.0 * ncorrect / len(lab)
        f1 = 100.0 * weighted_f1(lab, preds)
        string = "accuracy: {:.2f} ({:d} / {:d}), f1 (weighted): {:.2f}, loss: {:.2e}".format(
            accuracy, ncorrect, len(lab), f1, loss)
        return string, accuracy, f1, loss, preds

    # -- fit's hooks: class ids, int32 on the device --------------------------------------
    def _fit_set(self, name, d, l):
        d = torch.as_tensor(d).to(device=self.device, dtype=torch.float32)
        if d.dim() == 2:
            d = d.unsqueeze(2)
        d = d.contiguous()
        if d.dim() != 3 or tuple(d.shape[1:]) != (self.M0, self.Fin):
            raise ValueError(f"fit: {name}_data must be [samples, {self.M0}, {self.Fin}], got "
                             f"{tuple(d.shape)}")
        l = ops.class_labels(l, self.C, self.device)
        if l.dim() != 1 or int(l.shape[0]) != int(d.shape[0]):
            raise ValueError(f"fit: {name}_labels must be [samples] class ids")
        return d, l

    def _fit_label_batch(self):
        return torch.empty((self.N,), device=self.device, dtype=torch.int32)
