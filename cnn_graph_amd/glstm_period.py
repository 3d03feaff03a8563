"""The closeness / period / trend gconv-LSTM networks of ``GconvModel``
(lib/gconv_lstm.py:431-607) -- what nips2016/gconvTest.py builds for every
inference function with "expand" in its name (:121-126) from the windows of
``load_ln_data_period(closeness, period, trend)`` -- trained as ``GraphModel``
trains them:

  x [N, M, C]    branch b reads the columns [F S_b, F (S_b + T_b)) (S_b the prefix
                 sum of T; :472-479) and unstacks them in time (:486-487): step t,
                 feature f is column F S_b + f T_b + t
  merge_{b}      per branch ITS OWN glstm_layer -- layer_count GConvLSTMCells, each
                 in its own DropoutWrapper(keep_prob) -- read at the last step
  merge by weights   ``inference_glstm_period_expand`` (:470-500) and
                 ``inference_glstm_period_expand_gconv1`` (:502-534; the same network,
                 the filter's variable one scope higher):
                 y_b = filter(dropout(h_T^b); W_b [H -> out]),  out = sum_b y_b w_b
                 with w_b [M, out] (ops.branch_merge: cg_branch_merge_forward, and
                 ONE cg_branch_merge_backward for every branch)
  merge by concat    ``inference_glstm_period_expand_gconv3`` (:566-607; three
                 branches) and ``inference_glstm_gconv_split`` (:431-468; two branches
                 of Tc steps each on the first 2 F Tc columns):
                 a = concat_b(dropout(h_T^b)) (ops.concat_drop: one pass, no dropped
                 tensors, no concat copy), then conv_init [B H -> num_hidden],
                 conv_layer_num residual layers and output_layer -- ``model._ResNet`` /
                 ``_FourierResNet`` with ``input_grad``, of width ``num_hidden`` (:455,
                 :594; NOT num_hidden_conv); its dx goes back through
                 cg_concat_drop_backward into the branches' dh_T
  loss / update  FlatTrainer's, unchanged: cg_mse_loss_ema, ONE all-reduce of the flat
                 gradient bucket when world > 1, ONE optimizer launch

``inference_glstm_period_expand_gconv2`` (:536-564) is refused: see ``REFUSED``.

Every parameter is a view into one flat buffer, carved in the reference's
creation order -- per branch the cells' Wx, Wh, b per layer, the branch's filter
weight, its merge weight; for the concat networks the head after the last branch
-- and drawn from one generator in that order.  (A branch's cells start 16-byte
aligned in the buffer: up to three zero floats that belong to no variable may
sit in front of them.)  The branches run one after the
other on the caller's stream (the one-launch layer kernel needs its workgroup
pairs co-resident: no second stream competes for the CUs).
"""
from __future__ import annotations

import torch

from . import ops
from .gconv_lstm import carve_cells, lstm_to_hT, make_cells, unstack_time, wrap_cells
from .graph_conv import truncated_normal_
from .model import LSTMHead, _net_class
from .trainer import DropoutEval, FlatTrainer, check_keep_prob, is_fourier_conv

# infer_func -> the scope of the branch filter's variable below merge_{b}/
# (fc_layer opens conv_init, :631-633; gconv1 calls the filter in merge_{b} itself)
WEIGHT_MERGE = {"inference_glstm_period_expand": "conv_init/",
                "inference_glstm_period_expand_gconv1": ""}
# infer_func -> its number of branches (None: one per entry of T)
CONCAT_MERGE = {"inference_glstm_period_expand_gconv3": None, "inference_glstm_gconv_split": 2}
REFUSED = {
    "inference_glstm_period_expand_gconv2":
        "inference_glstm_period_expand_gconv2 (lib/gconv_lstm.py:536-564) puts an extra tf.transpose "
        "in front of tf.unstack(x, T, 3): the unstacked axis then has feat_in entries, not T, so the "
        "reference's own graph build fails for every T != 2 -- there is no behaviour to reproduce",
}
INFER_FUNCS = tuple(WEIGHT_MERGE) + tuple(CONCAT_MERGE)


class GLSTMPeriodModel(LSTMHead, DropoutEval, FlatTrainer):
    """The multi-branch gconv-LSTM on device; ``infer_func`` selects the network
    by the reference's name (``INFER_FUNCS``).  T = (Tc, Tp, Tt): the steps of
    the closeness, period and trend windows."""

    def __init__(self, L, N: int, T=(3, 3, 3), feat_in: int = 2, num_hidden: int = 128, K: int = 2,
                 layer_count: int = 1, conv_layer_num: int = 1, out_features: int = 2,
                 keep_prob: float = 0.8, filter: str = "cheby_conv",
                 infer_func: str = "inference_glstm_period_expand", optimizer: str = "adam",
                 learning_rate: float = 1e-3, decay_rate: float = 0.95, decay_steps: int | None = None,
                 lmax: float = 2, gates: str = "reference", device=None, seed: int = 2017, comm=None):
        if infer_func in REFUSED:
            raise NotImplementedError(REFUSED[infer_func])
        if infer_func not in INFER_FUNCS:
            raise ValueError(f"infer_func must be one of {INFER_FUNCS}, got {infer_func!r}")
        fourier = is_fourier_conv(filter)
        self.keep_prob = check_keep_prob(keep_prob)
        self.infer_func, self.filter = infer_func, filter
        self.concat = infer_func in CONCAT_MERGE
        T = tuple(int(t) for t in ((T,) if isinstance(T, int) else T))
        if CONCAT_MERGE.get(infer_func):  # the split: two branches of Tc steps
            T = (T[0],) * CONCAT_MERGE[infer_func]
        if not 1 <= len(T) <= ops.MAX_BRANCHES or min(T) < 1:
            raise ValueError(f"T must hold 1 to {ops.MAX_BRANCHES} positive step counts, got {T}")
        self.T, self.B = T, len(T)
        self.N, self.F, self.H, self.K = int(N), int(feat_in), int(num_hidden), int(K)
        self.Fout, self.R = int(out_features), int(conv_layer_num)
        # branch b's first column / F (the prefix sums of T)
        self.S = [sum(T[:b]) for b in range(self.B)]
        self.C = self.F * sum(T)  # the columns the branches read
        device = torch.device(device if device is not None else "cuda")
        M, H, Fout, B = int(L.shape[0]), self.H, self.Fout, self.B
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        f32 = dict(device=device, dtype=torch.float32)
        fc_shape = (M, Fout, H) if fourier else (self.K * H, Fout)
        # the reference's creation order, drawn from one generator: per branch the
        # cells, then (merge by weights) the filter weight and the merge weight
        branches, tails = [], []
        for b in range(B):
            branches.append(make_cells(L, self.F, H, self.K, layer_count, lmax, gates, device, gen, filter))
            if not self.concat:
                tails.append((truncated_normal_(torch.empty(fc_shape, **f32), 0.1, gen),
                              truncated_normal_(torch.empty((M, Fout), **f32), 0.1, gen)))
        total = 0
        for b, cells in enumerate(branches):
            # every branch's cells start 16-byte aligned (FlatTrainer.align): the layer
            # kernels read them as float4, and a merge weight [M, out] in front need
            # not be a multiple of four floats
            total += -total % 4 + sum(p.numel() for c in cells for p in c.parameters())
            total += sum(t.numel() for t in tails[b]) if tails else 0
        if self.concat:
            total += sum(_net_class(fourier).sizes(B * H, H, self.K, M, self.R, Fout))
        super().__init__(total, (self.N, branches[0][0]._nNode, Fout), optimizer, learning_rate,
                         decay_rate, decay_steps, device, comm)
        self._graph_from_cell(branches[0][0], gft=self.concat)
        self.cells, self.wrapped = branches, []
        self.fc_W, self.merge_w = [], []
        for b, cells in enumerate(branches):
            scope = f"merge_{b}/"
            self.align(4)
            carve_cells(self, cells, scope)
            # every branch's wrappers draw their own mask streams
            self.wrapped.append(wrap_cells(cells, keep_prob, seed, comm, first=b * int(layer_count)))
            if not self.concat:
                W, w = tails[b]
                self.fc_W.append(self.carve(fc_shape, f"{scope}{WEIGHT_MERGE[infer_func]}weights", init=W)[0])
                self.merge_w.append(self.carve((M, Fout), f"{scope}weight_{b}/weights", init=w)[0])
        if self.concat:  # the head's width is num_hidden (:455, :594)
            self._make_head(fourier, B * H, H, self.R, Fout, gen)
        self._carved()
        self._out = None

    # -- the input split (:472-479, :486-487) ------------------------------------------------
    def split(self, x):
        """x [N, M, C] -> per branch the steps [T_b, N, M, F]: unstack_time on the
        branch's column slice (one copy per branch)."""
        C = self.C
        ok = x.dim() == 3 and tuple(x.shape[:2]) == (self.N, self.M) and x.is_cuda and \
            (x.shape[2] >= C if self.infer_func == "inference_glstm_gconv_split" else x.shape[2] == C)
        if not ok:
            need = f">= {C}" if self.infer_func == "inference_glstm_gconv_split" else str(C)
            raise ValueError(f"x must be a cuda tensor of [N, M, C] = [{self.N}, {self.M}, {need}], "
                             f"got {tuple(x.shape)}")
        F = self.F
        return [unstack_time(x[:, :, F * s:F * (s + t)], t) for s, t in zip(self.S, self.T)]

    def forward(self, x, stream=None, dropout: bool = True):
        """The network's output [N, M, out_features].  ``dropout=False`` runs every
        layer unwrapped.  ``backward`` continues from the state this call leaves."""
        s = self._stream(stream)
        hs, masks = [], []
        for cells, wrapped, xs in zip(self.cells, self.wrapped, self.split(x)):
            # the last layer runs unwrapped and hands its mask out: (keep, seed, offset)
            h, mask = lstm_to_hT(cells, wrapped, xs, dropout)
            hs.append(h)
            masks.append(mask)
        if self.concat:
            keep, seeds = 1.0, None
            if masks[0] is not None:
                keep = masks[0][0]
                seeds = [(seed + ops.DROP_WEYL * off) & ((1 << 64) - 1) for _, seed, off in masks]
            return self._head_forward(ops.concat_drop(hs, keep, seeds), s)
        ys = []
        for h, mask, W in zip(hs, masks, self.fc_W):
            if mask is not None:
                keep, seed, off = mask
                h = ops.dropout(h, keep, seed, offset=off)
            ys.append(ops.fourier_conv(h, W, self.U) if self.filter == "fourier_conv"
                      else ops.cheb_conv(h, W, self.plan, self.K))
        self._out = ops.branch_merge(ys, self.merge_w)
        return self._out

    def backward(self, dout, stream=None):
        """Every gradient of the last forward from d(out) [N, M, out_features], into
        the (zeroed) bucket.  Merge by weights: autograd from the merge down (ONE
        cg_branch_merge_backward, each branch's filter backward, its BPTT).  Merge
        by concat: the head's explicit schedule, then conv_init's dx through
        cg_concat_drop_backward as every branch's dh_T (``LSTMHead``).  An input that
        requires grad gets its ``.grad``."""
        if self.concat:
            return self._head_backward(dout, self._stream(stream))
        self.grad.zero_()
        out, self._out = self._out, None
        if out is not None and out.requires_grad:
            out.backward(dout)
