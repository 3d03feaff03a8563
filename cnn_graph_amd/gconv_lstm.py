"""gconv-LSTM on the HIP Chebyshev path: drop-in for ``lib/gconv_lstm.py``'s
``GConvLSTMCell`` (lib/gconv_lstm.py:29-221) and the ``static_rnn`` over a
``MultiRNNCell`` that ``GconvModel.glstm_layer`` builds (:609-627).

Reference behaviour kept:
  * eight ``cheby_conv`` weights ``W{z,i,f,o}{x,h}t`` of shape [K*feat_in, H]
    and [K*H, H], ``random_uniform(-0.1, 0.1)`` (:98-115), and four biases
    ``b{z,i,f,o}t`` [H] with ``tf.get_variable``'s default (Glorot-uniform)
    initialiser (:173-176); ``K`` defaults to 2 (:95-96);
  * gate functions z = tan, i = f = sigmoid, o = tanh (:188, :195, :202, :209)
    -- ``gates="standard"`` gives the usual tanh / sigmoid instead;
  * ``filter_type="fourier_conv"`` (:59, :116-133): the per-gate variables are
    ``[nNode, feat_out, feat_in]`` spectral weights (``uniform(-0.1, 0.1)``), kept
    concatenated along feat_out as ``Wx`` [M, 4H, Fin] and ``Wh`` [M, 4H, H];
    ``K`` is accepted and ignored (lib/filter.py:32); ``cell.U`` is the device
    Fourier basis;
  * ``forget_bias`` is accepted and ignored, as in the reference (:49);
  * ``__call__(inputs, state) -> (new_h, LSTMStateTuple(new_c, new_h))``.
  * ``DropoutWrapper(cell, output_keep_prob)`` (:616, :623): the cell's outputs
    go through ``tf.nn.dropout`` on a HIP kernel (``ops.dropout``); every
    wrapper draws its own mask stream (a distinct seed per wrapper unless one
    is given), as each TF DropoutWrapper owns an independent random op.
  * ``LSTMStackTrainer``: glstm_layer's cells and wrappers with their parameters
    carved from ``trainer.FlatTrainer``'s flat buffers, and ``lstm_to_hT``, the
    walk to the last step's output -- shared by ``GLSTMModel`` and
    ``glstm_gconv.GLSTMGconvModel``.
  * ``GLSTMModel``: ``inference_glstm`` (:271-281) -- glstm_layer, the last
    step's output, ``fc_layer`` (:629-636) -- with FlatTrainer's MSE loss and
    optimizer step (lib/graph_model.py:246-310; sgd / rmsprop of
    lib/gconvRNN.py:381-389), data parallel with ONE all-reduce of a flat
    gradient bucket per step (config E: batch 512 over 4 GPUs).

Run validation / inference under ``torch.no_grad()``: with gradients enabled a
lost pair hand-off of the one-launch layer is reported when the backward runs
(or at the next layer() call on the plan), not before the forward returns.

MI355X design: the four x-weights (and the four h-weights) are stored
concatenated as one [K*F, 4H] matrix, so a cell step is ONE x-conv plus ONE
h-step, not the reference's eight filters.  With H = 32 on graphs of up to
1024 vertices (config E) the h-step is a single launch
(``cg_lstm_hconv_step``): the Chebyshev basis of h in LDS, the gate
contraction on MFMA and the gate update in its epilogue (``hconv="fused"``);
otherwise it is a chebyshev5 call plus the pointwise kernel.  ``static_rnn``
additionally batches the x-conv of ALL time steps into one call (it does not
depend on the recurrence), runs the T h-steps back to back, and in the
backward sums the h-weight gradient of all steps per Chebyshev order with one
``cg_weight_grad`` over the stacked steps.

The Fourier cell sums the x and h contributions in the spectral domain (the
inverse transform is linear) and synthesises once per step: a layer is one
analysis and one per-frequency contraction for the x part of all steps, then
three launches per step (``cg_flstm_step``: analysis of h on MFMA with the
exact three-term bf16 split, the per-frequency accumulate on MFMA, the
synthesis with the gate update in its epilogue).  ``hconv="unfused"`` (and any
H that is not a multiple of 8) is the composition of ``ops.fourier_conv`` and
the pointwise gate kernel.

Which code runs.  ``hconv="auto"`` resolves to the first row that applies; a
single ``cell(x, state)`` step is ``_StepLayer`` at T = 1 (``_FourierLayer``
for the fused Fourier cell) and never takes the sequence kernel.  Launches
per time step of a layer; the x-conv of all steps, the weight gradients and
the bias gradient are per layer:

  cell              layer() runs     forward, per step        backward, per step
  ----------------  ---------------  -----------------------  -------------------------
  .seq and .seq_x   _SeqLayer        1 / T (x-conv included)  1 (cg_lstm_bwd_step)
  .seq              _SeqLayer        1 / T                    1 (cg_lstm_bwd_step)
  .fused            _StepLayer       1 (cg_lstm_hconv_step)   pointwise + chebyshev5 dx
  neither           _StepLayer       chebyshev5 + pointwise   pointwise + chebyshev5 dx
  Fourier .fused    _FourierLayer    3 (cg_flstm_step)        pointwise + 3
  Fourier unfused   autograd of ops  2 fourier_conv + gates   their backwards

(``.seq``: H = 32, M <= 1024, K <= 4, L~ in LDS; ``.seq_x``: also feat_in <= 8;
``.fused``: H = 32, M <= 1024; Fourier ``.fused``: H a multiple of 8.)
"""
from __future__ import annotations

import collections
import itertools
import math

import torch

from . import _lib
from . import ops
from .graph_conv import truncated_normal_
from .plan import plan_for
from .trainer import DropoutEval, FlatTrainer, check_keep_prob, is_fourier_conv

# distinct default mask streams per DropoutWrapper (TF: one random op each)
_DROPOUT_ORDINAL = itertools.count(1)

_LSTMStateTuple = collections.namedtuple("LSTMStateTuple", ("c", "h"))


class LSTMStateTuple(_LSTMStateTuple):
    """(c, h) -- lib/gconv_lstm.py:16-26."""
    __slots__ = ()

    @property
    def dtype(self):
        c, h = self
        if c.dtype != h.dtype:
            raise TypeError("Inconsistent internal state")
        return c.dtype


GATE_NAMES = ("z", "i", "f", "o")


class GConvLSTMCell:
    """lib/gconv_lstm.py:29-221 on the HIP kernels.  Parameters live in
    ``Wx`` [K*feat_in, 4H], ``Wh`` [K*H, 4H], ``b`` [4H]; ``variables`` maps the
    reference's variable names (``Wzxt``, ``Wiht``, ``bft``, ...) to views.
    With filter_type="fourier_conv" (lib/gconv_lstm.py:116-133) the per-gate
    [nNode, feat_out, feat_in] variables are concatenated along feat_out in
    the order z, i, f, o: ``Wx`` [M, 4H, Fin], ``Wh`` [M, 4H, H]."""

    def __init__(self, num_units, forget_bias=1.0, state_is_tuple=True, activation=None,
                 reuse=None, laplacian=None, lmax=None, K=None, feat_in=None, nNode=None,
                 filter_type="cheby_conv", gates="reference", device=None, generator=None,
                 hconv="auto"):
        self.filter_type = filter_type
        fourier = filter_type == "fourier_conv"
        if not fourier and filter_type != "cheby_conv":
            raise NotImplementedError(f"filter_type={filter_type!r}: the filters on the MI355X path "
                                      "are 'cheby_conv' and 'fourier_conv'")
        if laplacian is None or feat_in is None:
            raise ValueError("laplacian and feat_in are required")
        if gates not in ops.LSTM_GATES:
            raise ValueError(f"gates must be one of {list(ops.LSTM_GATES)}")
        self._num_units = H = int(num_units)
        self._forget_bias = forget_bias          # unused, as in the reference
        self._state_is_tuple = state_is_tuple
        self._laplacian = laplacian
        self._lmax = 2 if lmax is None else lmax  # graph.lmax(normalized L) == 2
        # :95-96; the Fourier filter accepts and ignores it (lib/filter.py:32)
        self._K = K = 2 if K is None else int(K)
        self._feat_in = F = int(feat_in)
        self._nNode = M = int(nNode) if nNode is not None else int(laplacian.shape[0])
        if fourier and M != int(laplacian.shape[0]):
            raise ValueError(f"nNode={M} does not match the Laplacian ({laplacian.shape[0]})")
        self.gates = gates
        self.device = torch.device(device if device is not None else "cuda")
        if not fourier:
            dev_index = self.device.index if self.device.index is not None else 0
            self.plan = plan_for(laplacian, lmax=self._lmax, device=dev_index)
        wx_shape, wh_shape = ((M, 4 * H, F), (M, 4 * H, H)) if fourier else \
            ((K * F, 4 * H), (K * H, 4 * H))
        f32 = dict(device=self.device, dtype=torch.float32)
        with torch.no_grad():
            Wx = torch.empty(wx_shape, **f32).uniform_(-0.1, 0.1, generator=generator)
            Wh = torch.empty(wh_shape, **f32).uniform_(-0.1, 0.1, generator=generator)
            lim = math.sqrt(6.0 / (H + H))  # glorot_uniform of a [H] vector: fan_in = fan_out = H
            b = torch.empty((4 * H,), **f32).uniform_(-lim, lim, generator=generator)
        self.Wx = torch.nn.Parameter(Wx)
        self.Wh = torch.nn.Parameter(Wh)
        self.b = torch.nn.Parameter(b)
        if fourier:
            self._resolve_fourier_hconv(hconv)
        else:
            self._resolve_cheby_hconv(hconv)

    def _resolve_cheby_hconv(self, hconv):
        """h path: "seq" = the whole layer's T steps in one launch
        (cg_lstm_seq_forward) and one launch per BPTT step (cg_lstm_bwd_step);
        "fused" = one launch per forward step (cg_lstm_hconv_step); "unfused"
        = chebyshev5 + pointwise kernel; "auto" picks the first that applies."""
        H, K = self._num_units, self._K
        if hconv not in ("auto", "seq", "fused", "unfused"):
            raise ValueError("hconv must be 'auto', 'seq', 'fused' or 'unfused'")
        supported = ops.lstm_hconv_supported(self.plan, H, K)
        seq_ok = ops.lstm_seq_supported(self.plan, H, K)
        if hconv == "fused" and not supported:
            raise ValueError(f"hconv='fused' needs H = 32 and M <= 1024 (H={H}, M={self.plan.M})")
        if hconv == "seq" and not seq_ok:
            raise ValueError(f"hconv='seq' needs H = 32, M <= 1024, K <= 4 and L~ in LDS "
                             f"(H={H}, M={self.plan.M}, K={K})")
        self.seq = seq_ok and hconv in ("auto", "seq")
        # feat_in <= 8: the x-conv runs inside the sequence kernel too
        self.seq_x = self.seq and ops.lstm_seq_x_supported(self.plan, self._feat_in, H, K)
        self.fused = supported and hconv != "unfused"

    def _resolve_fourier_hconv(self, hconv):
        """h path: "fused" = three launches per step (analysis, per-frequency
        accumulate, synthesis + gates: cg_flstm_step); "unfused" = the
        composition of ops.fourier_conv and the pointwise gate kernel."""
        from . import filter as _filter
        H = self._num_units
        if hconv == "seq":
            raise ValueError("hconv='seq' is a Chebyshev path; the Fourier cell has 'fused' and 'unfused'")
        if hconv not in ("auto", "fused", "unfused"):
            raise ValueError("hconv must be 'auto', 'fused' or 'unfused'")
        supported = ops.flstm_supported(self._nNode, H, self._feat_in)
        if hconv == "fused" and not supported:
            raise ValueError(f"hconv='fused' needs H a multiple of 8 (H={H})")
        self.fused = supported and hconv != "unfused"
        self.seq = self.seq_x = False
        self.U = _filter.fourier_basis(self._laplacian, self.device)  # [M, M], eigenvectors in columns
        # U pre-split into its bf16 terms, kept with the cell
        self.gft_basis = ops.gft_prepare(self.U) if self.fused else None

    # -- reference properties ---------------------------------------------------
    @property
    def state_size(self):
        if self._state_is_tuple:
            return LSTMStateTuple((self._nNode, self._num_units), (self._nNode, self._num_units))
        return 2 * self._num_units

    @property
    def output_size(self):
        return self._num_units

    @property
    def variables(self):
        H = self._num_units
        v = {}
        for q, g in enumerate(GATE_NAMES):
            sl = slice(q * H, (q + 1) * H)  # the gate's feat_out slice: axis 1 for both filters
            v[f"W{g}xt"], v[f"W{g}ht"], v[f"b{g}t"] = self.Wx[:, sl], self.Wh[:, sl], self.b[sl]
        return v

    def parameters(self):
        return [self.Wx, self.Wh, self.b]

    def zero_state(self, batch_size, dtype=torch.float32):
        """(c, h) zeros of [batch, nNode, H] (lib/gconv_lstm.py:71-76)."""
        shape = (int(batch_size), self._nNode, self._num_units)
        return (torch.zeros(shape, device=self.device, dtype=dtype),
                torch.zeros(shape, device=self.device, dtype=dtype))

    # -- one step (lib/gconv_lstm.py:77-221) -----------------------------------------
    def __call__(self, inputs, state, scope=None):
        if self._state_is_tuple:
            c, h = state
        else:
            c, h = torch.split(state, self._nNode, dim=1)  # tf.split(state, 2, axis=1) (:82)
        # a single step is a layer of T = 1 with a given state; a .seq cell steps
        # too (the sequence kernel is layer()'s)
        if self.filter_type == "fourier_conv" and not self.fused:
            new_c, new_h = _fourier_unfused_step(self, inputs, c, h)
        else:
            args = (inputs.unsqueeze(0), c.contiguous(), h.contiguous(), self.Wx, self.Wh, self.b,
                    self, False, True)
            _, new_c, new_h = _FourierLayer.apply(*args) if self.filter_type == "fourier_conv" \
                else _StepLayer.apply(*args, True)
        if self._state_is_tuple:
            new_state = LSTMStateTuple(new_c, new_h)
        else:
            new_state = torch.cat([new_c, new_h], 1)  # tf.concat([new_c, new_h], 1) (:220)
        return new_h, new_state


def _hweight_grad_planes(t0_parts, planes, dpre_parts, H: int, K: int):
    """dWh [K*H, 4H] (row c*K + k) from the Chebyshev orders of h kept as
    planes: order 0 is h itself, given as row blocks t0_parts matched with
    dpre_parts (summed with one cg_weight_grad each, accumulated); order k >= 1
    is planes[k-1] (rows matching the concatenation of dpre_parts)."""
    dev = dpre_parts[0].device
    tmp = torch.empty((K, H, 4 * H), device=dev, dtype=torch.float32)
    for i, (a, d) in enumerate(zip(t0_parts, dpre_parts)):
        ops.weight_grad(a, d, out=tmp[0], accumulate=i > 0)
    dcat = dpre_parts[0] if len(dpre_parts) == 1 else None
    for k in range(1, K):
        if dcat is not None:
            ops.weight_grad(planes[k - 1], dcat, out=tmp[k])
        else:  # the planes' rows follow the concatenation of dpre_parts
            off = 0
            for i, d in enumerate(dpre_parts):
                rows = d.numel() // (4 * H)
                ops.weight_grad(planes[k - 1].reshape(-1, H)[off:off + rows], d, out=tmp[k],
                                accumulate=i > 0)
                off += rows
    return tmp.permute(1, 0, 2).reshape(K * H, 4 * H)


def _prev_state(t: int, zero_init: bool, s0, ss):
    """The state entering step t: ss[t-1], the given s0 at t = 0, None = zero."""
    if t > 0:
        return ss[t - 1]
    return None if zero_init else s0


def _bptt_grads(dhs, dcT, dhT, T: int):
    """What every layer backward starts from: (dc, dh_at) -- dc the contiguous
    gradient of c_T (or None) and dh_at(t) the gradient reaching h_t from
    outside the recurrence (or None).  h_{T-1} is reached twice: through hs
    and through h_T."""
    dhs = dhs.contiguous() if dhs is not None else None
    dc = dcT.contiguous() if dcT is not None else None
    dh_last = None
    if dhT is not None:
        dh_last = dhT.contiguous() if dhs is None else dhs[T - 1] + dhT
    elif dhs is not None:
        dh_last = dhs[T - 1]

    def dh_at(t):
        return dh_last if t == T - 1 else (None if dhs is None else dhs[t])

    return dc, dh_at


def _final_c(ctx, cs, want_c: bool):
    """c_T as an output of its own, or -- the caller does not read it -- an
    empty placeholder that autograd refuses to differentiate (no 16 MB copy)."""
    if want_c:
        return cs[-1].clone()
    z = cs.new_empty(0)
    ctx.mark_non_differentiable(z)
    return z


class _SeqLayer(torch.autograd.Function):
    """static_rnn of one ``cell.seq`` cell over a [T, N, M, F] sequence: all T
    steps in ONE launch (with ``cell.seq_x`` the x-conv too, else the x-conv of
    every step batched in front), BPTT with one launch per step, then the
    weight gradients over all steps at once."""

    @staticmethod
    def forward(ctx, xs, c0, h0, Wx, Wh, b, cell: GConvLSTMCell, zero_init: bool, want_c: bool,
                check_now: bool):
        H, K, plan, gates = cell._num_units, cell._K, cell.plan, cell.gates
        xs = xs.contiguous()
        T, N, M, F = xs.shape
        R = N * M
        f32 = dict(device=xs.device, dtype=torch.float32)
        if cell.seq_x:  # the x-conv inside the sequence kernel; its basis kept as planes
            basis_x = torch.empty((K, T * R, F), **f32)
        else:  # x-conv of every step at once: a batch of T*N samples
            basis_x, gx = ops.cheb_forward(plan, xs.view(T * N, M, F), Wx, K)
        # a hand-off fault of an earlier launch on this plan not reported yet
        ops.lstm_seq_fault(plan, wait=False)
        cs = torch.empty((T, N, M, H), **f32)
        act = torch.empty((T, R, 4 * H), **f32)  # unit-major [R][H][4]
        # The h basis of every step as K planes [K][T+1][R][H] of one buffer:
        # plane 0 at t = h_{t-1} (hs IS plane 0 shifted by one step, slot 0 =
        # h0), planes k >= 1 written by the kernel -- so the h-weight gradient
        # is ONE planes-layout GEMM over all orders and steps
        hp = torch.empty((K, T + 1, R, H), **f32)
        hs = hp[0, 1:].view(T, N, M, H)
        state = dict(h0=None if zero_init else h0, c0=None if zero_init else c0, out_hs=hs,
                     out_cs=cs, out_act=act, planes=hp[1] if K > 1 else None,
                     plane_stride=(T + 1) * R * H)
        if not zero_init:
            hp[0, 0].copy_(h0.reshape(R, H))
        if cell.seq_x:
            if zero_init:  # no h-conv at step 0: zero rows for the one-pass weight gradients
                hp[:, 0].zero_()
            ops.lstm_seq_forward_x(plan, xs, Wx, Wh, b, K, gates, xplanes=basis_x, **state)
        else:
            ops.lstm_seq_forward(plan, gx.view(T, R, 4 * H), Wh, b, K, T, N, gates, **state)
        # a lost pair hand-off leaves NaN in hs / cs / act: an inference call
        # checks the launch before returning its outputs, a training call
        # before its backward consumes them (one event wait, no device sync)
        if check_now:
            ops.lstm_seq_fault(plan, wait=True)
        ctx.save_for_backward(basis_x, hp, Wx, Wh, act, cs, c0)
        ctx.cell, ctx.zero_init, ctx.shape = cell, zero_init, (T, N, M, F)
        # outputs nobody differentiates reach the backward as None (no zero
        # [T, N, M, H] gradient materialised for a sequence read only at its
        # last step: h_T is an output of its own)
        ctx.set_materialize_grads(False)
        return hs, _final_c(ctx, cs, want_c), hs[T - 1].clone()

    @staticmethod
    def backward(ctx, dhs, dcT, dhT):
        basis_x, hp, Wx, Wh, act, cs, c0 = ctx.saved_tensors
        cell, zero_init = ctx.cell, ctx.zero_init
        H, K, plan, gates = cell._num_units, cell._K, cell.plan, cell.gates
        # a fault already known raises now; the blocking check runs after the
        # backward is queued (a wait here would idle the GPU while the host
        # queues the backward), before any gradient is returned
        ops.lstm_seq_fault(plan, wait=False)
        T, N, M, F = ctx.shape
        R = N * M
        dpre = torch.empty((T, R, 4 * H), device=act.device, dtype=torch.float32)
        dc, dh_at = _bptt_grads(dhs, dcT, dhT, T)
        dh_rec = None
        t_first = 1 if zero_init else 0  # first step whose h-conv ran
        for t in range(T - 1, -1, -1):
            # one launch: gates backward, dBasis = dpre Wh^T on MFMA and the
            # reverse recurrence over L~^T -> the gradient of h_{t-1} (None at a
            # step that ran no h-conv: the pointwise part alone)
            _, dc, dh_rec = ops.lstm_bwd_step(plan, dh_at(t), dh_rec, dc, act[t],
                                              _prev_state(t, zero_init, c0, cs), cs[t], Wh, K, gates,
                                              out_dpre=dpre[t], act_unit_major=True,
                                              need_dh_prev=t >= t_first)
        dy = dpre.view(T * N, M, 4 * H)
        need_dx = ctx.needs_input_grad[0]
        if cell.seq_x:
            # dWh, dWx and db in ONE pass over dpre: the h planes of every step
            # (a zero-state layer's step 0 has none: the forward zeroed its slots) and
            # the x planes [K][T*R][F] (dx needs no basis)
            dWh, dWx, db = ops.lstm_weight_grads(hp[0, 0:T].reshape(-1, H), (T + 1) * R * H,
                                                 basis_x[0], T * R * F, K, T * R, dpre)
            dxs = ops.cheb_backward(plan, dy, None, Wx, K, need_dW=False)[0] if need_dx else None
        else:
            if T <= t_first:
                dWh = torch.zeros_like(Wh)
            else:  # one GEMM over the K planes of every step with an h-conv
                dWh = ops.weight_grad_planes(hp[0, t_first:T].reshape(-1, H), (T + 1) * R * H, K,
                                             (T - t_first) * R, dpre[t_first:])
            dxs, dWx = ops.cheb_backward(plan, dy, basis_x, Wx, K, need_dx=need_dx)
            db = ops.bias_grad(dpre)
        # raises CGError if the forward's launch lost a pair hand-off
        ops.lstm_seq_fault(plan, wait=True)
        return (dxs.view(T, N, M, F) if dxs is not None else None, None if zero_init else dc,
                None if zero_init else dh_rec, dWx, dWh, db, None, None, None, None)


class _StepLayer(torch.autograd.Function):
    """static_rnn of one cell over a [T, N, M, F] sequence, one h-step per time
    step (a single cell step is T = 1 with a given state): the x-conv of every
    step batched in front, T h-steps, BPTT per step, then the h-weight
    gradient of all steps summed per Chebyshev order."""

    @staticmethod
    def forward(ctx, xs, c0, h0, Wx, Wh, b, cell: GConvLSTMCell, zero_init: bool, want_c: bool,
                step: bool):
        H, K, plan, gates = cell._num_units, cell._K, cell.plan, cell.gates
        xs = xs.contiguous()
        T, N, M, F = xs.shape
        R = N * M
        f32 = dict(device=xs.device, dtype=torch.float32)
        # x-conv of every step at once: a batch of T*N samples
        basis_x, gx = ops.cheb_forward(plan, xs.view(T * N, M, F), Wx, K)
        gx = gx.view(T, R, 4 * H)
        hs = torch.empty((T, N, M, H), **f32)
        cs = torch.empty((T, N, M, H), **f32)
        act = torch.empty((T, R, 4 * H), **f32)
        # h bases kept for the backward's weight gradient: the fused h-step
        # writes the orders 1..K-1 as planes [K-1][T][R][H] (order 0 is h_prev),
        # chebyshev5 the rows [T][R][H*K]
        if cell.fused:
            hb = torch.empty((max(K - 1, 1), T, R, H), **f32)
        else:
            hb = torch.empty((T, R, H * K), **f32)
            gh = torch.empty((N, M, 4 * H), **f32)
        for t in range(T):
            h_prev = _prev_state(t, zero_init, h0, hs)
            c_prev = _prev_state(t, zero_init, c0, cs)
            if h_prev is None:  # step 0 of a zero-state layer: no h-conv
                ops.lstm_cell_forward(gx[t], None, b, c_prev, H, gates, out_c=cs[t], out_h=hs[t],
                                      out_act=act[t])
            elif cell.fused:  # one launch: h-conv + gates
                ops.lstm_hconv_step(plan, h_prev, c_prev, gx[t], Wh, b, K, gates, out_c=cs[t],
                                    out_h=hs[t], out_act=act[t], planes=hb[0, t],
                                    plane_stride=T * R * H)
            else:
                ops.cheb_forward(plan, h_prev, Wh, K, out_basis=hb[t], out_y=gh)
                ops.lstm_cell_forward(gx[t], gh, b, c_prev, H, gates, out_c=cs[t], out_h=hs[t],
                                      out_act=act[t])
        ctx.save_for_backward(basis_x, hb, Wx, Wh, act, cs, c0, h0, hs)
        ctx.cell, ctx.zero_init, ctx.shape = cell, zero_init, (T, N, M, F)
        ctx.set_materialize_grads(False)  # (as in _SeqLayer)
        if step:  # the caller reads (c, h) of its one step, not hs: no copies
            return None, cs[0], hs[0]
        return hs, _final_c(ctx, cs, want_c), hs[T - 1].clone()

    @staticmethod
    def backward(ctx, dhs, dcT, dhT):
        basis_x, hb, Wx, Wh, act, cs, c0, h0, hs = ctx.saved_tensors
        cell, zero_init = ctx.cell, ctx.zero_init
        H, K, plan = cell._num_units, cell._K, cell.plan
        T, N, M, F = ctx.shape
        R = N * M
        dpre = torch.empty((T, R, 4 * H), device=act.device, dtype=torch.float32)
        dc, dh_at = _bptt_grads(dhs, dcT, dhT, T)
        dh_rec = None
        t_first = 1 if zero_init else 0  # first step whose h-conv ran
        # a lone unfused step: its h-conv's backward gives dWh along with dh
        lone = T == 1 and t_first == 0 and not cell.fused
        for t in range(T - 1, -1, -1):
            dc, dh_rec, dWh = _bptt_step(cell, dh_at(t), dh_rec, dc, act[t],
                                         _prev_state(t, zero_init, c0, cs), cs[t], Wh, dpre[t],
                                         None if cell.fused else hb[t], t >= t_first, lone)
        if T <= t_first:
            dWh = torch.zeros_like(Wh)
        elif cell.fused:
            t0_parts, dparts = [], []
            if t_first == 0:  # step 0 ran its h-conv on h0
                t0_parts.append(h0.reshape(R, H))
                dparts.append(dpre[0])
            if T > 1:
                t0_parts.append(hs[0:T - 1].reshape(-1, H))
                dparts.append(dpre[1:T])
            dWh = _hweight_grad_planes(t0_parts, [hb[k, t_first:T] for k in range(K - 1)], dparts,
                                       H, K)
        elif not lone:
            dWh = ops.weight_grad(hb[t_first:], dpre[t_first:])
        dxs, dWx = ops.cheb_backward(plan, dpre.view(T * N, M, 4 * H), basis_x, Wx, K,
                                     need_dx=ctx.needs_input_grad[0])
        db = ops.bias_grad(dpre)
        return (dxs.view(T, N, M, F) if dxs is not None else None, None if zero_init else dc,
                None if zero_init else dh_rec, dWx, dWh, db, None, None, None, None)


def _bptt_step(cell, dh, dh_rec, dc, act, c_prev, c_out, Wh, dpre, basis_h, h_ran: bool,
               need_dW: bool):
    """One BPTT step of _StepLayer: dpre [R, 4H] filled; returns (dc_prev,
    dh_prev or None if the step ran no h-conv, dWh if need_dW).  A ``cell.seq``
    cell (a single step of it: its layers are _SeqLayer's) has the one-launch
    backward step; the others the pointwise kernel plus chebyshev5's backward."""
    H, K, plan, gates = cell._num_units, cell._K, cell.plan, cell.gates
    if cell.seq:
        _, dc_prev, dh_prev = ops.lstm_bwd_step(plan, dh, dh_rec, dc, act, c_prev, c_out, Wh, K,
                                                gates, out_dpre=dpre, need_dh_prev=h_ran)
        return dc_prev, dh_prev, None
    _, dc_prev = ops.lstm_cell_backward(dh, dh_rec, dc, act, c_prev, c_out, H, gates, out_dpre=dpre)
    if not h_ran:
        return dc_prev, None, None
    dh_prev, dWh = ops.cheb_backward(plan, dpre.view(-1, plan.M, 4 * H), basis_h, Wh, K,
                                     need_dW=need_dW)
    return dc_prev, dh_prev, dWh


class _FourierGates(torch.autograd.Function):
    """The pointwise gate update on pre-activation parts gx, gh [N, M, 4H]
    (ops.lstm_cell_forward / backward) for the unfused Fourier composition."""

    @staticmethod
    def forward(ctx, gx, gh, b, c, H, gates):
        c = c.contiguous()
        c_out, h_out, act = ops.lstm_cell_forward(gx.contiguous(), gh.contiguous(), b, c, H, gates)
        ctx.save_for_backward(act, c, c_out)
        ctx.H, ctx.gates = H, gates
        return c_out, h_out

    @staticmethod
    def backward(ctx, dc_out, dh_out):
        act, c, c_out = ctx.saved_tensors
        dh = dh_out.contiguous() if dh_out is not None else None
        dc = dc_out.contiguous() if dc_out is not None else None
        dpre, dc_prev = ops.lstm_cell_backward(dh, None, dc, act, c, c_out, ctx.H, ctx.gates)
        return dpre, dpre, ops.bias_grad(dpre), dc_prev, None, None


def _fourier_unfused_step(cell, x, c, h):
    """(c', h') as the composition of the existing ops: two spectral filters
    with the concatenated weights and the pointwise gate kernel."""
    gx = ops.fourier_conv(x, cell.Wx, cell.U)
    gh = ops.fourier_conv(h, cell.Wh, cell.U)
    return _FourierGates.apply(gx, gh, cell.b, c, cell._num_units, cell.gates)


class _FourierLayer(torch.autograd.Function):
    """static_rnn of one Fourier cell over a [T, N, M, F] sequence (a single
    cell step is T = 1).  Forward: ONE analysis of all T*N inputs, ONE
    per-frequency contraction giving the x part of every step's spectral
    pre-activations, then per step the three-launch h-step (cg_flstm_step; step
    0 of a zero-state layer is the synthesis + gates alone).  Backward: per
    step the gate backward, the analysis of dpre, the transposed contraction
    with Wh and a synthesis give the gradient of h_{t-1}; after the loop dWh
    and dWx are ONE weight-gradient launch each over the stacked steps."""

    @staticmethod
    def forward(ctx, xs, c0, h0, Wx, Wh, b, cell: GConvLSTMCell, zero_init: bool, want_c: bool):
        H, gates, basis = cell._num_units, cell.gates, cell.gft_basis
        xs = xs.contiguous()
        T, N, M, F = xs.shape
        f32 = dict(device=xs.device, dtype=torch.float32)
        xhat = ops.gft(basis, xs.view(T * N, M, F))
        ghx = ops.fourier_mix("fwd", Wx, x=xhat).view(T, N, M, 4 * H)
        hs = torch.empty((T, N, M, H), **f32)
        cs = torch.empty((T, N, M, H), **f32)
        act = torch.empty((T, N, M, 4 * H), **f32)
        hhat = torch.empty((T, N, M, H), **f32)  # U^T h_{t-1}: the weight gradient's operand
        for t in range(T):
            ops.flstm_step(basis, _prev_state(t, zero_init, h0, hs), _prev_state(t, zero_init, c0, cs),
                           ghx[t], Wh, b, gates, out_c=cs[t], out_h=hs[t], out_act=act[t],
                           out_hhat=hhat[t])
        ctx.save_for_backward(xhat, hhat, Wx, Wh, act, cs, c0)
        ctx.cell, ctx.zero_init, ctx.shape = cell, zero_init, (T, N, M, F)
        ctx.set_materialize_grads(False)
        return hs, _final_c(ctx, cs, want_c), hs[T - 1].clone()

    @staticmethod
    def backward(ctx, dhs, dcT, dhT):
        xhat, hhat, Wx, Wh, act, cs, c0 = ctx.saved_tensors
        cell, zero_init = ctx.cell, ctx.zero_init
        H, gates, basis = cell._num_units, cell.gates, cell.gft_basis
        T, N, M, F = ctx.shape
        f32 = dict(device=act.device, dtype=torch.float32)
        dpre = torch.empty((T, N, M, 4 * H), **f32)
        dghat = torch.empty((T, N, M, 4 * H), **f32)
        dc, dh_at = _bptt_grads(dhs, dcT, dhT, T)
        dh_rec = None
        t_first = 1 if zero_init else 0  # first step whose h part ran
        dhhat = torch.empty((N, M, H), **f32)
        for t in range(T - 1, -1, -1):
            _, dc = ops.lstm_cell_backward(dh_at(t), dh_rec, dc, act[t], _prev_state(t, zero_init, c0, cs),
                                           cs[t], H, gates, out_dpre=dpre[t])
            ops.gft(basis, dpre[t], out=dghat[t])  # a = U ghat  ->  d ghat = U^T dpre
            if t >= t_first:
                ops.fourier_mix("t", Wh, g=dghat[t], out=dhhat)
                dh_rec = ops.gft(basis, dhhat, inverse=True)
            else:
                dh_rec = None
        if T > t_first:  # the stacked (t, n) rows of every step with an h part, one launch
            dWh = ops.fourier_mix("dw", x=hhat[t_first:], g=dghat[t_first:])
        else:
            dWh = torch.zeros_like(Wh)
        dWx = ops.fourier_mix("dw", x=xhat, g=dghat)
        db = ops.bias_grad(dpre)
        dxs = None
        if ctx.needs_input_grad[0]:
            dxhat = ops.fourier_mix("t", Wx, g=dghat.view(T * N, M, 4 * H))
            dxs = ops.gft(basis, dxhat, inverse=True).view(T, N, M, F)
        return (dxs, None if zero_init else dc, None if zero_init else dh_rec, dWx, dWh, db,
                None, None, None)


def _fourier_unfused_layer(cell, xs, initial_state, final_c):
    """layer() for the unfused Fourier cell: the composition, step by step under autograd."""
    c, h = cell.zero_state(xs.shape[1]) if initial_state is None else initial_state
    outs = []
    for t in range(xs.shape[0]):
        c, h = _fourier_unfused_step(cell, xs[t], c, h)
        outs.append(h)
    return torch.stack(outs), LSTMStateTuple(c if final_c else c.new_empty(0), h)


class DropoutWrapper:
    """tf.nn.rnn_cell.DropoutWrapper(cell, output_keep_prob) as glstm_layer
    wraps every layer's cell (lib/gconv_lstm.py:616, :623): the cell's OUTPUTS
    go through tf.nn.dropout (ops.dropout: a HIP kernel, mask regenerated in the
    backward from a per-call seed), its state passes through untouched.  Like
    the reference graph, it drops whenever it is applied (there is no training
    flag); output_keep_prob = 1 is the identity.  The mask stream is seeded
    from ``seed`` and advances every call (TF's own random stream is not
    reproducible here, only its semantics).  With ``seed=None`` every wrapper
    gets its own stream (torch.initial_seed() mixed with the wrapper's creation
    ordinal), so two same-shaped layers never share masks."""

    def __init__(self, cell: GConvLSTMCell, output_keep_prob: float = 1.0, seed: int | None = None):
        self.cell = cell
        self.output_keep_prob = check_keep_prob(output_keep_prob, "output_keep_prob")
        if seed is None:
            seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + next(_DROPOUT_ORDINAL) * 0xBF58476D1CE4E5B9)
        self._seed = int(seed) & ((1 << 64) - 1)
        self._calls = 0

    def next_seed(self) -> int:
        self._calls += 1
        return (self._seed + 0xD1B54A32D192ED03 * self._calls) & ((1 << 64) - 1)

    def __getattr__(self, name):  # state_size, output_size, zero_state, parameters, ...
        # only reached for names not found normally; 'cell' itself missing means
        # an instance built without __init__ (copy / pickle probing): no recursion
        if name == "cell" or name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.cell, name)

    def __call__(self, inputs, state, scope=None):
        out, new_state = self.cell(inputs, state, scope)
        return ops.dropout(out, self.output_keep_prob, self.next_seed()), new_state


def layer(cell, xs: torch.Tensor, initial_state=None, final_c: bool = True):
    """Run ``cell`` over xs [T, N, M, feat_in]; returns (hs [T, N, M, H],
    LSTMStateTuple(c_T, h_T)).  initial_state None = zero state; final_c False
    = the caller does not read c_T (an empty tensor in its place, no copy).

    On the one-launch path a lost pair hand-off (cg_lstm_seq_fault) raises
    CGError: here when no gradient will be taken (the outputs go straight to
    the caller), else in the backward, before any gradient is returned (the
    outputs then hold NaN from the lost step on).

    ``cell`` may be a DropoutWrapper: the returned outputs are then dropped
    out, the state (c_T, h_T) is not (DropoutWrapper semantics)."""
    if isinstance(cell, DropoutWrapper):
        hs, state = layer(cell.cell, xs, initial_state, final_c)
        return ops.dropout(hs, cell.output_keep_prob, cell.next_seed()), state
    fourier = cell.filter_type == "fourier_conv"
    if fourier and not cell.fused:
        return _fourier_unfused_layer(cell, xs, initial_state, final_c)
    zero_init = initial_state is None
    if zero_init:
        c0 = h0 = xs.new_empty(0)  # placeholders: a zero state is never read (no fill launch)
    else:
        c0, h0 = (s.contiguous() for s in initial_state)
    args = (xs, c0, h0, cell.Wx, cell.Wh, cell.b, cell, zero_init, final_c)
    if fourier:
        hs, cT, hT = _FourierLayer.apply(*args)
    elif cell.seq:
        # nobody will call a backward: the sequence launch is checked before returning
        check_now = not (torch.is_grad_enabled() and any(t.requires_grad for t in args[:6]))
        hs, cT, hT = _SeqLayer.apply(*args, check_now)
    else:
        hs, cT, hT = _StepLayer.apply(*args, False)
    return hs, LSTMStateTuple(cT, hT)


def static_rnn(cells, inputs, initial_states=None):
    """``tf.nn.static_rnn(MultiRNNCell(cells), inputs)`` (lib/gconv_lstm.py:625-626).

    inputs: a list of T tensors [N, M, F] or one [T, N, M, F] tensor.
    Returns (outputs: list of T tensors [N, M, H] of the last layer,
    states: tuple of LSTMStateTuple per layer).  Layer-by-layer evaluation
    equals the reference's time-major one (layer l at step t depends only on
    layer l-1 at step t and layer l at step t-1)."""
    if isinstance(cells, (GConvLSTMCell, DropoutWrapper)):
        cells = [cells]
    xs = torch.stack(list(inputs)) if isinstance(inputs, (list, tuple)) else inputs
    states = []
    for li, cell in enumerate(cells):
        init = None if initial_states is None else initial_states[li]
        xs, st = layer(cell, xs, init)
        states.append(st)
    return list(xs.unbind(0)), tuple(states)


def clip_gradients(params, max_grad_norm, check_numerics: bool = True):
    """gconvRNN.Model._build_optim's gradient clipping (lib/gconvRNN.py:392-402)
    on the parameters' .grad: per variable tf.clip_by_norm(grad, max_grad_norm)
    then tf.check_numerics (raises FloatingPointError on NaN / Inf), in place
    on the HIP kernels.  max_grad_norm None = no clipping (the reference's else
    branch)."""
    if max_grad_norm is None:
        return
    grads = [p.grad for p in params if p.grad is not None]
    ops.clip_by_norm_(grads, float(max_grad_norm), check_numerics)


def unstack_time(x: torch.Tensor, T: int) -> torch.Tensor:
    """inference_glstm's split (lib/gconv_lstm.py:272-275): [N, M, F*T] ->
    reshape [N, M, F, T] -> unstack axis 3 -> [T, N, M, F] (contiguous)."""
    N, M, C = x.shape
    return x.reshape(N, M, C // T, T).permute(3, 0, 1, 2).contiguous()


def dropout_seed(seed: int, rank: int, layer: int) -> int:
    """A 64-bit mask-stream seed from (model seed, rank, layer index): a
    splitmix64 finaliser over the three (deterministic across processes, unlike
    Python's salted ``hash``)."""
    z = (int(seed) * 0x9E3779B97F4A7C15 + int(rank) * 0xBF58476D1CE4E5B9 +
         (int(layer) + 1) * 0x94D049BB133111EB) & ((1 << 64) - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
    return z ^ (z >> 31)


def lstm_to_hT(cells, wrapped, xs, dropout: bool):
    """static_rnn(wrapped, xs) then outputs[-1], with the last layer's sequence
    read at its last step only.  Returns (h_T, mask): that layer runs unwrapped,
    and its h_T (a separate output: the backward gets no zero [T, N, M, H]
    gradient) is still to go through ``mask`` = (keep_prob, seed, offset), the
    last-step slice of the layer's mask stream (element offset (T-1) N M H) --
    the values and gradients of the whole-sequence form, 1/T of its dropout
    traffic.  The caller applies it (``ops.dropout``) or folds it into what
    reads h_T.  ``dropout=False`` runs every layer unwrapped; mask is None then,
    and when the layers have no wrapper."""
    last = len(cells) - 1
    for li in range(last):
        xs, _ = layer(wrapped[li] if dropout else cells[li], xs, final_c=False)
    _, st = layer(cells[last], xs, final_c=False)
    w = wrapped[last]
    if dropout and isinstance(w, DropoutWrapper):
        return st.h, (w.output_keep_prob, w.next_seed(), (xs.shape[0] - 1) * st.h.numel())
    return st.h, None


def make_cells(L, feat_in, H, K, layer_count, lmax, gates, device, gen, filter, hconv="auto"):
    """glstm_layer's cells (lib/gconv_lstm.py:609-627): layer_count GConvLSTMCells,
    the first reading feat_in features, the others H; their initial values are
    drawn from ``gen`` in creation order."""
    return [GConvLSTMCell(H, laplacian=L, lmax=lmax, K=K, feat_in=feat_in if li == 0 else H,
                          gates=gates, device=device, generator=gen, filter_type=filter, hconv=hconv)
            for li in range(int(layer_count))]


def carve_cells(trainer: FlatTrainer, cells, scope: str = ""):
    """Move every cell's Wx, Wh, b into the trainer's flat buffers (the next
    views ``carve`` hands out), as autograd-owned Parameters whose ``.grad`` is
    the bucket view; ``scope`` prefixes the variable names."""
    for li, c in enumerate(cells):
        for n in ("Wx", "Wh", "b"):
            t = getattr(c, n).detach()
            name = f"{scope}gconv_lstm_layer/rnn/multi_rnn_cell/cell_{li}/{n}"
            setattr(c, n, trainer.carve(t.shape, name, init=t)[0])


def wrap_cells(cells, keep_prob, seed, comm, first: int = 0):
    """Each cell in its DropoutWrapper(keep_prob) (the cell itself at keep_prob
    1).  Each wrapper's mask stream comes from (model seed, rank, first + layer):
    training is reproducible from the seed, and the ranks draw independent
    masks for their shards (TF: one random op per wrapper per replica)."""
    rank = int(getattr(comm, "rank", 0)) if comm is not None else 0
    return [DropoutWrapper(c, keep_prob, seed=dropout_seed(seed, rank, first + li))
            if keep_prob < 1.0 else c for li, c in enumerate(cells)]


class LSTMStackTrainer(DropoutEval, FlatTrainer):
    """The part ``GLSTMModel``, ``GLSTMGconvModel`` and ``GConvRNNModel`` share:
    ``glstm_layer`` (lib/gconv_lstm.py:609-627) -- layer_count GConvLSTMCells, each
    in a DropoutWrapper(keep_prob) -- with every cell's Wx, Wh, b carved from the
    flat buffers first, as autograd-owned Parameters whose ``.grad`` is the bucket
    view.  ``tail_numel`` parameters follow, for the subclass to carve (drawing
    from ``self._gen``, after the cells' own initial draws).  ``head``: a residual
    head follows (``_graph_from_cell``'s ``gft``)."""

    def __init__(self, L, N, T, feat_in, num_hidden, K, layer_count, out_features, keep_prob, filter,
                 tail_numel, optimizer, learning_rate, decay_rate, decay_steps, lmax, gates, device,
                 seed, comm, hconv="auto", head=False):
        is_fourier_conv(filter)
        self.filter = filter
        self.N, self.T, self.F, self.H, self.K = int(N), int(T), int(feat_in), int(num_hidden), int(K)
        self.Fout = int(out_features)
        device = torch.device(device if device is not None else "cuda")
        self._gen = gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        cells = make_cells(L, self.F, self.H, self.K, layer_count, lmax, gates, device, gen, filter, hconv)
        super().__init__(sum(p.numel() for c in cells for p in c.parameters()) + tail_numel,
                         (self.N, cells[0]._nNode, self.Fout), optimizer, learning_rate, decay_rate,
                         decay_steps, device, comm)
        self._graph_from_cell(cells[0], gft=head)
        carve_cells(self, cells)
        self.cells = cells
        self.wrapped = wrap_cells(cells, keep_prob, seed, comm)

    def _steps(self, x):
        if x.dim() == 3:  # [N, M, F*T] as the reference feeds it
            return unstack_time(x, self.T)
        return x.contiguous()


class GLSTMModel(LSTMStackTrainer):
    """``GconvModel.inference_glstm`` (lib/gconv_lstm.py:271-281) trained as
    ``GraphModel`` trains it (lib/graph_model.py:246-310):

      x [N, M, F*T]  --unstack time (:272-275)-->  T x [N, M, F]
      glstm_layer    layer_count GConvLSTMCells under static_rnn (:609-627),
                     each in a DropoutWrapper(output_keep_prob) (:616, :623)
      fc_layer       out = cheby_conv(outputs[-1]; W_fc [K*H, Fout]) (:629-636); with
                     filter="fourier_conv" the cells and the fc layer use the
                     Fourier filter (Wx [M, 4H, Fin], Wh [M, 4H, H], W_fc [M, Fout, H])
      loss / exchange / update   FlatTrainer's: cg_mse_loss_ema, ONE all-reduce(sum)
                     of the flat gradient bucket (world > 1), ONE optimizer launch
                     with grad_scale = 1/world: Adam (graph_model.py:293, staircase
                     exponential decay) or gconvRNN's sgd / rmsprop
                     (lib/gconvRNN.py:381-389)

    Every parameter (each layer's Wx [K*Fin, 4H], Wh [K*H, 4H], b [4H], then
    W_fc) is a view into one flat fp32 buffer and its ``.grad`` a view into one
    flat gradient bucket that autograd accumulates into in place -- at config E
    (Fin 2, H 32, K 3, one layer) 13 376 floats = 53.5 KB -- so the data-parallel
    exchange of a step is one collective and the update one launch."""

    def __init__(self, L, N: int, T: int, feat_in: int, num_hidden: int = 32, K: int = 3,
                 layer_count: int = 1, out_features: int = 2, keep_prob: float = 0.8,
                 optimizer: str = "adam", learning_rate: float = 1e-3, decay_rate: float = 0.95,
                 decay_steps: int | None = None, lmax: float = 2, gates: str = "reference",
                 device=None, seed: int = 2017, comm=None, filter: str = "cheby_conv"):
        # fc_layer (lib/gconv_lstm.py:629-636) uses the same filter by name
        H, Fout = int(num_hidden), int(out_features)
        fc_shape = (int(L.shape[0]), Fout, H) if filter == "fourier_conv" else (int(K) * H, Fout)
        super().__init__(L, N, T, feat_in, num_hidden, K, layer_count, out_features, keep_prob, filter,
                         math.prod(fc_shape), optimizer, learning_rate, decay_rate, decay_steps, lmax,
                         gates, device, seed, comm)
        w0 = truncated_normal_(torch.empty(fc_shape, device=self.device, dtype=torch.float32), 0.1,
                               self._gen)
        self.W_fc = self.carve(fc_shape, "conv_init/weights", init=w0)[0]
        self._carved()
        self._out = None

    def forward(self, x, dropout: bool = True, stream=None):
        """inference_glstm: the fc layer's output [N, M, out_features] (lstm_to_hT,
        the last-step mask through ops.dropout, fc_layer).  ``dropout=False``
        runs every layer unwrapped.  Every launch goes to torch's current stream;
        ``stream`` is train_step's and must be that stream.  ``backward`` continues
        from the output this call keeps."""
        h, mask = lstm_to_hT(self.cells, self.wrapped, self._steps(x), dropout)
        if mask is not None:
            keep, seed, off = mask
            h = ops.dropout(h, keep, seed, offset=off)
        self._out = ops.fourier_conv(h, self.W_fc, self.U) if self.filter == "fourier_conv" \
            else ops.cheb_conv(h, self.W_fc, self.plan, self.K)
        return self._out

    def backward(self, dout, stream=None):
        """Every gradient of the last forward from d(out): autograd, accumulating
        into the (zeroed) bucket."""
        self.grad.zero_()
        out, self._out = self._out, None
        out.backward(dout)
