"""PyTorch-facing ops over the HIP kernels (device memory, streams, autograd).

PyTorch is plumbing here: every op hands raw device pointers and the current
HIP stream to libcheb_mi355.so.  There is no CPU/eager fallback: a CPU tensor
or a missing library raises.

  cheb_forward / cheb_backward  -- lib/graph_conv.py:144-176 and its TF autodiff
  ChebConv (autograd.Function)  -- what chebyshev5 / cheby_conv call
  bias_act                      -- b1relu / b1tanh / b2relu, lib/graph_conv.py:178-199
  matmul                        -- tf.matmul of fc, lib/graph_conv.py:220-226 (MFMA GEMM)
  fourier_conv                  -- filter_in_fourier, lib/graph_conv.py:83-111
  fourier_conv_act              -- the same filter inside the residual block (:234-262):
                                   residual add and ReLU in the synthesis' store
  mpool1, apool1                -- lib/graph_conv.py:201-218
  perm_data                     -- lib/coarsening.py:219-240 (device gather)
  batch_gather                  -- lib/graph_model.py:149 (a batch out of a dataset on the device)
  adam_update                   -- lib/graph_model.py:293-298
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .plan import ChebPlan


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _plan_ws(plan: ChebPlan, nbytes: int, t: torch.Tensor):
    """(workspace tensor, stream) for a call on t's current stream: the plan's
    cached per-stream buffer (no allocation per autograd call)."""
    s = _stream(t)
    return plan.workspace(nbytes, t.device, s), s


def _check_dev(name, t: torch.Tensor, dtype=torch.float32):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a HIP (cuda) tensor, got {t.device}; "
                         "cnn_graph_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _p(t):
    return None if t is None else t.data_ptr()


def _check_out(name, t, shape):
    """A caller-supplied output: fp32, on the GPU, contiguous, with prod(shape) elements."""
    _check_dev(name, t)
    n = 1
    for s in shape:
        n *= int(s)
    if not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{name}: need a contiguous tensor of {tuple(shape)} elements, "
                         f"got {tuple(t.shape)}")


def _ws_bytes(entry, *args, sizes=1):
    """The ``sizes`` byte counts a cg_*_workspace_bytes entry reports for ``args``."""
    out = [ctypes.c_size_t() for _ in range(sizes)]
    _lib.call(entry, *args, *(ctypes.byref(o) for o in out))
    return [o.value for o in out]


def _workspace(entry, *args, device, sizes=1, pick=0):
    """(uint8 tensor, nbytes): a fresh workspace of the size ``entry`` reports
    (number ``pick`` of its ``sizes``), at least 1 byte.  Not cached: only the
    plan's per-stream buffer (_plan_ws) is.  Shared package-wide: trainer.py and
    gconv_rnn.py size their preallocated workspaces with it."""
    nbytes = _ws_bytes(entry, *args, sizes=sizes)[pick]
    return torch.empty(max(nbytes, 1), device=device, dtype=torch.uint8), nbytes


def _out(name, given, shape, device, elems=None, accumulate=False):
    """The caller's output tensor or a fresh fp32 one of ``shape``, checked by
    _check_out against ``elems`` (default: shape).  accumulate: there must be a
    given tensor to add into."""
    if given is None:
        if accumulate:
            raise ValueError("accumulate=True needs an out tensor")
        given = torch.empty(tuple(shape), device=device, dtype=torch.float32)
    _check_out(name, given, elems if elems is not None else shape)
    return given


def _check_opt(name, t, n: int, aligned: bool):
    """An optional input: None, or fp32 on the GPU, contiguous, n elements and --
    where the kernel reads it as float4 -- 16-byte aligned."""
    if t is None:
        return
    _check_dev(name, t)
    if not t.is_contiguous() or t.numel() != n or (aligned and t.data_ptr() % 16):
        raise ValueError(f"{name}: need a contiguous{' 16-byte aligned' if aligned else ''} tensor "
                         f"of {n} floats, got {tuple(t.shape)}")


def _check_planes(name, t, n: int, stride: int, per: int, aligned: bool):
    """``t``'s storage holds n planes of ``per`` floats, ``stride`` floats apart,
    from t's first element on; aligned: the kernel moves them as float4."""
    avail = t.untyped_storage().nbytes() // 4 - t.storage_offset()
    if n > 0 and (stride < per or avail < (n - 1) * stride + per):
        raise ValueError(f"{name}: storage too small for {n} planes of {per} floats at this stride")
    if aligned and (t.data_ptr() % 16 or (n > 0 and stride % 4)):
        raise ValueError(f"{name}: needs a 16-byte aligned start and a stride that is a "
                         "multiple of 4 floats (the kernel moves float4)")


def _check_weight(name, W, rows: int, cols: int):
    if tuple(W.shape) != (rows, cols) or not W.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [{rows}, {cols}] tensor")


def _supported(entry, *args) -> bool:
    ok = ctypes.c_int32()
    _lib.call(entry, *args, ctypes.byref(ok))
    return bool(ok.value)


ACTS = _lib.enum_names("CG_ACT_")


def act_forward_(y: torch.Tensor, residual: torch.Tensor | None = None, act: str = "none"):
    """y <- act(y + residual) in place: the epilogue of the Chebyshev forward as
    its own launch (what the routes without a fused store finish through)."""
    _check_dev("y", y)
    if not y.is_contiguous():
        raise ValueError("y must be contiguous (it is written in place)")
    if residual is not None:
        _check_dev("residual", residual)
        residual = residual.contiguous()
        if residual.numel() != y.numel():
            raise ValueError("residual must have y's size")
    _lib.call("cg_act_forward", y.numel(), _p(y), _p(residual), ACTS[act], _stream(y))
    return y


def basis_layout_for(plan: ChebPlan, N: int, Fin: int, K: int, Fout: int) -> str:
    """The layout a caller that keeps the basis to itself (the autograd
    functions below) should use: 'planes' where it applies (sample-major
    streaming path, Fin % 16 == 0: no basis-assembly pass), else 'rows'."""
    return "planes" if plan.basis_elems(N, Fin, K, Fout, "planes") else "rows"


def cheb_forward(plan: ChebPlan, x: torch.Tensor, W: torch.Tensor | None, K: int,
                 want_basis: bool = True, out_basis: torch.Tensor | None = None,
                 out_y: torch.Tensor | None = None, residual: torch.Tensor | None = None,
                 act: str = "none", layout: str = "rows"):
    """Basis (N*M, Fin*K) and y = act(basis @ W + residual) (N, M, Fout).
    W None -> basis only.  out_basis / out_y: pre-allocated contiguous outputs.
    layout: the basis layout ('rows' = lib/graph_conv.py:172; 'planes' =
    [K, N*M, Fin], see ChebRunner); pass the same one to the backward."""
    _check_dev("x", x)
    x = x.contiguous()
    N, M, Fin = x.shape
    if M != plan.M:
        raise ValueError(f"x has M={M} vertices but the Laplacian has {plan.M}")
    if W is not None:
        _check_dev("W", W)
        W = W.contiguous()
        if W.shape[0] != Fin * K:
            raise ValueError(f"W must be [Fin*K, Fout] = [{Fin * K}, *], got {tuple(W.shape)}")
        Fout = int(W.shape[1])
    else:
        Fout = 1
    dev = x.device
    # the streaming path's GEMM reads the basis from HBM, so it always needs one
    need_basis = want_basis or W is None or plan.query_path(N, Fin, K, Fout) == "stream"
    basis = y = None
    if need_basis:
        shape = (K, N * M, Fin) if layout == "planes" else (N * M, Fin * K)
        basis = _out("out_basis", out_basis, shape, dev, elems=(N * M, Fin * K))
    if W is not None:
        y = _out("out_y", out_y, (N, M, Fout), dev, elems=(N * M * Fout,))
    if residual is not None:
        _check_dev("residual", residual)
        residual = residual.contiguous()
        if W is None or residual.numel() != N * M * Fout:
            raise ValueError(f"residual must be [N, M, Fout] = [{N}, {M}, {Fout}]")
    fwd_ws, _ = plan.workspace_bytes(N, Fin, K, Fout)
    ws, s = _plan_ws(plan, fwd_ws, x)
    _lib.call("cg_cheb_forward_layout", plan.handle, N, Fin, K, Fout, _p(x), _p(W), _p(residual),
              ACTS[act], _lib.BASIS_LAYOUTS[layout], _p(basis), _p(y), _p(ws), fwd_ws, s)
    return basis, y


def _cheb_backward(plan, dy, y, act, basis, W, K, dx, dx_accumulate, need_dx, need_dW, layout,
                   want_dz):
    """The body of cheb_backward (y None, act 'none', no dz: the C side then
    makes no copy of dy) and cheb_backward_ex: (dx, dW, dz)."""
    _check_dev("dy", dy)
    dy = dy.contiguous()
    N, M, Fout = dy.shape
    FinK = int(W.shape[0])
    Fin = FinK // K
    dev = dy.device
    if dx is not None:
        _check_out("dx", dx, (N, M, Fin))
    elif need_dx:
        if dx_accumulate:
            raise ValueError("dx_accumulate needs a dx tensor")
        dx = torch.empty((N, M, Fin), device=dev, dtype=torch.float32)
    dW = torch.empty((FinK, Fout), device=dev, dtype=torch.float32) if need_dW else None
    dz = torch.empty((N, M, Fout), device=dev, dtype=torch.float32) if want_dz else None
    _, bwd_ws = plan.workspace_bytes(N, Fin, K, Fout)
    ws, s = _plan_ws(plan, bwd_ws, dy)
    _lib.call("cg_cheb_backward_layout", plan.handle, N, Fin, K, Fout, _p(dy), _p(y), ACTS[act],
              _lib.BASIS_LAYOUTS[layout], _p(basis), _p(W.contiguous()),
              _p(dx if need_dx else None), int(dx_accumulate), _p(dW), _p(dz), _p(ws), bwd_ws, s)
    return (dx if need_dx else None), dW, dz


def cheb_backward(plan: ChebPlan, dy: torch.Tensor, basis: torch.Tensor, W: torch.Tensor, K: int,
                  need_dx: bool = True, need_dW: bool = True, layout: str = "rows"):
    """(dx [N,M,Fin] or None, dW [Fin*K, Fout] or None); layout: the forward's."""
    return _cheb_backward(plan, dy, None, "none", basis, W, K, None, False, need_dx, need_dW,
                          layout, want_dz=False)[:2]


def cheb_backward_ex(plan: ChebPlan, dy: torch.Tensor, y: torch.Tensor | None, act: str,
                     basis: torch.Tensor, W: torch.Tensor, K: int, dx: torch.Tensor | None = None,
                     dx_accumulate: bool = False, need_dx: bool = True, need_dW: bool = True,
                     layout: str = "rows"):
    """Backward through y = act(basis W + residual): returns (dx, dW, dz) where
    dz = dy * act'(y) is also the gradient of the residual input.  With
    dx_accumulate the input gradient is added into the given ``dx``."""
    return _cheb_backward(plan, dy, y, act, basis, W, K, dx, dx_accumulate, need_dx, need_dW,
                          layout, want_dz=True)


def mse_loss(pred: torch.Tensor, labels: torch.Tensor, need_grad: bool = True):
    """lib/graph_model.py:255 mean((labels - pred)^2) on device: (loss [1], dpred or None)."""
    _check_dev("pred", pred)
    _check_dev("labels", labels)
    pred, labels = pred.contiguous(), labels.contiguous()
    if pred.numel() != labels.numel():
        raise ValueError("pred and labels differ in size")
    n = pred.numel()
    ws, nb = _workspace("cg_mse_loss_workspace_bytes", n, device=pred.device)
    loss = torch.empty((1,), device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if need_grad else None
    _lib.call("cg_mse_loss", _p(pred), _p(labels), n, _p(loss), _p(dpred), _p(ws), nb, _stream(pred))
    return loss, dpred


class ChebRunner:
    """Pre-allocated forward/backward of one (plan, N, Fin, K, Fout) shape:
    every device buffer (basis, y, dx, dW, workspace) is allocated once, so a
    step is just the C-ABI launches on the current stream -- no allocator or
    Python-side shape work per call (and safe to capture in a HIP graph).
    The forward's workspace is dead once the forward has run, so the forward
    and the backward share ONE buffer of max(fwd, bwd) bytes (config D at
    N = 256: 51.5 GB instead of 68.7 GB)."""

    def __init__(self, plan: ChebPlan, N: int, Fin: int, K: int, Fout: int, device,
                 basis_layout: str = "rows"):
        """basis_layout: 'rows' ([N*M, Fin*K], lib/graph_conv.py:172), 'orders'
        ([N, Fin*K, Mb], one plane per order: the fast forward stores it during
        the recurrence; Fin <= 2 fast path with fused dW only) or 'planes'
        ([K, N*M, Fin], T_k in the layout of x: the streaming steps write their
        own plane and skip the basis assembly; sample-major streaming path with
        Fin % 16 == 0 only).  The basis is
        this runner's saved tensor either way.  On config B the orders layout
        makes the forward ~1.3 us faster and the backward ~1.9 us slower
        (profiles/r02_orders), so 'rows' stays the default."""
        self.plan, self.N, self.Fin, self.K, self.Fout = plan, int(N), int(Fin), int(K), int(Fout)
        dev = torch.device(device)
        self.path = plan.query_path(N, Fin, K, Fout)
        fb, bb = plan.workspace_bytes(N, Fin, K, Fout)
        M = plan.M
        f32 = dict(device=dev, dtype=torch.float32)
        if basis_layout == "orders":
            if plan.basis_elems(N, Fin, K, Fout, "orders") is None:
                raise ValueError("orders basis layout does not apply to this shape "
                                 "(needs the fast forward and the fused-dW fast backward)")
            self.basis = torch.empty((N, Fin * K, (M + 31) // 32 * 32), **f32)
        elif basis_layout == "planes":
            if plan.basis_elems(N, Fin, K, Fout, "planes") is None:
                raise ValueError("planes basis layout does not apply to this shape (needs the "
                                 "sample-major streaming path, Fin % 16 == 0, K >= 2)")
            self.basis = torch.empty((K, N * M, Fin), **f32)
        elif basis_layout == "rows":
            self.basis = torch.empty((N * M, Fin * K), **f32)
        else:
            raise ValueError(f"unknown basis layout {basis_layout!r}")
        self.basis_layout = basis_layout
        self._lay = _lib.BASIS_LAYOUTS[basis_layout]
        self.y = torch.empty((N, M, Fout), **f32)
        self.dx = torch.empty((N, M, Fin), **f32)
        self.dW = torch.empty((Fin * K, Fout), **f32)
        self.ws = torch.empty(max(fb, bb, 1), device=dev, dtype=torch.uint8)
        self.fws = self.bws = self.ws
        self.fwd_bytes, self.bwd_bytes = fb, bb
        self._fwd = _lib.lib().cg_cheb_forward_layout
        self._bwd = _lib.lib().cg_cheb_backward_layout

    def input_plane(self) -> torch.Tensor | None:
        """Planes layout: plane 0 of the saved basis as an [N, M, Fin] tensor.  A
        producer that writes the filter input there (and passes it as x) saves
        the forward's copy of x into plane 0 (cg_cheb_forward_layout reads
        T_0 in place when x == basis).  None for the other layouts."""
        if self.basis_layout != "planes":
            return None
        return self.basis[0].view(self.N, self.plan.M, self.Fin)

    def basis_rows(self) -> torch.Tensor:
        """The saved basis as [N*M, Fin*K] (a copy when the layout is 'orders')."""
        if self.basis_layout == "rows":
            return self.basis
        if self.basis_layout == "planes":  # [K][N*M][Fin] -> column fin*K + k
            return self.basis.permute(1, 2, 0).reshape(self.N * self.plan.M, self.Fin * self.K)
        M = self.plan.M
        return self.basis[:, :, :M].permute(0, 2, 1).reshape(self.N * M, self.Fin * self.K)

    def forward(self, x: torch.Tensor, W: torch.Tensor, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        st = self._fwd(self.plan.handle, self.N, self.Fin, self.K, self.Fout, x.data_ptr(),
                       W.data_ptr(), None, 0, self._lay, self.basis.data_ptr(), self.y.data_ptr(),
                       self.fws.data_ptr(), self.fwd_bytes, s)
        _lib.check("cg_cheb_forward_layout", st)
        return self.y

    def forward_adam(self, x: torch.Tensor, W: torch.Tensor, grad: torch.Tensor, m: torch.Tensor,
                     v: torch.Tensor, W_out: torch.Tensor, m_out: torch.Tensor,
                     v_out: torch.Tensor, step: int, lr: float = 1e-3, beta1: float = 0.9,
                     beta2: float = 0.999, eps: float = 1e-8, grad_scale: float = 1.0,
                     stream=None):
        """The exchange step's Adam on W applied by the forward that consumes it
        (cg_cheb_forward_adam): W_out, m_out, v_out = ApplyAdam(W, grad; m, v),
        then y = chebyshev5(x; W_out).  Outputs out of place (double-buffer them)."""
        shape = (self.Fin * self.K, self.Fout)
        for name, t_ in (("W", W), ("grad", grad), ("m", m), ("v", v), ("W_out", W_out),
                         ("m_out", m_out), ("v_out", v_out)):
            _check_out(name, t_, shape)
        s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        st = _lib.lib().cg_cheb_forward_adam(
            self.plan.handle, self.N, self.Fin, self.K, self.Fout, x.data_ptr(), W.data_ptr(),
            grad.data_ptr(), m.data_ptr(), v.data_ptr(), lr, beta1, beta2, eps, step, grad_scale,
            W_out.data_ptr(), m_out.data_ptr(), v_out.data_ptr(), self._lay,
            self.basis.data_ptr(), self.y.data_ptr(), self.fws.data_ptr(), self.fwd_bytes, s)
        _lib.check("cg_cheb_forward_adam", st)
        return self.y

    def backward(self, dy: torch.Tensor, W: torch.Tensor, need_dx: bool = True, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(dy.device).cuda_stream
        st = self._bwd(self.plan.handle, self.N, self.Fin, self.K, self.Fout, dy.data_ptr(), None, 0,
                       self._lay, self.basis.data_ptr(), W.data_ptr(),
                       self.dx.data_ptr() if need_dx else None, 0, self.dW.data_ptr(), None,
                       self.bws.data_ptr(), self.bwd_bytes, s)
        _lib.check("cg_cheb_backward_layout", st)
        return (self.dx if need_dx else None), self.dW

    def backward_adam(self, dy: torch.Tensor, W: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                      step: int, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999,
                      eps: float = 1e-8, grad_scale: float = 1.0, need_dx: bool = True,
                      stream=None):
        """backward + Adam on W in place, the update fused into the dW reduction
        (cg_cheb_backward_adam_layout; one-GPU step, lib/graph_model.py:277-298)."""
        shape = (self.Fin * self.K, self.Fout)
        for name, t_ in (("W", W), ("m", m), ("v", v)):
            _check_out(name, t_, shape)   # updated in place for i < Fin*K*Fout
        if len({W.data_ptr(), m.data_ptr(), v.data_ptr(), self.dW.data_ptr()}) != 4:
            raise ValueError("backward_adam: W, m, v and dW must be distinct buffers")
        s = stream if stream is not None else torch.cuda.current_stream(dy.device).cuda_stream
        st = _lib.lib().cg_cheb_backward_adam_layout(
            self.plan.handle, self.N, self.Fin, self.K, self.Fout, self._lay, dy.data_ptr(),
            self.basis.data_ptr(), W.data_ptr(), self.dx.data_ptr() if need_dx else None,
            self.dW.data_ptr(), m.data_ptr(), v.data_ptr(), lr, beta1, beta2, eps, step,
            grad_scale, self.bws.data_ptr(), self.bwd_bytes, s)
        _lib.check("cg_cheb_backward_adam_layout", st)
        return (self.dx if need_dx else None), self.dW


def _saved_basis_layout(plan: ChebPlan, basis: torch.Tensor, layout: str, N: int, Fin: int, K: int,
                        Fout: int):
    """The basis an autograd backward hands to the C ABI: the saved one, or --
    when the plan's path / variant was changed between forward and backward so
    that the planes layout no longer applies -- the same values re-laid as
    the rows layout of lib/graph_conv.py:172 (column fin*K + k)."""
    if layout != "planes" or plan.basis_elems(N, Fin, K, Fout, "planes"):
        return basis, layout
    return basis.permute(1, 2, 0).reshape(N * plan.M, Fin * K).contiguous(), "rows"


class ChebConv(torch.autograd.Function):
    """y = chebyshev5(x; L~, W, K) with the HIP forward/backward kernels."""

    @staticmethod
    def forward(ctx, x, W, plan: ChebPlan, K: int):
        # the saved basis is internal: the planes layout where it applies
        lay = basis_layout_for(plan, x.shape[0], x.shape[2], K, W.shape[1])
        basis, y = cheb_forward(plan, x, W, K, want_basis=True, layout=lay)
        ctx.save_for_backward(basis, W)
        ctx.plan, ctx.K, ctx.layout = plan, K, lay
        return y

    @staticmethod
    def backward(ctx, dy):
        basis, W = ctx.saved_tensors
        N, Fout = dy.shape[0], W.shape[1]
        basis, lay = _saved_basis_layout(ctx.plan, basis, ctx.layout, N, W.shape[0] // ctx.K, ctx.K,
                                         Fout)
        dx, dW = cheb_backward(ctx.plan, dy, basis, W, ctx.K, need_dx=ctx.needs_input_grad[0],
                               layout=lay)
        return dx, dW, None, None


class ChebConvAct(torch.autograd.Function):
    """y = act(chebyshev5(x; L~, W, K) + residual) in one kernel pass
    (lib/graph_conv.py:256-262); residual may be None."""

    @staticmethod
    def forward(ctx, x, W, residual, plan: ChebPlan, K: int, act: str):
        lay = basis_layout_for(plan, x.shape[0], x.shape[2], K, W.shape[1])
        basis, y = cheb_forward(plan, x, W, K, want_basis=True, residual=residual, act=act,
                                layout=lay)
        ctx.save_for_backward(basis, W, y)
        ctx.plan, ctx.K, ctx.act, ctx.has_res = plan, K, act, residual is not None
        ctx.layout = lay
        return y

    @staticmethod
    def backward(ctx, dy):
        basis, W, y = ctx.saved_tensors
        basis, lay = _saved_basis_layout(ctx.plan, basis, ctx.layout, dy.shape[0],
                                         W.shape[0] // ctx.K, ctx.K, W.shape[1])
        dx, dW, dz = cheb_backward_ex(ctx.plan, dy, y, ctx.act, basis, W, ctx.K,
                                      need_dx=ctx.needs_input_grad[0], layout=lay)
        return dx, dW, (dz if ctx.has_res else None), None, None, None


def cheb_conv(x, W, plan: ChebPlan, K: int, residual=None, act: str = "none"):
    if residual is None and act == "none":
        return ChebConv.apply(x, W, plan, K)
    return ChebConvAct.apply(x, W, residual, plan, K, act)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p: int):
        _check_dev("x", x)
        x = x.contiguous()
        N, M, F = x.shape
        y = torch.empty((N, M // p, F), device=x.device, dtype=torch.float32)
        arg = torch.empty((N, M // p, F), device=x.device, dtype=torch.int32)
        _lib.call("cg_maxpool_forward", _p(x), N, M, F, p, _p(y), _p(arg), _stream(x))
        ctx.save_for_backward(arg)
        ctx.shape, ctx.p = (N, M, F), p
        ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, dy, _darg):
        (arg,) = ctx.saved_tensors
        N, M, F = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty((N, M, F), device=dy.device, dtype=torch.float32)
        _lib.call("cg_maxpool_backward", _p(dy), _p(arg), N, M, F, ctx.p, _p(dx), _stream(dy))
        return dx, None


def mpool1_with_argmax(x, p: int):
    """(y, argmax) -- argmax is the absolute vertex of the first maximum."""
    return _MaxPool.apply(x, p)


def mpool1(x, p: int):
    """Max pooling of size p along vertices (lib/graph_conv.py:201-209)."""
    if p <= 1:
        return x
    return _MaxPool.apply(x, p)[0]


class _AvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p: int):
        _check_dev("x", x)
        x = x.contiguous()
        N, M, F = x.shape
        y = torch.empty((N, M // p, F), device=x.device, dtype=torch.float32)
        _lib.call("cg_avgpool_forward", _p(x), N, M, F, p, _p(y), _stream(x))
        ctx.shape, ctx.p = (N, M, F), p
        return y

    @staticmethod
    def backward(ctx, dy):
        N, M, F = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty((N, M, F), device=dy.device, dtype=torch.float32)
        _lib.call("cg_avgpool_backward", _p(dy), N, M, F, ctx.p, _p(dx), _stream(dy))
        return dx, None


def apool1(x, p: int):
    """Average pooling of size p along vertices (lib/graph_conv.py:211-218)."""
    if p <= 1:
        return x
    return _AvgPool.apply(x, p)


def perm_data(x: torch.Tensor, perm) -> torch.Tensor:
    """Device perm_data (lib/coarsening.py:219-240): x [N, M] or [N, M, F] ->
    [N, len(perm)(, F)] with fake vertices (perm[i] >= M) set to 0."""
    _check_dev("x", x)
    squeeze = x.dim() == 2
    x3 = (x.unsqueeze(-1) if squeeze else x).contiguous()
    N, M, F = x3.shape
    perm_t = torch.as_tensor(perm, dtype=torch.int32, device=x.device).contiguous()
    Mo = int(perm_t.numel())
    out = torch.empty((N, Mo, F), device=x.device, dtype=torch.float32)
    _lib.call("cg_perm_gather", _p(x3), _p(perm_t), N, M, Mo, F, _p(out), _stream(x))
    return out[..., 0] if squeeze else out


def batch_gather(data: torch.Tensor, labels: torch.Tensor | None, idx: torch.Tensor, N: int,
                 out_x: torch.Tensor | None = None, out_y: torch.Tensor | None = None):
    """One training batch out of a dataset on the device (cg_batch_gather; the
    ``train_data[idx, :], train_labels[idx]`` of lib/graph_model.py:149): ``x[n] =
    data[idx[n]]``, ``y[n] = labels[idx[n]]`` for n < N in ONE launch, a zero row
    where ``idx[n]`` is outside [0, S).  data [S, ...] and labels [S, ...] (or
    None) are contiguous fp32; ``idx`` is an int32 cuda tensor whose first N
    entries are read.  Returns ``(x, y)`` (``y`` None without labels).  No
    autograd: the inputs are data."""
    _check_dev("data", data)
    _check_dev("idx", idx, torch.int32)
    N, S = int(N), int(data.shape[0]) if data.dim() else 0
    if N < 1 or S < 1 or not data.is_contiguous():
        raise ValueError("batch_gather: data must be a contiguous [S, ...] tensor, S >= 1 and N >= 1")
    if idx.dim() != 1 or not idx.is_contiguous() or idx.numel() < N:
        raise ValueError(f"batch_gather: idx must be a contiguous 1-D tensor of at least N = {N} entries")
    row = data.numel() // S
    x = _out("out_x", out_x, (N,) + tuple(data.shape[1:]), data.device)
    y, lrow = None, 0
    if labels is not None:
        _check_dev("labels", labels)
        if labels.dim() < 1 or int(labels.shape[0]) != S or not labels.is_contiguous():
            raise ValueError(f"batch_gather: labels must be a contiguous [S = {S}, ...] tensor")
        lrow = labels.numel() // S
        y = _out("out_y", out_y, (N,) + tuple(labels.shape[1:]), data.device)
    elif out_y is not None:
        raise ValueError("batch_gather: out_y without labels")
    _lib.call("cg_batch_gather", _p(data), _p(labels), _p(idx), N, S, row, lrow, _p(x), _p(y),
              _stream(data))
    return x, y


def weight_grad(basis: torch.Tensor, dy: torch.Tensor, out: torch.Tensor | None = None,
                accumulate: bool = False) -> torch.Tensor:
    """dW = basis^T dy over all rows (basis [R, FinK], dy [R, Fout] in any
    [..., Fout] shape); accumulate=True adds into ``out``."""
    _check_dev("basis", basis)
    _check_dev("dy", dy)
    FinK = int(basis.shape[-1])
    R = basis.numel() // FinK
    Fout = int(dy.shape[-1])
    if dy.numel() != R * Fout:
        raise ValueError(f"dy has {dy.numel()} elements, expected R*Fout = {R * Fout}")
    out = _out("out", out, (FinK, Fout), basis.device, accumulate=accumulate)
    ws, nb = _workspace("cg_weight_grad_workspace_bytes", R, FinK, Fout, device=basis.device)
    _lib.call("cg_weight_grad", R, FinK, Fout, _p(basis.contiguous()), _p(dy.contiguous()), _p(out),
              int(accumulate), _p(ws), nb, _stream(basis))
    return out


def weight_grad_planes(planes: torch.Tensor, plane_stride: int, K: int, R: int, dy: torch.Tensor,
                       out: torch.Tensor | None = None, accumulate: bool = False) -> torch.Tensor:
    """dW [Fin*K, Fout] (row fin*K + k) = sum_k planes_k^T dy over R rows, the K
    planes [R, Fin] of ``planes``' storage plane_stride floats apart (plane k
    at planes.data_ptr() + k*plane_stride floats); one pass over dy."""
    _check_dev("planes", planes)
    _check_dev("dy", dy)
    Fin = int(planes.shape[-1])
    Fout = int(dy.shape[-1])
    if dy.numel() != R * Fout or not dy.is_contiguous():
        raise ValueError(f"dy must be a contiguous tensor of R*Fout = {R * Fout} elements")
    _check_planes("planes", planes, K, plane_stride, R * Fin, aligned=False)
    out = _out("out", out, (Fin * K, Fout), planes.device, accumulate=accumulate)
    ws, nb = _workspace("cg_weight_grad_workspace_bytes", R, Fin * K, Fout, device=planes.device)
    _lib.call("cg_weight_grad_planes", int(R), Fin, int(K), Fout, _p(planes), int(plane_stride),
              _p(dy), _p(out), int(accumulate), _p(ws), nb, _stream(planes))
    return out


def lstm_weight_grads(h_planes: torch.Tensor, h_plane_stride: int, x_planes: torch.Tensor,
                      x_plane_stride: int, K: int, R: int, dpre: torch.Tensor):
    """dWh [H*K, 4H], dWx [Fin*K, 4H] and db [4H] of a gconv-LSTM layer in ONE
    pass over dpre [R, 4H] (cg_lstm_weight_grads): the K h planes [R, H] of
    h_planes' storage h_plane_stride floats apart, the K x planes [R, Fin] of
    x_planes' storage likewise."""
    for name, t in (("h_planes", h_planes), ("x_planes", x_planes), ("dpre", dpre)):
        _check_dev(name, t)
    H, Fin = int(h_planes.shape[-1]), int(x_planes.shape[-1])
    if dpre.numel() != R * 4 * H or not dpre.is_contiguous():
        raise ValueError(f"dpre must be a contiguous tensor of R*4H = {R * 4 * H} elements")
    _check_planes("h_planes", h_planes, K, h_plane_stride, R * H, aligned=False)
    _check_planes("x_planes", x_planes, K, x_plane_stride, R * Fin, aligned=False)
    f32 = dict(device=dpre.device, dtype=torch.float32)
    dWh = torch.empty((H * K, 4 * H), **f32)
    dWx = torch.empty((Fin * K, 4 * H), **f32)
    db = torch.empty((4 * H,), **f32)
    ws, nb = _workspace("cg_lstm_weight_grads_workspace_bytes", int(R), H, Fin, int(K),
                        device=dpre.device)
    _lib.call("cg_lstm_weight_grads", int(R), H, Fin, int(K), _p(h_planes), int(h_plane_stride),
              _p(x_planes), int(x_plane_stride), _p(dpre), _p(dWh), _p(dWx), _p(db), _p(ws),
              nb, _stream(dpre))
    return dWh, dWx, db


def bias_grad(dy: torch.Tensor, out: torch.Tensor | None = None, accumulate: bool = False):
    """db = dy summed over every axis but the last (gradient of a broadcast bias)."""
    _check_dev("dy", dy)
    C = int(dy.shape[-1])
    R = dy.numel() // C
    out = _out("out", out, (C,), dy.device, accumulate=accumulate)
    ws, nb = _workspace("cg_bias_grad_workspace_bytes", R, C, device=dy.device)
    _lib.call("cg_bias_grad", R, C, _p(dy.contiguous()), _p(out), int(accumulate), _p(ws), nb,
              _stream(dy))
    return out


LSTM_GATES = _lib.enum_names("CG_LSTM_GATES_")


def _cell_outs(out_c, out_h, out_act, lead, R: int, H: int, dev):
    """(c', h', act) of one cell step: the caller's or fresh [*lead, H] / [*lead, 4H]."""
    return (_out("c_out", out_c, lead + (H,), dev, elems=(R, H)),
            _out("h_out", out_h, lead + (H,), dev, elems=(R, H)),
            _out("act", out_act, lead + (4 * H,), dev, elems=(R, 4 * H)))


def lstm_cell_forward(gx, gh, bias, c, H: int, gates="reference", out_c=None, out_h=None,
                      out_act=None):
    """Pointwise part of GConvLSTMCell (lib/gconv_lstm.py:183-221): gx, gh
    [..., 4H] gate pre-activations of the x- and h-conv (gh None = 0), bias
    [4H] (None = 0), c [..., H] (None = 0).  Returns (c', h', act [..., 4H])."""
    _check_dev("gx", gx)
    R = gx.numel() // (4 * H)
    lead = tuple(gx.shape[:-1])
    dev = gx.device
    for name, t, n in (("gh", gh, R * 4 * H), ("bias", bias, 4 * H), ("c", c, R * H)):
        _check_opt(name, t, n, aligned=False)
    c_out, h_out, act = _cell_outs(out_c, out_h, out_act, lead, R, H, dev)
    _lib.call("cg_lstm_cell_forward", R, H, LSTM_GATES[gates], _p(gx.contiguous()), _p(gh), _p(bias),
              _p(c), _p(c_out), _p(h_out), _p(act), _stream(gx))
    return c_out, h_out, act


def lstm_hconv_supported(plan: ChebPlan, H: int, K: int) -> bool:
    """Whether cg_lstm_hconv_step serves this graph / hidden size / order."""
    return _supported("cg_lstm_hconv_supported", plan.handle, int(H), int(K))


def lstm_hconv_step(plan: ChebPlan, h_prev, c_prev, gx, Wh, bias, K: int, gates="reference",
                    out_c=None, out_h=None, out_act=None, planes=None, plane_stride: int = 0):
    """One time step of GConvLSTMCell's h path in one launch (cg_lstm_hconv_step):
    the Chebyshev basis of h_prev, gh = basis Wh on MFMA and the gate update,
    given the step's x-conv gx [..., 4H].  planes (optional, a tensor whose
    storage holds K-1 planes [N, M, H] plane_stride floats apart) receives
    T_1 .. T_{K-1} of h_prev.  Returns (c', h', act)."""
    _check_dev("h_prev", h_prev)
    h_prev = h_prev.contiguous()
    N, M, H = (int(v) for v in h_prev.shape)
    R = N * M
    dev = h_prev.device
    for name, t, n in (("gx", gx, R * 4 * H), ("c_prev", c_prev, R * H), ("bias", bias, 4 * H)):
        _check_opt(name, t, n, aligned=False)
    _check_weight("Wh", Wh, K * H, 4 * H)
    c_out, h_out, act = _cell_outs(out_c, out_h, out_act, (N, M), R, H, dev)
    if planes is not None:
        _check_dev("planes", planes)
        _check_planes("planes", planes, K - 1, plane_stride, R * H, aligned=True)
    if h_prev.data_ptr() % 16:
        h_prev = h_prev.clone()  # float4 loads: a view at an odd offset is copied
    _lib.call("cg_lstm_hconv_step", plan.handle, N, H, int(K), LSTM_GATES[gates], _p(h_prev),
              _p(c_prev), _p(gx), _p(Wh), _p(bias), _p(c_out), _p(h_out), _p(act), _p(planes),
              int(plane_stride), _stream(h_prev))
    return c_out, h_out, act


def lstm_cell_backward(dh, dh_rec, dc, act, c, c_out, H: int, gates="reference", out_dpre=None,
                       need_dc_prev=True):
    """Backward of lstm_cell_forward: (dpre [..., 4H], dc_prev [..., H] or None)."""
    _check_dev("act", act)
    _check_dev("c_out", c_out)
    R = act.numel() // (4 * H)
    dev = act.device
    for name, t in (("dh", dh), ("dh_rec", dh_rec), ("dc", dc), ("c", c)):
        _check_opt(name, t, R * H, aligned=False)
    dpre = _out("dpre", out_dpre, act.shape, dev, elems=(R, 4 * H))
    dc_prev = torch.empty(tuple(c_out.shape), device=dev, dtype=torch.float32) if need_dc_prev else None
    _lib.call("cg_lstm_cell_backward", R, H, LSTM_GATES[gates], _p(dh), _p(dh_rec), _p(dc), _p(act),
              _p(c), _p(c_out), _p(dpre), _p(dc_prev), _stream(act))
    return dpre, dc_prev


def lstm_seq_supported(plan: ChebPlan, H: int, K: int) -> bool:
    """Whether the one-launch layer forward (cg_lstm_seq_forward) and the
    one-launch BPTT step (cg_lstm_bwd_step) serve this graph / H / K."""
    return _supported("cg_lstm_seq_supported", plan.handle, int(H), int(K))


def lstm_seq_fault(plan: ChebPlan, wait: bool = True) -> bool | None:
    """The plan's sticky sequence-launch fault word (cg_lstm_seq_fault): raises
    CGError (and resets the word) if a pair hand-off of any k_lstm_seq launch
    so far timed out -- that launch's hs / cs / act then hold NaN from the lost
    step on.  wait=True blocks until the last launch has completed and returns
    False; wait=False never blocks and returns None while it is in flight."""
    f = ctypes.c_int32()
    _lib.call("cg_lstm_seq_fault", plan.handle, int(bool(wait)), 1, ctypes.byref(f))
    return None if f.value < 0 else False


def _lstm_seq_prepare(plan: ChebPlan, dev, T: int, N: int, M: int, H: int, K: int, bias, h0, c0,
                      out_hs, out_cs, out_act, planes, plane_stride: int):
    """What lstm_seq_forward and lstm_seq_forward_x share: the bias / state
    checks, the hs / cs outputs (allocated unless given), the act check, the
    K-1 h planes (allocated unless given) and the launch's workspace.
    Returns (hs, cs, planes, plane_stride, workspace)."""
    R = T * N * M
    for name, t, n in (("bias", bias, 4 * H), ("h0", h0, N * M * H), ("c0", c0, N * M * H)):
        _check_opt(name, t, n, aligned=True)
    hs = _out("hs", out_hs, (T, N, M, H), dev, elems=(R, H))
    cs = _out("cs", out_cs, (T, N, M, H), dev, elems=(R, H))
    if out_act is not None:
        _check_out("act", out_act, (R, 4 * H))
    if planes is None and K > 1:  # the kernel hands Chebyshev orders through them
        planes = torch.empty((K - 1, R, H), device=dev, dtype=torch.float32)
        plane_stride = R * H
    if planes is not None:
        _check_dev("planes", planes)
        if K > 1:  # (K = 1: no plane is written; the C entry judges the pointer)
            _check_planes("planes", planes, K - 1, plane_stride, R * H, aligned=True)
    ws, _ = _workspace("cg_lstm_seq_workspace_bytes", plan.handle, int(N), device=dev)
    return hs, cs, planes, plane_stride, ws


def lstm_seq_forward(plan: ChebPlan, gx, Wh, bias, K: int, T: int, N: int, gates="reference",
                     h0=None, c0=None, out_hs=None, out_cs=None, out_act=None, planes=None,
                     plane_stride: int = 0, check: bool = False):
    """All T steps of a gconv-LSTM layer in ONE launch (cg_lstm_seq_forward):
    gx [T, N, M, 4H] (the x-conv of every step), h0 / c0 [N, M, H] or None
    (zero state).  planes (optional; a tensor whose storage holds K-1 planes
    [T, N, M, H] plane_stride floats apart) receives T_k of h_{t-1}, k >= 1.
    check=True waits for the launch and raises CGError if a pair hand-off timed
    out (lstm_seq_fault); without it the fault surfaces at the next check.
    Returns (hs [T, N, M, H], cs [T, N, M, H], act or None) -- act UNIT-major,
    [T, N, M, 4H] holding act[..., 4u + g] (g = z, i, f, o): lstm_bwd_step
    reads it with act_unit_major=True."""
    _check_dev("gx", gx)
    H = int(Wh.shape[1]) // 4
    M = plan.M
    R = T * N * M
    if not gx.is_contiguous() or gx.numel() != R * 4 * H:
        raise ValueError(f"gx must be a contiguous [{T}, {N}, {M}, {4 * H}] tensor")
    _check_weight("Wh", Wh, K * H, 4 * H)
    hs, cs, planes, plane_stride, ws = _lstm_seq_prepare(plan, gx.device, T, N, M, H, K, bias, h0,
                                                         c0, out_hs, out_cs, out_act, planes,
                                                         plane_stride)
    s = _stream(gx)
    _lib.call("cg_lstm_seq_forward", plan.handle, int(T), int(N), int(H), int(K), LSTM_GATES[gates],
              _p(gx), _p(Wh), _p(bias), _p(h0), _p(c0), _p(hs), _p(cs), _p(out_act), _p(planes),
              int(plane_stride), _p(ws), ws.numel(), s)
    if check:
        lstm_seq_fault(plan, wait=True)
    return hs, cs, out_act


def lstm_seq_x_supported(plan: ChebPlan, Fin: int, H: int, K: int) -> bool:
    """Whether cg_lstm_seq_forward_x (the x-conv fused in) serves feat_in = Fin."""
    return _supported("cg_lstm_seq_x_supported", plan.handle, int(Fin), int(H), int(K))


def lstm_seq_forward_x(plan: ChebPlan, xs, Wx, Wh, bias, K: int, gates="reference", h0=None,
                       c0=None, out_hs=None, out_cs=None, out_act=None, planes=None,
                       plane_stride: int = 0, xplanes=None, check: bool = False):
    """lstm_seq_forward with the x-conv fused in (cg_lstm_seq_forward_x; feat_in
    <= 8): xs [T, N, M, F] instead of gx.  xplanes (optional, [K, T, N*M, F]):
    receives the x basis T_k(x_t), k = 0..K-1.  Returns (hs, cs, act, xplanes)."""
    _check_dev("xs", xs)
    xs = xs.contiguous()
    T, N, M, F = (int(v) for v in xs.shape)
    H = int(Wh.shape[1]) // 4
    R = T * N * M
    dev = xs.device
    _check_weight("Wx", Wx, K * F, 4 * H)
    _check_weight("Wh", Wh, K * H, 4 * H)
    hs, cs, planes, plane_stride, ws = _lstm_seq_prepare(plan, dev, T, N, M, H, K, bias, h0, c0,
                                                         out_hs, out_cs, out_act, planes,
                                                         plane_stride)
    xplanes = _out("xplanes", xplanes, (K, R, F), dev, elems=(K * R * F,))
    s = _stream(xs)
    _lib.call("cg_lstm_seq_forward_x", plan.handle, T, N, F, int(H), int(K), LSTM_GATES[gates],
              _p(xs), _p(Wx), _p(xplanes), R * F, _p(Wh), _p(bias), _p(h0), _p(c0), _p(hs), _p(cs),
              _p(out_act), _p(planes), int(plane_stride), _p(ws), ws.numel(), s)
    if check:
        lstm_seq_fault(plan, wait=True)
    return hs, cs, out_act, xplanes


def lstm_bwd_step(plan: ChebPlan, dh, dh_rec, dc, act, c_prev, c_out, Wh, K: int,
                  gates="reference", out_dpre=None, need_dc_prev=True, out_dh_prev=None,
                  act_unit_major=False, need_dh_prev=True):
    """One BPTT step of a gconv-LSTM layer in ONE launch (cg_lstm_bwd_step):
    dpre = the gradient of the gate pre-activations, dc_prev, and dh_prev =
    the h-conv's input gradient.  dh / dh_rec / dc / c_prev may be None (= 0).
    act: gate-major [..., 4H] (lstm_cell_forward / lstm_hconv_step) or, with
    act_unit_major, the unit-major [..., H, 4] records of lstm_seq_forward*.
    need_dh_prev=False: the step ran no h-conv (step 0 of a zero-state layer):
    the pointwise backward only, dh_prev None.
    Returns (dpre [..., 4H], dc_prev [..., H] or None, dh_prev [..., H] or None)."""
    _check_dev("act", act)
    _check_dev("c_out", c_out)
    H = int(Wh.shape[1]) // 4
    R = act.numel() // (4 * H)
    N = R // plan.M
    dev = act.device
    for name, t in (("dh", dh), ("dh_rec", dh_rec), ("dc", dc), ("c_prev", c_prev),
                    ("c_out", c_out)):
        _check_opt(name, t, R * H, aligned=True)
    if not act.is_contiguous() or act.data_ptr() % 16:
        raise ValueError("act: need a contiguous 16-byte aligned tensor")
    _check_weight("Wh", Wh, K * H, 4 * H)
    dpre = _out("dpre", out_dpre, tuple(c_out.shape[:-1]) + (4 * H,), dev, elems=(R, 4 * H))
    dc_prev = torch.empty(tuple(c_out.shape), device=dev, dtype=torch.float32) if need_dc_prev else None
    dh_prev = _out("dh_prev", out_dh_prev, c_out.shape, dev, elems=(R, H)) if need_dh_prev else None
    _lib.call("cg_lstm_bwd_step", plan.handle, int(N), int(H), int(K), LSTM_GATES[gates], _p(dh),
              _p(dh_rec), _p(dc), _p(act), int(bool(act_unit_major)), _p(c_prev), _p(c_out), _p(Wh),
              _p(dpre), _p(dc_prev),
              _p(dh_prev), _stream(act))
    return dpre, dc_prev, dh_prev


class _Dropout(torch.autograd.Function):
    """tf.nn.dropout (TF 1.x) as DropoutWrapper applies it to a cell's outputs
    (lib/gconv_lstm.py:616, :623): cg_dropout_forward / cg_dropout_backward,
    the mask regenerated from ``seed`` in the backward."""

    @staticmethod
    def forward(ctx, x, keep_prob: float, seed: int):
        _check_dev("x", x)
        x = x.contiguous()
        y = torch.empty_like(x)
        _lib.call("cg_dropout_forward", _p(x), x.numel(), float(keep_prob), int(seed), _p(y), _stream(x))
        ctx.keep, ctx.seed = float(keep_prob), int(seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        _lib.call("cg_dropout_backward", _p(dy), dy.numel(), ctx.keep, ctx.seed, _p(dx), _stream(dy))
        return dx, None, None


DROP_WEYL = 0x9E3779B97F4A7C15  # the mask draw's Weyl increment (cg_internal.h drop_u)


def dropout(x, keep_prob: float, seed: int, offset: int = 0):
    """y = (x / keep_prob) * floor(keep_prob + u), u ~ U[0,1) per element from
    (seed, index); keep_prob == 1 returns x.

    offset: x is the slice starting at element ``offset`` of a larger tensor
    dropped out under ``seed`` -- element i draws as element offset + i would
    there (the draw hashes seed + DROP_WEYL * (index + 1), so the offset folds
    into the seed: the same mask bits, no wider ABI)."""
    if int(offset) < 0:
        raise ValueError("dropout offset must be >= 0")
    if keep_prob >= 1.0:
        return x
    s = (int(seed) + DROP_WEYL * int(offset)) & ((1 << 64) - 1)
    return _Dropout.apply(x, keep_prob, s)


def clip_by_norm_(grads, clip_norm: float, check_numerics: bool = True):
    """tf.clip_by_norm + tf.check_numerics per gradient tensor, in place
    (gconvRNN.Model._build_optim, lib/gconvRNN.py:392-402): each g becomes
    (g * clip_norm) / max(||g||, clip_norm); with check_numerics a NaN / Inf
    in any clipped gradient raises FloatingPointError (one sync at the end)."""
    flag = None
    for g in grads:
        _check_dev("grad", g)
        if not g.is_contiguous():
            raise ValueError("clip_by_norm_: gradients must be contiguous")
        if flag is None:
            flag = torch.zeros((1,), device=g.device, dtype=torch.int32)
        _lib.call("cg_clip_by_norm", _p(g), g.numel(), float(clip_norm),
                  _p(flag) if check_numerics else None, _stream(g))
    if check_numerics and flag is not None and int(flag.item()):
        raise FloatingPointError("Numerical error in gradient (check_numerics after clip_by_norm)")
    return grads


# -- the per-step output head + vertex softmax loss (lib/gconvRNN.py:306-340) -------
SeqXent = collections.namedtuple("SeqXent", ("loss", "logits", "ce", "dhs", "dw", "db"))


def seq_xent_labels(labels, M: int, device) -> torch.Tensor:
    """Step-major labels [T, N] as the int32 device tensor cg_seq_xent_head
    reads.  Host labels (numpy, lists, CPU tensors) are validated against [0, M)
    before the upload (ValueError); a device tensor is taken as it is -- an
    out-of-range entry then gives that pair NaN, as TF's GPU kernel does."""
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        return labels.to(dtype=torch.int32).contiguous()
    a = np.asarray(labels.numpy() if isinstance(labels, torch.Tensor) else labels)
    if a.dtype.kind not in "iu":
        raise TypeError(f"labels must be integers, got {a.dtype}")
    if a.size and (a.min() < 0 or a.max() >= M):
        raise ValueError(f"labels must lie in [0, {M}), got [{a.min()}, {a.max()}]")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


def seq_xent_workspace_bytes(T: int, N: int, M: int, H: int) -> int:
    return _ws_bytes("cg_seq_xent_workspace_bytes", int(T), int(N), int(M), int(H))[0]


def seq_xent_call(hs, w, b, labels, keep: float = 1.0, seed: int = 0, loss_scale: float = 1.0,
                  need_grad: bool = True, want_logits: bool = False, want_ce: bool = False,
                  ws=None, out_dhs=None, out_dw=None, out_db=None) -> SeqXent:
    """cg_seq_xent_head on hs [T, N, M, H], w [H] (or [H, 1]), b [1], labels
    [T, N] (seq_xent_labels): one pass gives loss [1] = loss_scale * sum ce and,
    with need_grad, dhs, dw [H], db [1]; logits [N, M, T] (pred_out) and ce
    [T, N] on request.  keep < 1 folds DropoutWrapper's mask of stream ``seed``
    (already offset) into the read of hs and the write of dhs."""
    _check_dev("hs", hs)
    _check_dev("w", w)
    _check_dev("b", b)
    _check_dev("labels", labels, torch.int32)
    if hs.dim() != 4:
        raise ValueError("hs must be [T, N, M, H]")
    T, N, M, H = (int(d) for d in hs.shape)
    if w.numel() != H or b.numel() != 1 or tuple(labels.shape) != (T, N):
        raise ValueError(f"need w [{H}], b [1] and labels [{T}, {N}]")
    hs, w, labels = hs.contiguous(), w.contiguous(), labels.contiguous()
    f32 = dict(device=hs.device, dtype=torch.float32)
    if ws is None:
        ws, _ = _workspace("cg_seq_xent_workspace_bytes", T, N, M, H, device=hs.device)
    else:
        seq_xent_workspace_bytes(T, N, M, H)  # (the query also judges the shape)
    loss = torch.empty((1,), **f32)
    logits = torch.empty((N, M, T), **f32) if want_logits else None
    ce = torch.empty((T, N), **f32) if want_ce else None
    dhs = dw = db = None
    if need_grad:
        dhs = _out("out_dhs", out_dhs, hs.shape, hs.device)
        dw = _out("out_dw", out_dw, (H,), hs.device)
        db = _out("out_db", out_db, (1,), hs.device)
    _lib.call("cg_seq_xent_head", _p(hs), _p(w), _p(b), _p(labels), T, N, M, H, float(keep),
              int(seed) & ((1 << 64) - 1), float(loss_scale), _p(logits), _p(ce), _p(loss), _p(dhs),
              _p(dw), _p(db), _p(ws), ws.numel(), _stream(hs))
    return SeqXent(loss, logits, ce, dhs, dw, db)


class _SeqXentHead(torch.autograd.Function):
    """loss (and pred_out) of the head; the gradients are computed by the same
    launch and handed out, times the incoming scalar, in the backward (as the
    trainer uses cg_mse_loss_ema's dpred)."""

    @staticmethod
    def forward(ctx, hs, w, b, labels, keep, seed, loss_scale, want_logits):
        need = any(ctx.needs_input_grad[:3])
        r = seq_xent_call(hs, w.reshape(-1), b, labels, keep, seed, loss_scale, need_grad=need,
                          want_logits=want_logits)
        ctx.w_shape = tuple(w.shape)
        if need:
            ctx.save_for_backward(r.dhs, r.dw, r.db)
        logits = r.logits if want_logits else hs.new_empty(0)
        ctx.mark_non_differentiable(logits)
        return r.loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        dhs, dw, db = ctx.saved_tensors
        n = ctx.needs_input_grad
        return (dhs * dloss if n[0] else None, (dw * dloss).view(ctx.w_shape) if n[1] else None,
                db * dloss if n[2] else None, None, None, None, None, None)


def seq_xent_head(hs, w, b, labels, mask=None, loss_scale: float = 1.0, want_logits: bool = False):
    """The gconvRNN output head and loss (lib/gconvRNN.py:306-340) on hs
    [T, N, M, H]: logits[t, n, m] = hd[t, n, m, :] . w + b over hd = hs through
    ``mask`` = (keep_prob, seed) -- DropoutWrapper's mask, seed already offset --
    or hs itself; loss [1] = loss_scale * sum_{t,n} sparse_softmax_cross_entropy
    (logits[t, n, :], labels[t, n]).  labels [T, N]: host integers (validated
    against [0, M)) or an int32 device tensor.  Returns loss, or (loss, pred_out
    [N, M, T]) with want_logits.  With gradients disabled the launch is the
    forward-only one (dhs = NULL)."""
    _check_dev("hs", hs)
    labels = seq_xent_labels(labels, int(hs.shape[2]), hs.device)
    keep, seed = (1.0, 0) if mask is None else (float(mask[0]), int(mask[1]))
    _check_keep(keep)
    loss, logits = _SeqXentHead.apply(hs, w, b, labels, keep, seed, float(loss_scale),
                                      bool(want_logits))
    return (loss, logits) if want_logits else loss


def adam_update(param, grad, m, v, step: int, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                grad_scale=1.0):
    """In-place TF-1.x Adam step on device (lib/graph_model.py:293)."""
    for name, t in (("param", param), ("grad", grad), ("m", m), ("v", v)):
        _check_dev(name, t)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    _lib.call("cg_adam_update", _p(param), _p(grad), _p(m), _p(v), param.numel(), float(lr),
              float(beta1), float(beta2), float(eps), int(step), float(grad_scale), _stream(param))


def sgd_update(param, grad, lr=1e-3, grad_scale=1.0):
    """In-place tf.train.GradientDescentOptimizer step (lib/gconvRNN.py:383-384)."""
    for name, t in (("param", param), ("grad", grad)):
        _check_dev(name, t)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    _lib.call("cg_sgd_update", _p(param), _p(grad), param.numel(), float(lr), float(grad_scale),
              _stream(param))


def rmsprop_update(param, grad, ms, mom, lr=1e-3, rho=0.9, momentum=0.0, eps=1e-10,
                   grad_scale=1.0):
    """In-place tf.train.RMSPropOptimizer step (lib/gconvRNN.py:387-388; TF 1.x
    ApplyRMSProp, not centered).  ms starts at ONES, mom at zeros (TF 1.x slots)."""
    for name, t in (("param", param), ("grad", grad), ("ms", ms), ("mom", mom)):
        _check_dev(name, t)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    _lib.call("cg_rmsprop_update", _p(param), _p(grad), _p(ms), _p(mom), param.numel(), float(lr),
              float(rho), float(momentum), float(eps), float(grad_scale), _stream(param))


def _check_reg_range(n: int, reg_begin: int, reg_n: int):
    reg_begin, reg_n = int(reg_begin), int(reg_n)
    if reg_begin < 0 or reg_n < 0 or reg_begin + reg_n > n:
        raise ValueError(f"regularised range [{reg_begin}, {reg_begin + reg_n}) outside [0, {n})")
    return reg_begin, reg_n


def momentum_update(param, grad, accum=None, lr=1e-3, momentum=0.9, grad_scale=1.0, reg=0.0,
                    reg_begin: int = 0, reg_n: int = 0):
    """In-place tf.train.MomentumOptimizer step (lib/models.py:24-55; TF 1.x
    ApplyMomentum, no Nesterov) with the L2 term: g = grad * grad_scale, plus
    reg * param on the elements [reg_begin, reg_begin + reg_n); accum = accum *
    momentum + g; param -= lr * accum.  ``accum`` starts at zeros; momentum == 0
    is GradientDescentOptimizer (sgd_update's arithmetic) and takes no accum."""
    ts = [("param", param), ("grad", grad)] + ([("accum", accum)] if accum is not None else [])
    for name, t in ts:
        _check_dev(name, t)
        if not t.is_contiguous() or t.numel() != param.numel():
            raise ValueError(f"{name} must be contiguous with param's {param.numel()} elements")
    if not float(momentum) >= 0.0:
        raise ValueError(f"momentum must be >= 0, got {momentum}")
    if momentum != 0 and accum is None:
        raise ValueError("momentum != 0 needs the accum slot")
    reg_begin, reg_n = _check_reg_range(param.numel(), reg_begin, reg_n)
    _lib.call("cg_momentum_update", _p(param), _p(grad), _p(accum), param.numel(), float(lr),
              float(momentum), float(grad_scale), float(reg), reg_begin, reg_n, _stream(param))


# -- the class loss of the cgcnn classifier (lib/models.py:24-55) --------------------
ClassXent = collections.namedtuple("ClassXent", ("loss", "dlogits", "pred", "correct", "status"))


def class_labels(labels, C: int, device) -> torch.Tensor:
    """Class ids [N] as the int32 device tensor cg_class_xent_ema reads.  Host
    labels (numpy, lists, CPU tensors) are validated against [0, C) before the
    upload (ValueError; once per dataset); a device tensor is taken as it is --
    the kernel clamps what it indexes with, gives such a row NaN and reports it
    in its status word (``class_xent_call(..., check=True)`` raises)."""
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        if labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise TypeError(f"labels must be integers, got {labels.dtype}")
        return labels.to(dtype=torch.int32).contiguous()
    a = np.asarray(labels.numpy() if isinstance(labels, torch.Tensor) else labels)
    if a.dtype.kind not in "iu":
        raise TypeError(f"labels must be integers, got {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"labels must be [N] class ids, got shape {a.shape}")
    if a.size and (a.min() < 0 or a.max() >= C):
        raise ValueError(f"labels must lie in [0, {C}), got [{a.min()}, {a.max()}]")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


def class_xent_workspace_bytes(N: int, C: int, reg_n: int = 0) -> int:
    return _ws_bytes("cg_class_xent_workspace_bytes", int(N), int(C), int(reg_n))[0]


def class_xent_call(logits, labels, params=None, reg_begin: int = 0, reg_n: int = 0,
                    reg_scale: float = 0.0, need_grad: bool = True, ema=None, decay: float = 0.9,
                    want_pred: bool = False, check: bool = False, ws=None,
                    out_dlogits=None) -> ClassXent:
    """cg_class_xent_ema on logits [N, C] and int32 labels [N] (class_labels):
    loss [1] = mean softmax cross-entropy + reg_scale * 1/2 sum params[reg_begin :
    reg_begin + reg_n]^2; with need_grad dlogits = (softmax - onehot) / N; ``ema``
    (fp32 [3], updated in place) the loss moving average; with want_pred the
    first-maximum argmax [N] and the device count [1] of correct rows.
    ``status`` [1] holds the first row + 1 whose label is outside [0, C) (0:
    none); check=True reads it (one sync) and raises ValueError."""
    _check_dev("logits", logits)
    _check_dev("labels", labels, torch.int32)
    if logits.dim() != 2:
        raise ValueError("logits must be [N, C]")
    N, C = (int(d) for d in logits.shape)
    if tuple(labels.shape) != (N,):
        raise ValueError(f"labels must be [{N}], got {tuple(labels.shape)}")
    logits, labels = logits.contiguous(), labels.contiguous()
    reg_begin, reg_n = int(reg_begin), int(reg_n)
    if reg_n:
        if params is None:
            raise ValueError("a regularised range needs params")
        _check_dev("params", params)
        if not params.is_contiguous():
            raise ValueError("params must be contiguous")
        _check_reg_range(params.numel(), reg_begin, reg_n)
    _check_opt("ema", ema, 3, False)
    dev = logits.device
    if ws is None:
        ws, _ = _workspace("cg_class_xent_workspace_bytes", N, C, reg_n, device=dev)
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    dlogits = _out("out_dlogits", out_dlogits, (N, C), dev) if need_grad else None
    i32 = dict(device=dev, dtype=torch.int32)
    pred = torch.empty((N,), **i32) if want_pred else None
    correct = torch.empty((1,), **i32) if want_pred else None
    status = torch.empty((1,), **i32)
    _lib.call("cg_class_xent_ema", _p(logits), _p(labels), N, C, _p(params) if reg_n else None,
              reg_begin, reg_n, float(reg_scale), _p(loss), _p(dlogits), _p(ema), float(decay),
              _p(pred), _p(correct), _p(status), _p(ws), ws.numel(), _stream(logits))
    if check:
        bad = int(status.item())
        if bad:
            raise ValueError(f"label of row {bad - 1} lies outside [0, {C})")
    return ClassXent(loss, dlogits, pred, correct, status)


class _ClassXent(torch.autograd.Function):
    """The loss; dlogits comes out of the same launch and is handed out, times
    the incoming scalar, in the backward (as _SeqXentHead does).  The L2 term's
    gradient is the optimizer's (momentum_update's ``reg``), not autograd's."""

    @staticmethod
    def forward(ctx, logits, labels):
        need = ctx.needs_input_grad[0]
        r = class_xent_call(logits, labels, need_grad=need)
        if need:
            ctx.save_for_backward(r.dlogits)
        return r.loss

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dloss, None


def class_xent(logits, labels):
    """mean_n sparse_softmax_cross_entropy_with_logits(logits [N, C], labels [N])
    (lib/graph_model.py:251-253 as commented out) as a loss [1] with its
    gradient.  labels: host integers (validated against [0, C)) or an integer
    device tensor.  With gradients disabled the launch is the evaluation form."""
    _check_dev("logits", logits)
    return _ClassXent.apply(logits, class_labels(labels, int(logits.shape[-1]), logits.device))


# -- bias + activation (lib/graph_conv.py:178-199, fc :220-226) --------------------
class _BiasAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, act: str):
        _check_dev("x", x)
        x = x.contiguous()
        n = x.numel()
        blen = 1
        if bias is not None:
            _check_dev("bias", bias)
            bias = bias.contiguous()
            blen = bias.numel()
            if n % blen:
                raise ValueError(f"bias of {blen} elements does not tile x of {n}")
        y = torch.empty_like(x)
        _lib.call("cg_bias_act_forward", n, blen, _p(x), _p(bias), ACTS[act], _p(y), _stream(x))
        ctx.save_for_backward(y)
        ctx.act, ctx.blen, ctx.has_bias = act, blen, bias is not None
        ctx.bshape = None if bias is None else tuple(bias.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        n = dy.numel()
        dz = torch.empty_like(dy)
        db = ws = None
        nb = 0
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = torch.empty(ctx.bshape, device=dy.device, dtype=torch.float32)
            ws, nb = _workspace("cg_bias_act_workspace_bytes", n, ctx.blen, device=dy.device)
        _lib.call("cg_bias_act_backward", n, ctx.blen, _p(dy), _p(y), ACTS[ctx.act], _p(dz), _p(db),
                  0, _p(ws), nb, _stream(dy))
        return dz, db, None


def bias_act(x, bias=None, act: str = "relu"):
    """act(x + bias) with bias broadcast over the leading axes (bias [F] or
    [1,1,F]: one per filter; [1,M,F]: one per vertex and filter)."""
    return _BiasAct.apply(x, bias, act)


# -- plain GEMM on MFMA (the tf.matmul of fc / the Fourier transforms) -----------
def gemm(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False,
         out: torch.Tensor | None = None) -> torch.Tensor:
    """op(a) @ op(b) for 2-D fp32 device tensors (cg_gemm_f32)."""
    _check_dev("a", a)
    _check_dev("b", b)
    a, b = a.contiguous(), b.contiguous()
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    Kb, N = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if K != Kb:
        raise ValueError(f"gemm: inner dimensions differ ({K} vs {Kb})")
    out = _out("out", out, (M, N), a.device)
    _lib.call("cg_gemm_f32", int(trans_a), int(trans_b), M, N, K, _p(a), a.shape[1], _p(b), b.shape[1],
              _p(out), N, _stream(a))
    return out


class _MatMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return gemm(a, b)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        da = gemm(dc, b, trans_b=True) if ctx.needs_input_grad[0] else None
        db = gemm(a, dc, trans_a=True) if ctx.needs_input_grad[1] else None
        return da, db


def matmul(a, b):
    """tf.matmul(a, b) for 2-D operands with its gradient, on the HIP GEMM."""
    return _MatMul.apply(a, b)


# -- Fourier filter (lib/graph_conv.py:83-111) ----------------------------------------
class _Fourier(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, U):
        for name, t in (("x", x), ("W", W), ("U", U)):
            _check_dev(name, t)
        x, W, U = x.contiguous(), W.contiguous(), U.contiguous()
        N, M, Fin = (int(s) for s in x.shape)
        if tuple(W.shape[::2]) != (M, Fin) or tuple(U.shape) != (M, M):
            raise ValueError(f"fourier: need W [M, Fout, Fin] = [{M}, *, {Fin}] and U [{M}, {M}], "
                             f"got {tuple(W.shape)} and {tuple(U.shape)}")
        Fout = int(W.shape[1])
        # one query for both sizes: the backward's is kept on ctx, not asked for again
        fb, bb = _ws_bytes("cg_fourier_workspace_bytes", N, M, Fin, Fout, sizes=2)
        xhat = torch.empty((N, Fin, M), device=x.device, dtype=torch.float32)
        y = torch.empty((N, M, Fout), device=x.device, dtype=torch.float32)
        ws = torch.empty(max(fb, 1), device=x.device, dtype=torch.uint8)
        _lib.call("cg_fourier_forward", N, M, Fin, Fout, _p(U), _p(W), _p(x), _p(xhat), _p(y), _p(ws),
                  fb, _stream(x))
        ctx.save_for_backward(xhat, W, U)
        ctx.shape, ctx.bwd_bytes = (N, M, Fin, Fout), bb
        return y

    @staticmethod
    def backward(ctx, dy):
        xhat, W, U = ctx.saved_tensors
        N, M, Fin, Fout = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty((N, M, Fin), device=dy.device, dtype=torch.float32) \
            if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(W) if ctx.needs_input_grad[1] else None
        ws = torch.empty(max(ctx.bwd_bytes, 1), device=dy.device, dtype=torch.uint8)
        _lib.call("cg_fourier_backward", N, M, Fin, Fout, _p(U), _p(W), _p(xhat), _p(dy), _p(dx), _p(dW),
                  _p(ws), ctx.bwd_bytes, _stream(dy))
        return dx, dW, None


def fourier_conv(x, W, U):
    """filter_in_fourier (lib/graph_conv.py:83-99): x [N, M, Fin], W [M, Fout,
    Fin], U [M, M] (eigenvectors in columns, device fp32) -> [N, M, Fout]."""
    return _Fourier.apply(x, W, U)


# -- gconv-LSTM with the Fourier filter (lib/gconv_lstm.py:116-133, :183-221) --------
# Spectral tensors keep the sample-major layout of the vertex-domain ones,
# [..., M, C] with the frequency in the place of the vertex.
def gft_prepare(U: torch.Tensor) -> torch.Tensor:
    """The graph's transform operand for gft / flstm_step, prepared once from
    U [M, M] (cg_gft_prepare): an opaque uint8 device buffer."""
    _check_dev("U", U)
    U = U.contiguous()
    M = int(U.shape[0])
    if tuple(U.shape) != (M, M):
        raise ValueError(f"U must be square, got {tuple(U.shape)}")
    basis, nb = _workspace("cg_gft_workspace_bytes", M, device=U.device)
    _lib.call("cg_gft_prepare", M, _p(U), _p(basis), nb, _stream(U))
    return basis


def gft(basis: torch.Tensor, x: torch.Tensor, inverse: bool = False, out: torch.Tensor | None = None):
    """Batched graph Fourier transform of x [..., M, C]: U^T x per sample
    (analysis) or U x (inverse=True, synthesis), on MFMA (cg_gft)."""
    _check_dev("x", x)
    x = x.contiguous()
    M, C = int(x.shape[-2]), int(x.shape[-1])
    N = x.numel() // (M * C)
    out = _out("out", out, x.shape, x.device, elems=(N, M, C))
    _lib.call("cg_gft", int(bool(inverse)), N, M, C, _p(basis), basis.numel(), _p(x), _p(out),
              _stream(x))
    return out


FOURIER_MIX_FORMS = {"fwd": 0, "t": 1, "dw": 2}


def fourier_mix(form: str, W=None, x=None, g=None, add=None, out=None):
    """Per-frequency contraction on MFMA (cg_fourier_mix); W [M, Cout, Cin],
    x [..., M, Cin], g [..., M, Cout]:
      "fwd": add + W[m] x[., m, :]  -> [..., M, Cout]   (add None = 0; out may be add)
      "t":   W[m]^T g[., m, :]      -> [..., M, Cin]
      "dw":  sum over rows of g (x) x -> [M, Cout, Cin] (fixed order: bitwise reproducible)"""
    f = FOURIER_MIX_FORMS[form]
    ref = x if f != 1 else g
    for name, t in (("W", W), ("x", x), ("g", g), ("add", add)):
        if t is not None:
            _check_dev(name, t)
            if not t.is_contiguous():
                raise ValueError(f"{name}: must be contiguous")
    if f != 2:
        M, Cout, Cin = (int(s) for s in W.shape)
    else:
        M, Cin, Cout = int(x.shape[-2]), int(x.shape[-1]), int(g.shape[-1])
    R = ref.numel() // (M * int(ref.shape[-1]))
    lead = tuple(ref.shape[:-2])
    if x is not None and (f != 1) and (int(x.shape[-2]), int(x.shape[-1])) != (M, Cin):
        raise ValueError(f"x: need [..., {M}, {Cin}], got {tuple(x.shape)}")
    if g is not None and (f != 0) and ((int(g.shape[-2]), int(g.shape[-1])) != (M, Cout) or
                                       g.numel() != R * M * Cout):
        raise ValueError(f"g: need {R} rows of [{M}, {Cout}], got {tuple(g.shape)}")
    shape = (lead + (M, Cout), lead + (M, Cin), (M, Cout, Cin))[f]
    if out is None:
        out = torch.empty(shape, device=ref.device, dtype=torch.float32)
    n = 1
    for s in shape:
        n *= s
    _check_out("out", out, (n,))
    if add is not None and add.numel() != n:
        raise ValueError(f"add: bad shape {tuple(add.shape)}")
    _lib.call("cg_fourier_mix", f, R, M, Cin, Cout, _p(W), _p(x) if f != 1 else None,
              _p(g) if f != 0 else None, _p(add), _p(out), _stream(ref))
    return out


# -- residual block with the Fourier filter (lib/graph_conv.py:83-111 in :234-262) ------
def fres_workspace_bytes(N: int, M: int, Fin: int, Fout: int):
    """(forward, backward) workspace bytes of cg_fres_forward / cg_fres_backward."""
    return tuple(_ws_bytes("cg_fres_workspace_bytes", int(N), int(M), int(Fin), int(Fout), sizes=2))


def _check_keep(keep_prob):
    if not 0.0 < float(keep_prob) <= 1.0:
        raise ValueError(f"keep_prob must be in (0, 1], got {keep_prob}")


def fres_forward(basis, W, x, residual=None, act: str = "none", out_xhat=None, out_y=None,
                 keep_prob: float = 1.0, seed: int = 0, ws=None):
    """y = act(U (W[m] U^T x) + residual) in three launches (cg_fres_forward):
    x [N, M, Fin], W [M, Fout, Fin], basis from gft_prepare.  Returns
    (xhat [N, M, Fin], y [N, M, Fout]).

    keep_prob < 1 (cg_fres_forward_drop) is fres_forward of dropout(x, keep_prob,
    seed) without the dropped tensor: the mask is applied while the analysis
    stages x -- bit for bit ``dropout`` then ``fres_forward``, and xhat is the
    dropped x's.  ``seed`` already carries a slice offset (``dropout``'s
    folding: seed + DROP_WEYL * offset)."""
    _check_keep(keep_prob)
    for name, t in (("x", x), ("W", W)):
        _check_dev(name, t)
    x, W = x.contiguous(), W.contiguous()
    N, M, Fin = (int(s) for s in x.shape)
    if W.dim() != 3 or tuple(W.shape[::2]) != (M, Fin):
        raise ValueError(f"W must be [M, Fout, Fin] = [{M}, *, {Fin}], got {tuple(W.shape)}")
    Fout = int(W.shape[1])
    if residual is not None:
        _check_dev("residual", residual)
        residual = residual.contiguous()
        if residual.numel() != N * M * Fout:
            raise ValueError(f"residual must be [N, M, Fout] = [{N}, {M}, {Fout}]")
    xhat = _out("xhat", out_xhat, (N, M, Fin), x.device)
    y = _out("y", out_y, (N, M, Fout), x.device)
    if ws is None:
        ws, _ = _workspace("cg_fres_workspace_bytes", N, M, Fin, Fout, device=x.device, sizes=2)
    head = (N, M, Fin, Fout, _p(basis), basis.numel(), _p(W), _p(x))
    tail = (_p(residual), ACTS[act], _p(xhat), _p(y), _p(ws), ws.numel(), _stream(x))
    if keep_prob == 1.0:
        _lib.call("cg_fres_forward", *head, *tail)
    else:
        _lib.call("cg_fres_forward_drop", *head, float(keep_prob), int(seed) & ((1 << 64) - 1), *tail)
    return xhat, y


def fres_backward(basis, W, xhat, dy, y=None, act: str = "none", need_dz: bool = True, dx=None,
                  dx_accumulate: bool = False, need_dx: bool = True, out_dz=None, out_dW=None,
                  keep_prob: float = 1.0, seed: int = 0, ws=None):
    """Backward through fres_forward (cg_fres_backward): returns (dx, dW, dz)
    with dz = dy * [y > 0] the gradient of the residual input; with
    dx_accumulate the input gradient is added into the given ``dx``.

    keep_prob < 1 (cg_fres_backward_drop) is the backward of that forward: dx is
    the gradient of the UNdropped x -- the synthesis stores (acc * mask) /
    keep_prob, bit for bit ``fres_backward`` then the dropout's backward on dx.
    It always computes dx and never accumulates."""
    _check_keep(keep_prob)
    if keep_prob < 1.0 and (dx_accumulate or not need_dx):
        raise ValueError("keep_prob < 1 stores dx through the mask: no dx_accumulate, no need_dx=False")
    for name, t in (("W", W), ("xhat", xhat), ("dy", dy)):
        _check_dev(name, t)
    dy, W = dy.contiguous(), W.contiguous()
    N, M, Fout = (int(s) for s in dy.shape)
    Fin = int(W.shape[2])
    f32 = dict(device=dy.device, dtype=torch.float32)
    if act == "relu":
        if y is None:
            raise ValueError("act relu needs the forward's output y")
        _check_out("y", y, (N, M, Fout))
    _check_out("xhat", xhat, (N, M, Fin))
    if need_dx and dx is None:
        if dx_accumulate:
            raise ValueError("dx_accumulate needs a dx tensor")
        dx = torch.empty((N, M, Fin), **f32)
    if not need_dx:
        dx = None
    if dx is not None:
        _check_out("dx", dx, (N, M, Fin))
    dz = _out("dz", out_dz, (N, M, Fout), dy.device) if need_dz else None
    dW = _out("dW", out_dW, (M, Fout, Fin), dy.device)
    if ws is None:
        ws, _ = _workspace("cg_fres_workspace_bytes", N, M, Fin, Fout, device=dy.device, sizes=2,
                           pick=1)
    head = (N, M, Fin, Fout, _p(basis), basis.numel(), _p(W), _p(xhat), _p(dy),
            _p(y) if act == "relu" else None, ACTS[act])
    tail = (_p(dW), _p(ws), ws.numel(), _stream(dy))
    if keep_prob == 1.0:
        _lib.call("cg_fres_backward", *head, _p(dz), _p(dx), int(dx_accumulate), *tail)
    else:
        _lib.call("cg_fres_backward_drop", *head, float(keep_prob), int(seed) & ((1 << 64) - 1), _p(dz),
                  _p(dx), *tail)
    return dx, dW, dz


def fres_forward_drop(basis, W, x, keep_prob: float, seed: int, residual=None, act: str = "none",
                      out_xhat=None, out_y=None, ws=None):
    """fres_forward with the seam's arguments in front (cg_fres_forward_drop)."""
    return fres_forward(basis, W, x, residual, act, out_xhat, out_y, keep_prob, seed, ws)


def fres_backward_drop(basis, W, xhat, dy, keep_prob: float, seed: int, y=None, act: str = "none",
                       need_dz: bool = True, out_dx=None, out_dz=None, out_dW=None, ws=None):
    """fres_backward with the seam's arguments in front (cg_fres_backward_drop);
    dx is always computed."""
    return fres_backward(basis, W, xhat, dy, y, act, need_dz, dx=out_dx, out_dz=out_dz, out_dW=out_dW,
                         keep_prob=keep_prob, seed=seed, ws=ws)


class _FourierAct(torch.autograd.Function):
    """y = act(fourier(x; W) + residual) over cg_fres_forward / cg_fres_backward;
    saves xhat and y, the residual's gradient is the masked dz."""

    @staticmethod
    def forward(ctx, x, W, residual, basis, act: str):
        xhat, y = fres_forward(basis, W, x, residual, act)
        ctx.save_for_backward(xhat, W, y, basis)
        ctx.act, ctx.has_res = act, residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xhat, W, y, basis = ctx.saved_tensors
        need_dz = ctx.has_res and ctx.needs_input_grad[2]
        dx, dW, dz = fres_backward(basis, W, xhat, dy, y, ctx.act, need_dz=need_dz,
                                   need_dx=ctx.needs_input_grad[0])
        return dx, dW, dz, None, None


def fourier_conv_act(x, W, basis, residual=None, act: str = "none"):
    """act(filter_in_fourier(x; W) + residual) on the MFMA transforms with the
    residual add and the ReLU in the synthesis' store: x [N, M, Fin], W [M, Fout,
    Fin], basis = gft_prepare(U), residual [N, M, Fout] or None, act "none" /
    "relu" -> [N, M, Fout]."""
    return _FourierAct.apply(x, W, residual, basis, act)


def flstm_supported(M: int, H: int, Fin: int) -> bool:
    """Whether cg_flstm_step serves this hidden size (H a multiple of 8)."""
    return _supported("cg_flstm_supported", int(M), int(H), int(Fin))


def flstm_step(basis, h_prev, c_prev, ghat_x, Wh, bias, gates="reference", out_c=None, out_h=None,
               out_act=None, out_hhat=None):
    """One forward step of the Fourier gconv-LSTM's recurrent part
    (cg_flstm_step: analysis of h_prev, per-frequency accumulate onto ghat_x,
    synthesis with the gate update in its epilogue).  ghat_x [N, M, 4H]; h_prev,
    c_prev [N, M, H] or None (zero state).  Returns (c', h', act, hhat)."""
    _check_dev("ghat_x", ghat_x)
    N, M, H4 = (int(s) for s in ghat_x.shape)
    H = H4 // 4
    R = N * M
    dev = ghat_x.device
    for name, t, n in (("h_prev", h_prev, R * H), ("c_prev", c_prev, R * H), ("bias", bias, 4 * H),
                       ("Wh", Wh, M * 4 * H * H), ("ghat_x", ghat_x, R * 4 * H)):
        _check_opt(name, t, n, aligned=False)
    c_out, h_out, act = _cell_outs(out_c, out_h, out_act, (N, M), R, H, dev)
    hhat, ws, nbytes = None, None, 0
    if h_prev is not None:
        hhat = _out("hhat", out_hhat, (N, M, H), dev, elems=(R, H))
        ws, nbytes = _workspace("cg_flstm_workspace_bytes", N, M, H, device=dev)
    _lib.call("cg_flstm_step", N, M, H, LSTM_GATES[gates], _p(basis), basis.numel(), _p(h_prev),
              _p(c_prev), _p(ghat_x), _p(Wh), _p(bias), _p(c_out), _p(h_out), _p(act), _p(hhat),
              _p(ws), nbytes, _stream(ghat_x))
    return c_out, h_out, act, hhat


# -- stacked-input ResGNN pieces (lib/graph_conv.py:272-303) -----------------------
class _SliceChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c0: int, c1: int):
        _check_dev("x", x)
        x = x.contiguous()
        C = int(x.shape[-1])
        rows = x.numel() // C
        out = torch.empty(tuple(x.shape[:-1]) + (c1 - c0,), device=x.device, dtype=torch.float32)
        _lib.call("cg_slice_channels", _p(x), rows, C, int(c0), int(c1), _p(out), _stream(x))
        ctx.shape, ctx.c0, ctx.c1 = tuple(x.shape), c0, c1
        return out

    @staticmethod
    def backward(ctx, dy):
        raise RuntimeError("slice_channels: the input channels are data (no gradient), "
                           "as in lib/graph_conv.py:274-303")


def slice_channels(x, c0: int, c1: int):
    """x[..., c0:c1] of a [N, M, C] device tensor as a new contiguous tensor
    (the reshape / unstack / concat of lib/graph_conv.py:281-286)."""
    return _SliceChannels.apply(x, int(c0), int(c1))


class _StackMerge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out_i, w_i, acc):
        for name, t in (("out_i", out_i), ("w_i", w_i)):
            _check_dev(name, t)
        out_i, w_i = out_i.contiguous(), w_i.contiguous()
        N, M, F = (int(s) for s in out_i.shape)
        if tuple(w_i.shape) != (M, F):
            raise ValueError(f"merge weight must be [{M}, {F}], got {tuple(w_i.shape)}")
        y = torch.empty_like(out_i)
        if acc is not None:
            y.copy_(acc)  # (buffer plumbing: the kernel accumulates into y)
        _lib.call("cg_stack_merge_forward", N, M, F, _p(out_i), _p(w_i), int(acc is not None), _p(y),
                  _stream(out_i))
        ctx.save_for_backward(out_i, w_i)
        ctx.has_acc = acc is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        out_i, w_i = ctx.saved_tensors
        dy = dy.contiguous()
        N, M, F = (int(s) for s in out_i.shape)
        d_o = torch.empty_like(out_i) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w_i) if ctx.needs_input_grad[1] else None
        if d_o is not None or dw is not None:
            _lib.call("cg_stack_merge_backward", N, M, F, _p(dy), _p(out_i), _p(w_i), _p(d_o), _p(dw),
                      _stream(dy))
        return d_o, dw, (dy if ctx.has_acc else None)


def stack_merge(out_i, w_i, acc=None):
    """acc + relu(out_i) * w_i (w_i [M, F] broadcast over N; acc None: no add)
    -- one term of X = sum_i relu(net_i) * w_i, lib/graph_conv.py:292-301."""
    return _StackMerge.apply(out_i, w_i, acc)


# -- the branch seams of the closeness / period / trend networks (lib/gconv_lstm.py:431-607) --
MAX_BRANCHES = 4


def _ptr_array(ts):
    """A host array of device pointers (None entries = NULL) for the cg_branch_* / cg_concat_* calls."""
    return (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])


def _branches(name, ts, lead=None):
    """The branches of one seam call: 1 .. MAX_BRANCHES fp32 device tensors
    (made contiguous), every one [*lead, C_b] when ``lead`` is given."""
    ts = list(ts)
    if not 1 <= len(ts) <= MAX_BRANCHES:
        raise ValueError(f"{name}: 1 to {MAX_BRANCHES} branches, got {len(ts)}")
    for b, t in enumerate(ts):
        _check_dev(f"{name}[{b}]", t)
        if lead is not None and (t.dim() != len(lead) + 1 or tuple(t.shape[:-1]) != tuple(lead)):
            raise ValueError(f"{name}[{b}] must be [{', '.join(map(str, lead))}, *], got {tuple(t.shape)}")
    return [t.contiguous() for t in ts]


def branch_merge_forward(ys, ws, out=None):
    """cg_branch_merge_forward: ((y_0 w_0) + y_1 w_1) + ... with y_b [N, M, F]
    and w_b [M, F] broadcast over N, every product and sum rounded in that order."""
    ys = _branches("ys", ys)
    N, M, F = (int(s) for s in ys[0].shape)
    ys = _branches("ys", ys, (N, M))
    ws = _branches("ws", ws, (M,))
    if len(ws) != len(ys) or any(int(t.shape[-1]) != F for t in ys + ws):
        raise ValueError(f"branch_merge: need as many w [{M}, {F}] as y [{N}, {M}, {F}]")
    out = _out("out", out, (N, M, F), ys[0].device)
    _lib.call("cg_branch_merge_forward", len(ys), N, M, F, _ptr_array(ys), _ptr_array(ws), _p(out),
              _stream(ys[0]))
    return out


def branch_merge_backward(dout, ys, ws, need_dy=None, need_dw=None, out_dw=None,
                          accumulate_dw: bool = False):
    """cg_branch_merge_backward, ONE launch: (dys, dws) with dy_b = dout w_b and
    dw_b (+)= sum_n dout y_b; need_dy / need_dw: per-branch flags (default all),
    a False entry is skipped (None in its place).  out_dw: the tensors to write
    (accumulate_dw: to add into)."""
    ys = _branches("ys", ys)
    N, M, F = (int(s) for s in ys[0].shape)
    ws = _branches("ws", ws, (M,))
    B = len(ys)
    _check_dev("dout", dout)
    dout = dout.contiguous()
    if len(ws) != B or tuple(dout.shape) != (N, M, F):
        raise ValueError(f"branch_merge_backward: need dout [{N}, {M}, {F}] and {B} weights")
    need_dy = [True] * B if need_dy is None else list(need_dy)
    need_dw = [True] * B if need_dw is None else list(need_dw)
    dev = dout.device
    dys = [torch.empty((N, M, F), device=dev, dtype=torch.float32) if need_dy[b] else None
           for b in range(B)]
    dws = [_out(f"out_dw[{b}]", out_dw[b] if out_dw is not None else None, (M, F), dev,
                accumulate=accumulate_dw) if need_dw[b] else None for b in range(B)]
    if any(need_dy) or any(need_dw):
        _lib.call("cg_branch_merge_backward", B, N, M, F, _p(dout), _ptr_array(ys), _ptr_array(ws),
                  _ptr_array(dys), _ptr_array(dws), int(bool(accumulate_dw)), _stream(dout))
    return dys, dws


class _BranchMerge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, B, *yw):
        ys, ws = yw[:B], yw[B:]
        out = branch_merge_forward(ys, ws)
        ctx.save_for_backward(*ys, *ws)
        ctx.B = B
        return out

    @staticmethod
    def backward(ctx, dout):
        B, saved = ctx.B, ctx.saved_tensors
        need = ctx.needs_input_grad[1:]
        dys, dws = branch_merge_backward(dout, saved[:B], saved[B:], need[:B], need[B:])
        return (None, *dys, *dws)


def branch_merge(ys, ws):
    """X = sum_b y_b * w_b as the reference graph chains it (lib/gconv_lstm.py
    :494-497): ys B tensors [N, M, F], ws B tensors [M, F]; no activation.  The
    backward is one launch for every branch (cg_branch_merge_backward)."""
    ys, ws = list(ys), list(ws)
    if len(ys) != len(ws):
        raise ValueError("branch_merge: as many weights as branches")
    return _BranchMerge.apply(len(ys), *ys, *ws)


def _concat_args(hs, keep, seeds):
    N, M = int(hs[0].shape[0]), int(hs[0].shape[1])
    B = len(hs)
    if not 0.0 < float(keep) <= 1.0:
        raise ValueError(f"keep must be in (0, 1], got {keep}")
    seeds = [0] * B if seeds is None else [int(s) & ((1 << 64) - 1) for s in seeds]
    if len(seeds) != B:
        raise ValueError("concat_drop: one seed per branch")
    H = [int(t.shape[-1]) for t in hs]
    return N, M, B, H, (ctypes.c_int32 * B)(*H), (ctypes.c_uint64 * B)(*seeds)


def concat_drop_forward(hs, keep: float = 1.0, seeds=None, out=None):
    """cg_concat_drop_forward: cat_b(dropout(h_b, keep, seed_b)) along the last
    axis in one pass (seed_b already offset, as ``dropout``'s folded seed is)."""
    hs = _branches("hs", hs)
    hs = _branches("hs", hs, tuple(hs[0].shape[:2]))
    N, M, B, H, Hc, sc = _concat_args(hs, keep, seeds)
    out = _out("out", out, (N, M, sum(H)), hs[0].device)
    _lib.call("cg_concat_drop_forward", B, N, M, Hc, _ptr_array(hs), float(keep), sc, _p(out),
              _stream(hs[0]))
    return out


def concat_drop_backward(dx, H, keep: float = 1.0, seeds=None):
    """cg_concat_drop_backward: dx [N, M, sum H] split into the branches' dh_b
    [N, M, H_b] through the masks' backward form."""
    _check_dev("dx", dx)
    dx = dx.contiguous()
    N, M, S = (int(s) for s in dx.shape)
    if sum(H) != S:
        raise ValueError(f"concat_drop_backward: dx has {S} channels, the branches {sum(H)}")
    dhs = [torch.empty((N, M, int(h)), device=dx.device, dtype=torch.float32) for h in H]
    _, _, B, _, Hc, sc = _concat_args(dhs, keep, seeds)
    _lib.call("cg_concat_drop_backward", B, N, M, Hc, _p(dx), float(keep), sc, _ptr_array(dhs),
              _stream(dx))
    return dhs


class _ConcatDrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, keep, seeds, *hs):
        out = concat_drop_forward(hs, keep, seeds)
        ctx.keep, ctx.seeds, ctx.H = keep, seeds, [int(t.shape[-1]) for t in hs]
        return out

    @staticmethod
    def backward(ctx, dx):
        return (None, None, *concat_drop_backward(dx, ctx.H, ctx.keep, ctx.seeds))


def concat_drop(hs, keep: float = 1.0, seeds=None):
    """tf.concat(hs, axis=2) of the branches' h_T [N, M, H_b] (lib/gconv_lstm.py
    :451, :590), each branch through its own DropoutWrapper mask (keep, seed_b)
    on the way: the values of ``torch.cat([dropout(h_b, keep, seed_b)])`` bit
    for bit, without the dropped tensors and the concat copy.  seed_b is the
    folded seed (``seed + DROP_WEYL * offset``); keep == 1 is a plain concat."""
    return _ConcatDrop.apply(float(keep), None if seeds is None else tuple(int(s) for s in seeds), *hs)


# -- the dense LSTM baseline (lib/gconvRNN.py:280-285, :300; TF 1.x BasicLSTMCell) ----
DENSE_LSTM_PATHS = ("seq", "steps")


def dense_lstm_supported(H: int) -> bool:
    """Whether the one-launch kernels (cg_dlstm_seq_*) serve this hidden size."""
    return _supported("cg_dlstm_supported", int(H))


def _dlstm_ws(T: int, N: int, H: int, dev, pick: int):
    nb = _ws_bytes("cg_dlstm_workspace_bytes", T, N, H, sizes=2)[pick]
    return (torch.empty(nb, device=dev, dtype=torch.uint8) if nb else None), nb


def dense_lstm_seq_forward(gx, Wh, bias, forget_bias: float = 1.0, need_act: bool = True):
    """cg_dlstm_seq_forward: gx [T, N, 4H] (gate blocks i | j | f | o), Wh [H, 4H],
    bias [4H] -> (hs [T, N, H], cs [T, N, H], act [T, N, 4H] or None)."""
    for name, t in (("gx", gx), ("Wh", Wh), ("bias", bias)):
        _check_dev(name, t)
    T, N, G = (int(v) for v in gx.shape)
    H = G // 4
    _check_weight("Wh", Wh, H, G)
    _check_opt("bias", bias, G, aligned=False)
    if not gx.is_contiguous():
        raise ValueError("gx must be contiguous")
    f32 = dict(device=gx.device, dtype=torch.float32)
    hs, cs = torch.empty((T, N, H), **f32), torch.empty((T, N, H), **f32)
    act = torch.empty((T, N, G), **f32) if need_act else None
    ws, nb = _dlstm_ws(T, N, H, gx.device, 0)
    _lib.call("cg_dlstm_seq_forward", T, N, H, _p(gx), _p(Wh), _p(bias), float(forget_bias), _p(hs),
              _p(cs), _p(act), _p(ws), nb, _stream(gx))
    return hs, cs, act


def dense_lstm_seq_backward(dhs, act, cs, Wh, forget_bias: float = 1.0):
    """cg_dlstm_seq_backward: dpre [T, N, 4H] of the whole sequence from the
    output gradients dhs [T, N, H] and the forward's act and cs."""
    for name, t in (("dhs", dhs), ("act", act), ("cs", cs), ("Wh", Wh)):
        _check_dev(name, t)
    T, N, H = (int(v) for v in cs.shape)
    _check_weight("Wh", Wh, H, 4 * H)
    dhs = dhs.contiguous()
    if dhs.numel() != cs.numel() or act.numel() != 4 * cs.numel() or not act.is_contiguous():
        raise ValueError("dense_lstm_seq_backward: dhs / act do not match cs")
    dpre = torch.empty((T, N, 4 * H), device=cs.device, dtype=torch.float32)
    ws, nb = _dlstm_ws(T, N, H, cs.device, 1)
    _lib.call("cg_dlstm_seq_backward", T, N, H, _p(dhs), _p(act), _p(cs), _p(Wh), float(forget_bias),
              _p(dpre), _p(ws), nb, _stream(cs))
    return dpre


def _dlstm_perm(H: int, dev):
    """Column gather that takes TF's i | j | f | o to the cell kernels' z | i | f | o
    (z = j), and its inverse."""
    u = torch.arange(H, device=dev)
    perm = torch.cat([H + u, u, 2 * H + u, 3 * H + u])
    return perm, torch.argsort(perm)


class _DenseLSTMSeq(torch.autograd.Function):
    """BasicLSTMCell under static_rnn from the zero state over xs [T*N, C]:
    ``kernel`` [C + H, 4H] is TF's single variable (Wx its first C rows, Wh the
    rest), ``bias`` [4H].  path "seq": one cg_gemm_f32 for gx, then ONE launch a
    direction (cg_dlstm_seq_forward / _backward).  path "steps": the same
    network from the existing entries, per step cg_gemm_f32 (h Wh) and
    cg_lstm_cell_forward / _backward with the standard gates on columns
    permuted to z | i | f | o and forget_bias folded into the f bias.  Either
    way dWx = xs^T dpre, dWh = hs[0:T-1]^T dpre[1:T] (zeros for T = 1, no
    zero-row GEMM) and db = cg_bias_grad(dpre) land in one [C + H, 4H] gradient."""

    @staticmethod
    def forward(ctx, xs, kernel, bias, T: int, N: int, forget_bias: float, path: str):
        for name, t in (("xs", xs), ("kernel", kernel), ("bias", bias)):
            _check_dev(name, t)
        xs = xs.contiguous()
        C, G = int(xs.shape[1]), int(kernel.shape[1])
        H = G // 4
        if xs.shape[0] != T * N or tuple(kernel.shape) != (C + H, 4 * H) or not kernel.is_contiguous():
            raise ValueError(f"dense_lstm_seq: need xs [T*N, C] and a contiguous kernel [C + H, 4H], "
                             f"got {tuple(xs.shape)} and {tuple(kernel.shape)}")
        ctx.dims, ctx.fb, ctx.path = (T, N, C, H), float(forget_bias), path
        if path == "seq":
            gx = gemm(xs, kernel[:C]).view(T, N, G)
            hs, cs, act = dense_lstm_seq_forward(gx, kernel[C:], bias, forget_bias)
            ctx.save_for_backward(xs, kernel, hs, cs, act)
            return hs
        perm, _ = _dlstm_perm(H, xs.device)
        kp = kernel.index_select(1, perm)
        bp = bias.index_select(0, perm)
        bp[2 * H:3 * H] += float(forget_bias)
        gx = gemm(xs, kp[:C]).view(T, N, G)
        f32 = dict(device=xs.device, dtype=torch.float32)
        hs, cs, act = torch.empty((T, N, H), **f32), torch.empty((T, N, H), **f32), torch.empty((T, N, G), **f32)
        gh = torch.empty((N, G), **f32)
        for t in range(T):
            if t:
                gemm(hs[t - 1], kp[C:], out=gh)
            lstm_cell_forward(gx[t], gh if t else None, bp, cs[t - 1] if t else None, H, "standard",
                              out_c=cs[t], out_h=hs[t], out_act=act[t])
        ctx.save_for_backward(xs, kp, hs, cs, act)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        xs, kernel, hs, cs, act = ctx.saved_tensors
        T, N, C, H = ctx.dims
        G = 4 * H
        dhs = dhs.contiguous()
        f32 = dict(device=xs.device, dtype=torch.float32)
        Wh = kernel[C:]
        if ctx.path == "seq":
            dpre = dense_lstm_seq_backward(dhs, act, cs, Wh, ctx.fb)
        else:
            dpre = torch.empty((T, N, G), **f32)
            dh_rec, dc = None, None
            for t in range(T - 1, -1, -1):
                _, dc = lstm_cell_backward(dhs[t], dh_rec, dc, act[t], cs[t - 1] if t else None, cs[t], H,
                                           "standard", out_dpre=dpre[t], need_dc_prev=t > 0)
                if t:
                    dh_rec = gemm(dpre[t], Wh, trans_b=True)
        d2 = dpre.view(T * N, G)
        dk = torch.empty((C + H, G), **f32)
        gemm(xs, d2, trans_a=True, out=dk[:C])
        if T > 1:
            gemm(hs.view(T * N, H)[:(T - 1) * N], d2[N:], trans_a=True, out=dk[C:])
        else:
            dk[C:].zero_()
        db = bias_grad(d2)
        if ctx.path != "seq":
            _, inv = _dlstm_perm(H, xs.device)
            dk, db = dk.index_select(1, inv), db.index_select(0, inv)
        dx = gemm(d2, kernel[:C], trans_b=True) if ctx.needs_input_grad[0] else None
        return dx, dk, db, None, None, None, None


def dense_lstm_seq(xs, kernel, bias, T: int, N: int, forget_bias: float = 1.0, path: str = "seq"):
    """hs [T, N, H] of the dense LSTM over xs [T*N, C] (step-major rows), with
    its gradients (``_DenseLSTMSeq``).  ``path``: "seq" (one launch a direction;
    H % 16 == 0, 16 <= H <= 128) or "steps" (per-step composition of the
    existing entries, any H)."""
    if path not in DENSE_LSTM_PATHS:
        raise ValueError(f"path must be one of {DENSE_LSTM_PATHS}, got {path!r}")
    return _DenseLSTMSeq.apply(xs, kernel, bias, int(T), int(N), float(forget_bias), path)


ClassXentSum = collections.namedtuple("ClassXentSum", ("loss", "dlogits", "ce", "pred", "correct", "status"))


def class_xent_sum(logits, labels, loss_scale: float, need_grad: bool = True, want_ce: bool = False,
                   want_pred: bool = False, ws=None, out_dlogits=None) -> ClassXentSum:
    """cg_class_xent_sum on logits [R, C] and int32 labels [R] (class_labels):
    loss [1] = loss_scale * sum_rows ce; with need_grad dlogits = loss_scale *
    (softmax - onehot).  No L2 term, no moving average.  ``status`` as in
    class_xent_call."""
    _check_dev("logits", logits)
    _check_dev("labels", labels, torch.int32)
    if logits.dim() != 2:
        raise ValueError("logits must be [R, C]")
    R, C = (int(d) for d in logits.shape)
    if labels.numel() != R:
        raise ValueError(f"labels must hold {R} class ids, got {tuple(labels.shape)}")
    logits, labels = logits.contiguous(), labels.contiguous()
    dev = logits.device
    if ws is None:
        ws, _ = _workspace("cg_class_xent_workspace_bytes", R, C, 0, device=dev)
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    dlogits = _out("out_dlogits", out_dlogits, (R, C), dev) if need_grad else None
    i32 = dict(device=dev, dtype=torch.int32)
    ce = torch.empty((R,), device=dev, dtype=torch.float32) if want_ce else None
    pred = torch.empty((R,), **i32) if want_pred else None
    correct = torch.empty((1,), **i32) if want_pred else None
    status = torch.empty((1,), **i32)
    _lib.call("cg_class_xent_sum", _p(logits), _p(labels), R, C, float(loss_scale), _p(loss),
              _p(dlogits), _p(ce), _p(pred), _p(correct), _p(status), _p(ws), ws.numel(),
              _stream(logits))
    return ClassXentSum(loss, dlogits, ce, pred, correct, status)
