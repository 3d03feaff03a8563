"""The cases behind tests/golden/ops_pinned.json: what the LSTM, gradient, loss
and flstm wrappers of cnn_graph_amd/ops.py refuse (exception type and text) and
SHA-256 digests of what they compute.

scripts/record_ops_pinned.py records them, tests/test_gpu_ops_pinned.py replays
them.  Every refusal is raised by a Python-side check before any launch.  The
kernels behind the results reduce in a fixed order, so the bits are a function
of the inputs (numpy.random.default_rng on the host) and the shapes.

Shapes: config A's graph (M = 100), H = 32 (the sequence and fused kernels
need it), K = 3, T = 3, N = 3 and 4 (an odd and an even number of samples meet
the sequence kernel's pair hand-off), feat_in 2 on the x-fused path and 12 off
it, zero and given initial state, allocated and caller-supplied outputs;
flstm_step at H = 8."""
import hashlib
import os

import numpy as np
import scipy.sparse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, K, T = 32, 3, 3
FH = 8  # flstm_step's hidden size


def digest(t):
    if t is None:
        return None
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def digests(names, tensors):
    return dict(zip(names, map(digest, tensors)))


def make_plan():
    from cnn_graph_amd.plan import ChebPlan
    with np.load(os.path.join(GOLDEN, "golden_A.npz"), allow_pickle=False) as z:
        M = int(z["M"])
        Lt = scipy.sparse.csr_matrix((z["Lt_val"], z["Lt_col"], z["Lt_rowptr"]), shape=(M, M))
    return ChebPlan(Lt, device=0), M


class Draw:
    def __init__(self, dev, seed):
        import torch
        self.torch, self.dev, self.rng = torch, dev, np.random.default_rng(seed)

    def __call__(self, *shape, scale=0.3):
        a = self.rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)
        return self.torch.from_numpy(a).to(self.dev)

    def empty(self, *shape):
        """An output buffer, zero-filled: a digest of it cannot depend on stale memory."""
        return self.torch.zeros(shape, device=self.dev, dtype=self.torch.float32)

    def off4(self, *shape):
        """A contiguous tensor whose first element lies 4 bytes past a 16-byte boundary."""
        n = int(np.prod(shape))
        return self.empty(n + 1)[1:].view(shape)


def results(dev):
    """{case id: {output: digest}} on device ``dev``."""
    import torch

    from cnn_graph_amd import ops

    plan, M = make_plan()
    assert ops.lstm_hconv_supported(plan, H, K) and ops.lstm_seq_supported(plan, H, K)
    assert ops.lstm_seq_x_supported(plan, 2, H, K) and not ops.lstm_seq_x_supported(plan, 12, H, K)
    assert ops.flstm_supported(M, FH, 2)
    out = {}
    for N in (3, 4):
        d = Draw(dev, 100 + N)
        R = N * M
        tag = f"N{N}"
        Wh, bias = d(K * H, 4 * H), d(4 * H)
        gx, gh, c, h = d(N, M, 4 * H), d(N, M, 4 * H), d(N, M, H), d(N, M, H)
        dh, dh_rec, dc = d(N, M, H), d(N, M, H), d(N, M, H)

        # pointwise cell, allocated outputs / zero state into given outputs
        c1, h1, act = ops.lstm_cell_forward(gx, gh, bias, c, H)
        out[f"cell_forward_{tag}"] = digests(("c", "h", "act"), (c1, h1, act))
        oc, oh, oa = d.empty(N, M, H), d.empty(N, M, H), d.empty(N, M, 4 * H)
        r = ops.lstm_cell_forward(gx, None, None, None, H, "standard", out_c=oc, out_h=oh, out_act=oa)
        assert r[0] is oc and r[1] is oh and r[2] is oa
        out[f"cell_forward_zero_given_{tag}"] = digests(("c", "h", "act"), r)
        out[f"cell_backward_{tag}"] = digests(("dpre", "dc_prev"),
                                              ops.lstm_cell_backward(dh, dh_rec, dc, act, c, c1, H))
        od = d.empty(N, M, 4 * H)
        r = ops.lstm_cell_backward(dh, None, None, oa, None, oc, H, "standard", out_dpre=od,
                                   need_dc_prev=False)
        assert r[0] is od and r[1] is None
        out[f"cell_backward_zero_given_{tag}"] = digests(("dpre",), r[:1])

        # one-launch h step: planes given / no planes, zero c, given outputs
        planes = d.empty(K - 1, R, H)
        r = ops.lstm_hconv_step(plan, h, c, gx, Wh, bias, K, planes=planes, plane_stride=R * H)
        out[f"hconv_step_{tag}"] = digests(("c", "h", "act", "planes"), r + (planes,))
        act_h, c_h = r[2], r[0]
        r = ops.lstm_hconv_step(plan, h, None, gx, Wh, None, K, "standard", out_c=oc, out_h=oh,
                                out_act=oa)
        assert r[0] is oc and r[1] is oh and r[2] is oa
        out[f"hconv_step_zero_given_{tag}"] = digests(("c", "h", "act"), r)

        # one-launch BPTT step: gate-major act / unit-major act of the sequence launch
        r = ops.lstm_bwd_step(plan, dh, dh_rec, dc, act_h, c, c_h, Wh, K)
        out[f"bwd_step_{tag}"] = digests(("dpre", "dc_prev", "dh_prev"), r)

        # the sequence launches (feat_in 12: gx comes from outside; 2: fused in)
        gxs = d(T, N, M, 4 * H)
        acts = d.empty(T, N, M, 4 * H)
        hs, cs, a = ops.lstm_seq_forward(plan, gxs, Wh, bias, K, T, N, out_act=acts, check=True)
        assert a is acts
        out[f"seq_forward_zero_{tag}"] = digests(("hs", "cs", "act"), (hs, cs, a))
        ohs, ocs = d.empty(T, N, M, H), d.empty(T, N, M, H)
        pl = d.empty(K - 1, T * R, H)
        r = ops.lstm_seq_forward(plan, gxs, Wh, None, K, T, N, "standard", h0=h, c0=c, out_hs=ohs,
                                 out_cs=ocs, planes=pl, plane_stride=T * R * H, check=True)
        assert r[0] is ohs and r[1] is ocs and r[2] is None
        out[f"seq_forward_state_given_{tag}"] = digests(("hs", "cs", "planes"), (ohs, ocs, pl))
        r = ops.lstm_bwd_step(plan, dh, None, None, acts[T - 1], cs[T - 2], cs[T - 1], Wh, K,
                              out_dpre=od, out_dh_prev=oh, act_unit_major=True, need_dc_prev=False)
        assert r[0] is od and r[1] is None and r[2] is oh
        out[f"bwd_step_unit_major_given_{tag}"] = digests(("dpre", "dh_prev"), (od, oh))
        r = ops.lstm_bwd_step(plan, dh, None, dc, acts[0], None, cs[0], Wh, K, act_unit_major=True,
                              need_dh_prev=False)
        assert r[2] is None
        out[f"bwd_step_no_hconv_{tag}"] = digests(("dpre", "dc_prev"), r[:2])

        xs, Wx = d(T, N, M, 2), d(K * 2, 4 * H)
        r = ops.lstm_seq_forward_x(plan, xs, Wx, Wh, bias, K, out_act=acts, check=True)
        out[f"seq_forward_x_zero_{tag}"] = digests(("hs", "cs", "act", "xplanes"), r)
        xpl = d.empty(K, T * R, 2)
        r = ops.lstm_seq_forward_x(plan, xs, Wx, Wh, bias, K, "standard", h0=h, c0=c, out_hs=ohs,
                                   out_cs=ocs, xplanes=xpl, check=True)
        assert r[0] is ohs and r[1] is ocs and r[2] is None and r[3] is xpl
        out[f"seq_forward_x_state_given_{tag}"] = digests(("hs", "cs", "xplanes"), (ohs, ocs, xpl))

        # weight and bias gradients (feat_in 12 and 2)
        dpre = d(N, M, 4 * H)
        for Fin in (12, 2):
            basis, xp, hp = d(R, Fin * K), d(K, R, Fin), d(K, R, H)
            w = ops.weight_grad(basis, dpre)
            acc = ops.weight_grad(basis, dpre, out=w.clone(), accumulate=True)
            out[f"weight_grad_Fin{Fin}_{tag}"] = digests(("dW", "accumulated"), (w, acc))
            w = ops.weight_grad_planes(xp, R * Fin, K, R, dpre)
            acc = ops.weight_grad_planes(xp, R * Fin, K, R, dpre, out=w.clone(), accumulate=True)
            out[f"weight_grad_planes_Fin{Fin}_{tag}"] = digests(("dW", "accumulated"), (w, acc))
            out[f"lstm_weight_grads_Fin{Fin}_{tag}"] = digests(
                ("dWh", "dWx", "db"), ops.lstm_weight_grads(hp, R * H, xp, R * Fin, K, R, dpre))
        b = ops.bias_grad(dpre)
        acc = ops.bias_grad(dpre, out=b.clone(), accumulate=True)
        out[f"bias_grad_{tag}"] = digests(("db", "accumulated"), (b, acc))

        # bias + activation, forward and backward (with and without the bias gradient)
        for act_name in ("relu", "tanh"):
            x = d(N, M, 4 * H).requires_grad_()
            bb = d(4 * H).requires_grad_()
            y = ops.bias_act(x, bb, act_name)
            y.backward(dpre)
            out[f"bias_act_{act_name}_{tag}"] = digests(("y", "dx", "db"), (y, x.grad, bb.grad))
        x = d(N, M, 4 * H).requires_grad_()
        y = ops.bias_act(x, None, "relu")
        y.backward(dpre)
        out[f"bias_act_nobias_{tag}"] = digests(("y", "dx"), (y, x.grad))

        out[f"mse_loss_{tag}"] = digests(("loss", "dpred"), ops.mse_loss(gx, gh))
        out[f"mse_loss_nograd_{tag}"] = digests(("loss",), ops.mse_loss(gx, gh, need_grad=False)[:1])

        # Fourier gconv-LSTM step, H = 8
        U = d(M, M, scale=1.0) / M ** 0.5
        B = ops.gft_prepare(U)
        ghat, fWh, fb = d(N, M, 4 * FH), d(M, 4 * FH, FH), d(4 * FH)
        fh, fc = d(N, M, FH), d(N, M, FH)
        out[f"flstm_step_{tag}"] = digests(("c", "h", "act", "hhat"),
                                           ops.flstm_step(B, fh, fc, ghat, fWh, fb))
        fo = [d.empty(N, M, FH), d.empty(N, M, FH), d.empty(N, M, 4 * FH)]
        r = ops.flstm_step(B, None, None, ghat, None, None, "standard", out_c=fo[0], out_h=fo[1],
                           out_act=fo[2])
        assert r[0] is fo[0] and r[1] is fo[1] and r[2] is fo[2] and r[3] is None
        out[f"flstm_step_zero_given_{tag}"] = digests(("c", "h", "act"), r[:3])
    torch.cuda.synchronize()
    return out


def refusals(dev):
    """[(case id, thunk)]: each thunk calls an op with one bad argument and must
    raise from a Python-side check, before any launch."""
    import torch

    from cnn_graph_amd import ops

    plan, M = make_plan()
    d = Draw(dev, 7)
    N = 3
    R = N * M
    Wh, bias = d(K * H, 4 * H), d(4 * H)
    gx, gh, c, h = d(N, M, 4 * H), d(N, M, 4 * H), d(N, M, H), d(N, M, H)
    act = d(N, M, 4 * H)
    gxs, xs, Wx = d(T, N, M, 4 * H), d(T, N, M, 2), d(K * 2, 4 * H)
    dpre, basis, xp, hp = d(N, M, 4 * H), d(R, 12 * K), d(K, R, 12), d(K, R, H)
    B = ops.gft_prepare(d(M, M, scale=1.0) / M ** 0.5)
    ghat, fWh, fb, fh, fc = d(N, M, 4 * FH), d(M, 4 * FH, FH), d(4 * FH), d(N, M, FH), d(N, M, FH)
    f64 = torch.float64
    t_ = lambda x: x.transpose(0, 1)  # noqa: E731  (same elements, not contiguous)
    cases = [
        ("cell_forward/gx_dtype", lambda: ops.lstm_cell_forward(gx.to(f64), gh, bias, c, H)),
        ("cell_forward/gx_cpu", lambda: ops.lstm_cell_forward(gx.cpu(), gh, bias, c, H)),
        ("cell_forward/gh_noncontiguous", lambda: ops.lstm_cell_forward(gx, t_(gh), bias, c, H)),
        ("cell_forward/bias_count", lambda: ops.lstm_cell_forward(gx, gh, bias[:-1], c, H)),
        ("cell_forward/c_count", lambda: ops.lstm_cell_forward(gx, gh, bias, c[1:], H)),
        ("cell_forward/c_dtype", lambda: ops.lstm_cell_forward(gx, gh, bias, c.to(f64), H)),
        ("cell_forward/out_c_count", lambda: ops.lstm_cell_forward(gx, gh, bias, c, H, out_c=d.empty(R, H + 1))),
        ("cell_forward/out_act_dtype",
         lambda: ops.lstm_cell_forward(gx, gh, bias, c, H, out_act=act.to(f64))),
        ("cell_backward/act_dtype", lambda: ops.lstm_cell_backward(h, None, None, act.to(f64), c, c, H)),
        ("cell_backward/dh_count", lambda: ops.lstm_cell_backward(h[1:], None, None, act, c, c, H)),
        ("cell_backward/dc_noncontiguous", lambda: ops.lstm_cell_backward(h, None, t_(c), act, c, c, H)),
        ("cell_backward/out_dpre_count",
         lambda: ops.lstm_cell_backward(h, None, None, act, c, c, H, out_dpre=d.empty(R, H))),
        ("hconv_step/h_prev_dtype", lambda: ops.lstm_hconv_step(plan, h.to(f64), c, gx, Wh, bias, K)),
        ("hconv_step/gx_count", lambda: ops.lstm_hconv_step(plan, h, c, gx[1:], Wh, bias, K)),
        ("hconv_step/c_prev_noncontiguous", lambda: ops.lstm_hconv_step(plan, h, t_(c), gx, Wh, bias, K)),
        ("hconv_step/Wh_shape", lambda: ops.lstm_hconv_step(plan, h, c, gx, Wh[:-1], bias, K)),
        ("hconv_step/Wh_noncontiguous",
         lambda: ops.lstm_hconv_step(plan, h, c, gx, d(4 * H, K * H).t(), bias, K)),
        ("hconv_step/out_h_count", lambda: ops.lstm_hconv_step(plan, h, c, gx, Wh, bias, K, out_h=d.empty(R))),
        ("hconv_step/planes_storage", lambda: ops.lstm_hconv_step(
            plan, h, c, gx, Wh, bias, K, planes=d.empty(K - 1, R * H - 4), plane_stride=R * H)),
        ("hconv_step/planes_stride_short", lambda: ops.lstm_hconv_step(
            plan, h, c, gx, Wh, bias, K, planes=d.empty(K - 1, R * H), plane_stride=R * H - 4)),
        ("hconv_step/planes_misaligned", lambda: ops.lstm_hconv_step(
            plan, h, c, gx, Wh, bias, K, planes=d.off4(K - 1, R * H), plane_stride=R * H)),
        ("hconv_step/planes_stride_odd", lambda: ops.lstm_hconv_step(
            plan, h, c, gx, Wh, bias, K, planes=d.empty(K, R * H), plane_stride=R * H + 2)),
        ("seq_forward/gx_dtype", lambda: ops.lstm_seq_forward(plan, gxs.to(f64), Wh, bias, K, T, N)),
        ("seq_forward/gx_count", lambda: ops.lstm_seq_forward(plan, gxs[1:], Wh, bias, K, T, N)),
        ("seq_forward/Wh_shape", lambda: ops.lstm_seq_forward(plan, gxs, Wh[:-1], bias, K, T, N)),
        ("seq_forward/bias_misaligned", lambda: ops.lstm_seq_forward(plan, gxs, Wh, d.off4(4 * H), K, T, N)),
        ("seq_forward/bias_count", lambda: ops.lstm_seq_forward(plan, gxs, Wh, bias[:-4], K, T, N)),
        ("seq_forward/h0_count", lambda: ops.lstm_seq_forward(plan, gxs, Wh, bias, K, T, N, h0=h[1:], c0=c)),
        ("seq_forward/c0_dtype", lambda: ops.lstm_seq_forward(plan, gxs, Wh, bias, K, T, N, h0=h, c0=c.to(f64))),
        ("seq_forward/c0_misaligned",
         lambda: ops.lstm_seq_forward(plan, gxs, Wh, bias, K, T, N, h0=h, c0=d.off4(N, M, H))),
        ("seq_forward/out_hs_count",
         lambda: ops.lstm_seq_forward(plan, gxs, Wh, bias, K, T, N, out_hs=d.empty(T, R, H + 1))),
        ("seq_forward/out_act_count",
         lambda: ops.lstm_seq_forward(plan, gxs, Wh, bias, K, T, N, out_act=d.empty(T, R, H))),
        ("seq_forward/planes_storage", lambda: ops.lstm_seq_forward(
            plan, gxs, Wh, bias, K, T, N, planes=d.empty(K - 1, T * R * H - 4), plane_stride=T * R * H)),
        ("seq_forward/planes_misaligned", lambda: ops.lstm_seq_forward(
            plan, gxs, Wh, bias, K, T, N, planes=d.off4(K - 1, T * R * H), plane_stride=T * R * H)),
        ("seq_forward/planes_dtype", lambda: ops.lstm_seq_forward(
            plan, gxs, Wh, bias, K, T, N, planes=d.empty(K - 1, T * R * H).to(f64), plane_stride=T * R * H)),
        # K = 1 writes no plane: the wrapper leaves the pointer to the C entry (CGError)
        ("seq_forward/K1_planes_misaligned", lambda: ops.lstm_seq_forward(
            plan, gxs, d(H, 4 * H), bias, 1, T, N, planes=d.off4(4), plane_stride=0)),
        ("seq_forward_x/K1_planes_misaligned", lambda: ops.lstm_seq_forward_x(
            plan, xs, d(2, 4 * H), d(H, 4 * H), bias, 1, planes=d.off4(4), plane_stride=0)),
        ("seq_forward_x/xs_dtype", lambda: ops.lstm_seq_forward_x(plan, xs.to(f64), Wx, Wh, bias, K)),
        ("seq_forward_x/Wx_shape", lambda: ops.lstm_seq_forward_x(plan, xs, Wx[:-1], Wh, bias, K)),
        ("seq_forward_x/Wh_noncontiguous",
         lambda: ops.lstm_seq_forward_x(plan, xs, Wx, d(4 * H, K * H).t(), bias, K)),
        ("seq_forward_x/h0_misaligned",
         lambda: ops.lstm_seq_forward_x(plan, xs, Wx, Wh, bias, K, h0=d.off4(N, M, H), c0=c)),
        ("seq_forward_x/xplanes_count",
         lambda: ops.lstm_seq_forward_x(plan, xs, Wx, Wh, bias, K, xplanes=d.empty(K, T * R))),
        ("bwd_step/act_dtype", lambda: ops.lstm_bwd_step(plan, h, None, None, act.to(f64), c, c, Wh, K)),
        ("bwd_step/dh_misaligned",
         lambda: ops.lstm_bwd_step(plan, d.off4(N, M, H), None, None, act, c, c, Wh, K)),
        ("bwd_step/dc_count", lambda: ops.lstm_bwd_step(plan, h, None, c[1:], act, c, c, Wh, K)),
        ("bwd_step/c_prev_noncontiguous", lambda: ops.lstm_bwd_step(plan, h, None, None, act, t_(c), c, Wh, K)),
        ("bwd_step/act_misaligned",
         lambda: ops.lstm_bwd_step(plan, h, None, None, d.off4(N, M, 4 * H), c, c, Wh, K)),
        ("bwd_step/act_noncontiguous",
         lambda: ops.lstm_bwd_step(plan, h, None, None, d(M, N, 4 * H).transpose(0, 1), c, c, Wh, K)),
        ("bwd_step/Wh_shape", lambda: ops.lstm_bwd_step(plan, h, None, None, act, c, c, Wh[:-1], K)),
        ("bwd_step/out_dpre_count",
         lambda: ops.lstm_bwd_step(plan, h, None, None, act, c, c, Wh, K, out_dpre=d.empty(R, H))),
        ("bwd_step/out_dh_prev_dtype",
         lambda: ops.lstm_bwd_step(plan, h, None, None, act, c, c, Wh, K, out_dh_prev=h.to(f64))),
        ("weight_grad/basis_dtype", lambda: ops.weight_grad(basis.to(f64), dpre)),
        ("weight_grad/dy_count", lambda: ops.weight_grad(basis, dpre[1:])),
        ("weight_grad/accumulate_without_out", lambda: ops.weight_grad(basis, dpre, accumulate=True)),
        ("weight_grad/out_count", lambda: ops.weight_grad(basis, dpre, out=d.empty(12 * K, 4 * H + 1))),
        ("weight_grad_planes/planes_dtype",
         lambda: ops.weight_grad_planes(xp.to(f64), R * 12, K, R, dpre)),
        ("weight_grad_planes/dy_noncontiguous",
         lambda: ops.weight_grad_planes(xp, R * 12, K, R, d(4 * H, R).t())),
        ("weight_grad_planes/storage",
         lambda: ops.weight_grad_planes(d.empty(K * R - 1, 12), R * 12, K, R, dpre)),
        ("weight_grad_planes/stride_short", lambda: ops.weight_grad_planes(xp, R * 12 - 1, K, R, dpre)),
        ("weight_grad_planes/accumulate_without_out",
         lambda: ops.weight_grad_planes(xp, R * 12, K, R, dpre, accumulate=True)),
        ("weight_grad_planes/out_count",
         lambda: ops.weight_grad_planes(xp, R * 12, K, R, dpre, out=d.empty(12 * K, H))),
        ("lstm_weight_grads/dpre_dtype",
         lambda: ops.lstm_weight_grads(hp, R * H, xp, R * 12, K, R, dpre.to(f64))),
        ("lstm_weight_grads/dpre_count", lambda: ops.lstm_weight_grads(hp, R * H, xp, R * 12, K, R, dpre[1:])),
        ("lstm_weight_grads/h_planes_storage",
         lambda: ops.lstm_weight_grads(d.empty(K * R - 1, H), R * H, xp, R * 12, K, R, dpre)),
        ("lstm_weight_grads/x_planes_stride_short",
         lambda: ops.lstm_weight_grads(hp, R * H, xp, R * 12 - 1, K, R, dpre)),
        ("bias_grad/dy_dtype", lambda: ops.bias_grad(dpre.to(f64))),
        ("bias_grad/accumulate_without_out", lambda: ops.bias_grad(dpre, accumulate=True)),
        ("bias_grad/out_count", lambda: ops.bias_grad(dpre, out=d.empty(4 * H + 1))),
        ("bias_act/x_dtype", lambda: ops.bias_act(dpre.to(f64), bias)),
        ("bias_act/x_cpu", lambda: ops.bias_act(dpre.cpu(), bias)),
        ("bias_act/bias_does_not_tile", lambda: ops.bias_act(dpre, d(4 * H - 1))),
        ("mse_loss/labels_dtype", lambda: ops.mse_loss(gx, gh.to(f64))),
        ("mse_loss/sizes_differ", lambda: ops.mse_loss(gx, gh[1:])),
        ("flstm_step/ghat_x_dtype", lambda: ops.flstm_step(B, fh, fc, ghat.to(f64), fWh, fb)),
        ("flstm_step/h_prev_count", lambda: ops.flstm_step(B, fh[1:], fc, ghat, fWh, fb)),
        ("flstm_step/c_prev_noncontiguous", lambda: ops.flstm_step(B, fh, t_(fc), ghat, fWh, fb)),
        ("flstm_step/Wh_count", lambda: ops.flstm_step(B, fh, fc, ghat, fWh[1:], fb)),
        ("flstm_step/bias_count", lambda: ops.flstm_step(B, fh, fc, ghat, fWh, fb[1:])),
        ("flstm_step/out_c_count", lambda: ops.flstm_step(B, fh, fc, ghat, fWh, fb, out_c=d.empty(R, FH + 1))),
        ("flstm_step/out_hhat_dtype",
         lambda: ops.flstm_step(B, fh, fc, ghat, fWh, fb, out_hhat=fh.to(f64))),
    ]
    return cases


def refused(dev):
    """{case id: {"type": exception class name, "message": text}}; a case that
    does not raise is a bug in this table."""
    out = {}
    for name, thunk in refusals(dev):
        try:
            thunk()
        except (ValueError, TypeError, RuntimeError) as e:  # (CGError is a RuntimeError)
            out[name] = {"type": type(e).__name__, "message": str(e)}
        else:
            raise AssertionError(f"{name}: the call was not refused")
    return out


def abi_refused(dev):
    """{case id: {"status", "message"}} of the plan-taking C entries' refusals
    that need a plan (so a device): alignment, aliasing, strides, workspace and
    unsupported sizes.  Real tensors throughout; every call is refused by an
    argument check before any launch."""
    import ctypes

    from cnn_graph_amd import _lib

    plan, M = make_plan()
    lib, hd = _lib.lib(), plan.handle
    d = Draw(dev, 9)
    N = 3
    R = N * M
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    Wh, bias, Wx = d(K * H, 4 * H), d(4 * H), d(K * 2, 4 * H)
    gx, c, h, act = d(N, M, 4 * H), d(N, M, H), d(N, M, H), d(N, M, 4 * H)
    oc, oh, oa, od = d.empty(N, M, H), d.empty(N, M, H), d.empty(N, M, 4 * H), d.empty(N, M, 4 * H)
    pl = d.empty(K - 1, R, H)
    gxs, xs = d(T, N, M, 4 * H), d(T, N, M, 2)
    hs, cs, spl, xpl = d.empty(T, N, M, H), d.empty(T, N, M, H), d.empty(K - 1, T * R, H), d.empty(K, T * R, 2)
    nb = ctypes.c_size_t()
    _lib.call("cg_lstm_seq_workspace_bytes", hd, N, ctypes.byref(nb))
    ws = d.torch.empty(max(nb.value, 1), device=dev, dtype=d.torch.uint8)

    def hstep(h_prev=h, c_prev=c, c_out=oc, planes=pl, stride=R * H, Hh=H):
        return lib.cg_lstm_hconv_step(hd, N, Hh, K, 0, p(h_prev), p(c_prev), p(gx), p(Wh), p(bias), p(c_out),
                                      p(oh), p(oa), p(planes), stride, None)

    def seq(bias_=bias, h0=None, hs_=hs, planes=spl, stride=T * R * H, nbytes=None, Hh=H):
        return lib.cg_lstm_seq_forward(hd, T, N, Hh, K, 0, p(gxs), p(Wh), p(bias_), p(h0), None, p(hs_), p(cs),
                                       None, p(planes), stride, p(ws), nb.value if nbytes is None else nbytes,
                                       None)

    def seqx(Fin=2, xstride=T * R * 2):
        return lib.cg_lstm_seq_forward_x(hd, T, N, Fin, H, K, 0, p(xs), p(Wx), p(xpl), xstride, p(Wh), p(bias),
                                         None, None, p(hs), p(cs), None, p(spl), T * R * H, p(ws), nb.value,
                                         None)

    def bstep(dh=h, dpre=od, Kk=K):
        return lib.cg_lstm_bwd_step(hd, N, H, Kk, 0, p(dh), None, None, p(act), 0, p(c), p(c), p(Wh), p(dpre),
                                    None, p(oh), None)

    # workspaces one byte short: the Chebyshev forward on the streaming path, the
    # backward, and the bias gradient of bias_act (refused after its dz launch)
    from cnn_graph_amd.plan import ChebPlan
    splan = ChebPlan(scipy.sparse.csr_matrix((plan.val, plan.col, plan.rowptr), shape=(M, M)), device=0,
                     path="stream")
    Fin, Fout = 12, 32
    fwd, bwd = splan.workspace_bytes(N, Fin, K, Fout)
    assert fwd > 0 and bwd > 0
    x, W, dy = d(N, M, Fin), d(Fin * K, Fout), d(N, M, Fout)
    basis, y, dx, dW = d.empty(R, Fin * K), d.empty(N, M, Fout), d.empty(N, M, Fin), d.empty(Fin * K, Fout)
    cws = d.torch.zeros(max(fwd, bwd), device=dev, dtype=d.torch.uint8)
    db, ba = d.empty(4 * H), ctypes.c_size_t()
    _lib.call("cg_bias_act_workspace_bytes", R * 4 * H, 4 * H, ctypes.byref(ba))
    rows = [
        ("cheb_forward/stream_workspace_small", lambda: lib.cg_cheb_forward(
            splan.handle, N, Fin, K, Fout, p(x), p(W), p(basis), p(y), p(cws), fwd - 1, None)),
        ("cheb_backward/workspace_small", lambda: lib.cg_cheb_backward(
            splan.handle, N, Fin, K, Fout, p(dy), p(basis), p(W), p(dx), p(dW), p(cws), bwd - 1, None)),
        ("bias_act_backward/workspace_small", lambda: lib.cg_bias_act_backward(
            R * 4 * H, 4 * H, p(gx), p(act), 1, p(oa), p(db), 0, p(cws), ba.value - 1, None)),
        ("lstm_hconv_step/h_prev_misaligned", lambda: hstep(h_prev=d.off4(N, M, H))),
        ("lstm_hconv_step/planes_misaligned", lambda: hstep(planes=d.off4(K - 1, R, H))),
        ("lstm_hconv_step/stride_odd", lambda: hstep(planes=d.empty(K, R, H), stride=R * H + 2)),
        ("lstm_hconv_step/stride_short", lambda: hstep(stride=R * H - 4)),
        ("lstm_hconv_step/c_out_is_c_prev", lambda: hstep(c_out=c)),
        ("lstm_hconv_step/H_16", lambda: hstep(Hh=16)),
        ("lstm_seq_forward/no_planes", lambda: seq(planes=None)),
        ("lstm_seq_forward/stride_short", lambda: seq(stride=T * R * H - 4)),
        ("lstm_seq_forward/bias_misaligned", lambda: seq(bias_=d.off4(4 * H))),
        ("lstm_seq_forward/hs_is_h0", lambda: seq(h0=hs)),
        ("lstm_seq_forward/workspace_small", lambda: seq(nbytes=nb.value - 1)),
        ("lstm_seq_forward/H_16", lambda: seq(Hh=16)),
        ("lstm_seq_forward_x/feat_in_9", lambda: seqx(Fin=9)),
        ("lstm_seq_forward_x/x_stride_short", lambda: seqx(xstride=T * R * 2 - 1)),
        ("lstm_bwd_step/dh_misaligned", lambda: bstep(dh=d.off4(N, M, H))),
        ("lstm_bwd_step/dpre_is_act", lambda: bstep(dpre=act)),
        ("lstm_bwd_step/K_5", lambda: bstep(Kk=5)),
    ]
    out = {}
    for name, thunk in rows:
        st = thunk()
        if st not in (_lib.CG_ERR_ARG, _lib.CG_ERR_UNSUPPORTED):
            raise AssertionError(f"{name}: not refused by an argument check (status {st})")
        out[name] = {"status": int(st), "message": lib.cg_last_error().decode()}
    return out
