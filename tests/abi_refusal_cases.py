"""The table behind tests/golden/abi_refusals.json: calls that the C entries of
cheb_abi.cpp / fourier_abi.cpp refuse before any HIP call, with the status and
the cg_last_error() text of each.

scripts/record_abi_refusals.py records it, tests/test_abi_refusals_cpu.py
replays it.  No GPU: the pointers are plain integers (16-byte aligned and
distinct unless the case is about alignment or aliasing) and are never memory.
Every case must be refused by an argument check; the entries that take a plan
are reached with a null plan only (a plan needs a device), so their alignment
and aliasing refusals are pinned on the GPU by tests/test_gpu_ops_pinned.py."""
import ctypes

from cnn_graph_amd import _lib

P = [4096 * k for k in range(1, 16)]  # fake device pointers
ODD = P[14] + 4                        # not 16-byte aligned
BIG = 1 << 40                          # a workspace size that is always enough


def size(entry, *args, n=1):
    """The byte count(s) a cg_*_workspace_bytes entry reports."""
    out = [ctypes.c_size_t() for _ in range(n)]
    st = getattr(_lib.lib(), entry)(*args, *(ctypes.byref(o) for o in out))
    assert st == _lib.CG_OK, (entry, args, _lib.lib().cg_last_error().decode())
    return out[0].value if n == 1 else tuple(o.value for o in out)


def cases():
    """[(case id, entry, args)]"""
    a, b, c, d, e, f, g, h, i, j, k, ws = P[:12]
    adam = (1e-3, 0.9, 0.999, 1e-8)
    mse = size("cg_mse_loss_workspace_bytes", 10)
    sx = size("cg_seq_xent_workspace_bytes", 3, 2, 100, 32)
    wg = size("cg_weight_grad_workspace_bytes", 300, 36, 128)
    lwg = size("cg_lstm_weight_grads_workspace_bytes", 300, 32, 2, 3)
    bg = size("cg_bias_grad_workspace_bytes", 300, 128)
    ff, fb = size("cg_fourier_workspace_bytes", 3, 100, 4, 8, n=2)
    gb = size("cg_gft_workspace_bytes", 100)
    fl = size("cg_flstm_workspace_bytes", 3, 100, 8)
    rf, rb = size("cg_fres_workspace_bytes", 3, 100, 4, 8, n=2)
    fwd_adam = lambda W, gr, m, v, st, Wo, mo, vo, y: (  # noqa: E731
        "cg_cheb_forward_adam", (None, 1, 1, 2, 1, a, W, gr, m, v, *adam, st, 1.0, Wo, mo, vo, 0, None, y,
                                 None, 0, None))
    bwd_adam = lambda W, dW, m, v, st: (  # noqa: E731
        (None, 1, 1, 2, 1, a, b, W, None, dW, m, v, *adam, st, 1.0, None, 0, None))
    seq = lambda plan, gx, gates=0: (  # noqa: E731
        plan, 3, 3, 32, 3, gates, gx, b, None, None, None, c, d, None, e, 3 * 300 * 32, ws, BIG, None)
    flstm = lambda **kw: _flstm(gb, fl, **kw)  # noqa: E731
    rows = [
        ("mse_loss/null_pred", "cg_mse_loss", (None, b, 10, c, None, ws, BIG, None)),
        ("mse_loss/n_0", "cg_mse_loss", (a, b, 0, c, None, ws, BIG, None)),
        ("mse_loss/workspace_small", "cg_mse_loss", (a, b, 10, c, None, ws, mse - 1, None)),
        ("mse_loss/workspace_null", "cg_mse_loss", (a, b, 10, c, None, None, mse, None)),
        ("mse_loss_workspace_bytes/n_0", "cg_mse_loss_workspace_bytes", (0, None)),
        ("mse_loss_ema/null_ema", "cg_mse_loss_ema", (a, b, 10, c, None, None, 0.9, ws, BIG, None)),
        ("mse_loss_ema/decay", "cg_mse_loss_ema", (a, b, 10, c, None, d, 1.5, ws, BIG, None)),
        ("mse_loss_ema/workspace_small", "cg_mse_loss_ema", (a, b, 10, c, None, d, 0.9, ws, mse - 1, None)),
        ("dropout_forward/null", "cg_dropout_forward", (None, 10, 0.5, 1, b, None)),
        ("dropout_forward/keep", "cg_dropout_forward", (a, 10, 0.0, 1, b, None)),
        ("dropout_backward/keep", "cg_dropout_backward", (a, 10, 1.5, 1, b, None)),
        ("clip_by_norm/null", "cg_clip_by_norm", (None, 10, 1.0, None, None)),
        ("clip_by_norm/clip_0", "cg_clip_by_norm", (a, 10, 0.0, None, None)),
        ("seq_xent_workspace_bytes/T_0", "cg_seq_xent_workspace_bytes", (0, 2, 100, 32, None)),
        ("seq_xent_workspace_bytes/H_300", "cg_seq_xent_workspace_bytes",
         (3, 2, 100, 300, ctypes.byref(ctypes.c_size_t()))),
        ("seq_xent_head/null_hs", "cg_seq_xent_head",
         (None, b, c, d, 3, 2, 100, 32, 1.0, 0, 1.0, None, None, e, None, None, None, ws, BIG, None)),
        ("seq_xent_head/dhs_without_dw", "cg_seq_xent_head",
         (a, b, c, d, 3, 2, 100, 32, 1.0, 0, 1.0, None, None, e, f, None, None, ws, BIG, None)),
        ("seq_xent_head/M_0", "cg_seq_xent_head",
         (a, b, c, d, 3, 2, 0, 32, 1.0, 0, 1.0, None, None, e, None, None, None, ws, BIG, None)),
        ("seq_xent_head/keep", "cg_seq_xent_head",
         (a, b, c, d, 3, 2, 100, 32, 0.0, 0, 1.0, None, None, e, None, None, None, ws, BIG, None)),
        ("seq_xent_head/H_300", "cg_seq_xent_head",
         (a, b, c, d, 3, 2, 100, 300, 1.0, 0, 1.0, None, None, e, None, None, None, ws, BIG, None)),
        ("seq_xent_head/workspace_small", "cg_seq_xent_head",
         (a, b, c, d, 3, 2, 100, 32, 1.0, 0, 1.0, None, None, e, None, None, None, ws, sx - 1, None)),
        ("slice_channels/range", "cg_slice_channels", (a, 10, 16, 12, 17, b, None)),
        ("stack_merge_forward/alias", "cg_stack_merge_forward", (2, 10, 2, a, b, 0, a, None)),
        ("stack_merge_forward/null", "cg_stack_merge_forward", (2, 10, 2, a, None, 0, c, None)),
        ("stack_merge_backward/nothing", "cg_stack_merge_backward", (2, 10, 2, a, b, c, None, None, None)),
        ("stack_merge_backward/alias", "cg_stack_merge_backward", (2, 10, 2, a, b, c, a, None, None)),
        ("weight_grad_workspace_bytes/R_0", "cg_weight_grad_workspace_bytes", (0, 36, 128, None)),
        ("weight_grad/null", "cg_weight_grad", (300, 36, 128, None, b, c, 0, ws, BIG, None)),
        ("weight_grad/R_0", "cg_weight_grad", (0, 36, 128, a, b, c, 0, ws, BIG, None)),
        ("weight_grad/workspace_small", "cg_weight_grad", (300, 36, 128, a, b, c, 0, ws, wg - 1, None)),
        ("weight_grad/workspace_null", "cg_weight_grad", (300, 36, 128, a, b, c, 0, None, wg, None)),
        ("weight_grad_planes/stride_short", "cg_weight_grad_planes",
         (300, 12, 3, 128, a, 300 * 12 - 1, b, c, 0, ws, BIG, None)),
        ("weight_grad_planes/workspace_small", "cg_weight_grad_planes",
         (300, 12, 3, 128, a, 300 * 12, b, c, 0, ws, wg - 1, None)),
        ("lstm_weight_grads_workspace_bytes/K_0", "cg_lstm_weight_grads_workspace_bytes",
         (300, 32, 2, 0, None)),
        ("lstm_weight_grads/null_db", "cg_lstm_weight_grads",
         (300, 32, 2, 3, a, 300 * 32, b, 300 * 2, c, d, e, None, ws, BIG, None)),
        ("lstm_weight_grads/h_stride_short", "cg_lstm_weight_grads",
         (300, 32, 2, 3, a, 300 * 32 - 1, b, 300 * 2, c, d, e, f, ws, BIG, None)),
        ("lstm_weight_grads/H_128", "cg_lstm_weight_grads",
         (300, 128, 2, 3, a, 300 * 128, b, 300 * 2, c, d, e, f, ws, BIG, None)),
        ("lstm_weight_grads/FinK_66", "cg_lstm_weight_grads",
         (300, 32, 22, 3, a, 300 * 32, b, 300 * 22, c, d, e, f, ws, BIG, None)),
        ("lstm_weight_grads/workspace_small", "cg_lstm_weight_grads",
         (300, 32, 2, 3, a, 300 * 32, b, 300 * 2, c, d, e, f, ws, lwg - 1, None)),
        ("bias_grad_workspace_bytes/C_0", "cg_bias_grad_workspace_bytes", (300, 0, None)),
        ("bias_grad/null", "cg_bias_grad", (300, 128, None, b, 0, ws, BIG, None)),
        ("bias_grad/workspace_small", "cg_bias_grad", (300, 128, a, b, 0, ws, bg - 1, None)),
        ("bias_act_forward/null", "cg_bias_act_forward", (1280, 128, None, b, 1, c, None)),
        ("bias_act_forward/act", "cg_bias_act_forward", (1280, 128, a, b, 9, c, None)),
        ("bias_act_forward/bias_len", "cg_bias_act_forward", (1280, 127, a, b, 1, c, None)),
        ("bias_act_workspace_bytes/bias_len", "cg_bias_act_workspace_bytes", (1280, 127, None)),
        ("bias_act_backward/null", "cg_bias_act_backward", (1280, 128, None, b, 1, c, d, 0, ws, BIG, None)),
        ("bias_act_backward/act", "cg_bias_act_backward", (1280, 128, a, b, 9, c, d, 0, ws, BIG, None)),
        ("bias_act_backward/relu_without_y", "cg_bias_act_backward",
         (1280, 128, a, None, 1, c, d, 0, ws, BIG, None)),
        ("gemm_f32/null", "cg_gemm_f32", (0, 0, 4, 4, 4, None, 4, b, 4, c, 4, None)),
        ("gemm_f32/lda", "cg_gemm_f32", (0, 0, 4, 4, 4, a, 3, b, 4, c, 4, None)),
        ("gemm_f32/grid", "cg_gemm_f32", (0, 0, 4, 1 << 23, 4, a, 4, b, 1 << 23, c, 1 << 23, None)),
        ("lstm_cell_forward/gates", "cg_lstm_cell_forward", (4, 2, 7, a, None, None, None, b, c, None, None)),
        ("lstm_cell_forward/null", "cg_lstm_cell_forward", (4, 2, 0, None, None, None, None, b, c, None, None)),
        ("lstm_cell_forward/2^31", "cg_lstm_cell_forward", (1 << 30, 8, 0, a, None, None, None, b, c, None, None)),
        ("lstm_cell_forward/R_0", "cg_lstm_cell_forward", (0, 8, 0, a, None, None, None, b, c, None, None)),
        ("lstm_cell_backward/null", "cg_lstm_cell_backward",
         (4, 2, 0, None, None, None, None, None, b, c, None, None)),
        ("lstm_hconv_supported/null", "cg_lstm_hconv_supported", (None, 32, 3, None)),
        ("lstm_seq_supported/null", "cg_lstm_seq_supported", (None, 32, 3, None)),
        ("lstm_seq_x_supported/null", "cg_lstm_seq_x_supported", (None, 2, 32, 3, None)),
        ("lstm_seq_workspace_bytes/null", "cg_lstm_seq_workspace_bytes", (None, 3, None)),
        ("lstm_hconv_step/null_plan", "cg_lstm_hconv_step",
         (None, 3, 32, 3, 0, a, b, c, d, None, e, f, g, None, 0, None)),
        ("lstm_hconv_step/gates", "cg_lstm_hconv_step",
         (None, 3, 32, 3, 5, a, b, c, d, None, e, f, g, None, 0, None)),
        ("lstm_seq_forward/null_plan", "cg_lstm_seq_forward", seq(None, a)),
        ("lstm_seq_forward/gates", "cg_lstm_seq_forward", seq(None, a, 5)),
        ("lstm_seq_forward_x/null_xs", "cg_lstm_seq_forward_x",
         (None, 3, 3, 2, 32, 3, 0, None, a, b, 900 * 2, c, None, None, None, d, e, None, f, 900 * 32, ws, BIG,
          None)),
        ("lstm_seq_forward_x/null_plan", "cg_lstm_seq_forward_x",
         (None, 3, 3, 2, 32, 3, 0, g, a, b, 900 * 2, c, None, None, None, d, e, None, f, 900 * 32, ws, BIG,
          None)),
        ("lstm_seq_fault/null", "cg_lstm_seq_fault", (None, 1, 1, None)),
        ("lstm_seq_status/null", "cg_lstm_seq_status", (None, 3, None, None, None)),
        ("plan_set_seq_fault_test/null", "cg_plan_set_seq_fault_test", (None, 1)),
        ("lstm_bwd_step/null_plan", "cg_lstm_bwd_step",
         (None, 3, 32, 3, 0, a, None, None, b, 0, c, d, e, f, None, g, None)),
        ("lstm_bwd_step/H_0", "cg_lstm_bwd_step",
         (None, 3, 0, 3, 0, a, None, None, b, 0, c, d, e, f, None, g, None)),
        ("perm_gather/null", "cg_perm_gather", (a, None, 2, 10, 12, 1, b, None)),
        ("maxpool_forward/M_mod_p", "cg_maxpool_forward", (a, 1, 6, 1, 4, b, c, None)),
        ("maxpool_backward/null", "cg_maxpool_backward", (a, None, 1, 8, 1, 4, b, None)),
        ("avgpool_forward/M_mod_p", "cg_avgpool_forward", (a, 1, 6, 1, 4, b, None)),
        ("avgpool_backward/null", "cg_avgpool_backward", (None, 1, 8, 1, 4, b, None)),
        ("adam_update/null", "cg_adam_update", (None, b, c, d, 4, *adam, 1, 1.0, None)),
        ("adam_update/step_0", "cg_adam_update", (a, b, c, d, 4, *adam, 0, 1.0, None)),
        ("sgd_update/null", "cg_sgd_update", (None, b, 4, 0.1, 1.0, None)),
        ("rmsprop_update/eps_0", "cg_rmsprop_update", (a, b, c, d, 4, 0.1, 0.9, 0.0, 0.0, 1.0, None)),
        ("cheb_forward/null_plan", "cg_cheb_forward", (None, 1, 1, 2, 1, a, b, c, d, ws, BIG, None)),
        ("cheb_backward/null_plan", "cg_cheb_backward", (None, 1, 1, 2, 1, a, b, c, d, e, ws, BIG, None)),
        ("cheb_backward_ex/act", "cg_cheb_backward_ex",
         (None, 1, 1, 2, 1, a, b, 7, c, d, e, 0, f, g, ws, BIG, None)),
        ("cheb_backward_layout/null_plan", "cg_cheb_backward_layout",
         (None, 1, 1, 2, 1, a, b, 0, 0, c, d, e, 0, f, g, ws, BIG, None)),
        ("cheb_workspace_bytes/null_plan", "cg_cheb_workspace_bytes", (None, 1, 1, 2, 1, None, None)),
        ("cheb_basis_elems/null_plan", "cg_cheb_basis_elems", (None, 1, 1, 2, 1, 0, None)),
        ("plan_query_path/null_plan", "cg_plan_query_path", (None, 1, 1, 2, 1, None)),
        ("plan_set_path/null_plan", "cg_plan_set_path", (None, 0)),
        ("plan_set_variant/null_plan", "cg_plan_set_variant", (None, 0)),
        ("cheb_forward_adam/null_grad",) + fwd_adam(b, None, d, e, 1, f, g, h, i),
        ("cheb_forward_adam/step_0",) + fwd_adam(b, c, d, e, 0, f, g, h, i),
        ("cheb_forward_adam/W_out_is_W",) + fwd_adam(b, c, d, e, 1, b, g, h, i),
        ("cheb_forward_adam/v_out_is_grad",) + fwd_adam(b, c, d, e, 1, f, g, c, i),
        ("cheb_forward_adam/m_out_is_v_out",) + fwd_adam(b, c, d, e, 1, f, g, g, i),
        ("cheb_forward_adam/null_plan",) + fwd_adam(b, c, d, e, 1, f, g, h, i),
        ("cheb_backward_adam/null_m", "cg_cheb_backward_adam", bwd_adam(c, d, None, f, 1)),
        ("cheb_backward_adam/step_0", "cg_cheb_backward_adam", bwd_adam(c, d, e, f, 0)),
        ("cheb_backward_adam/dW_is_W", "cg_cheb_backward_adam", bwd_adam(c, c, e, f, 1)),
        ("cheb_backward_adam/m_is_v", "cg_cheb_backward_adam", bwd_adam(c, d, e, e, 1)),
        ("cheb_backward_adam/null_plan", "cg_cheb_backward_adam", bwd_adam(c, d, e, f, 1)),
        ("cheb_backward_adam_layout/W_is_v", "cg_cheb_backward_adam_layout",
         (None, 1, 1, 2, 1, 0, a, b, c, None, d, e, c, *adam, 1, 1.0, None, 0, None)),
        # the Fourier family
        ("fourier_workspace_bytes/N_0", "cg_fourier_workspace_bytes", (0, 100, 4, 8, None, None)),
        ("fourier_forward/null", "cg_fourier_forward", (3, 100, 4, 8, a, b, None, d, e, ws, BIG, None)),
        ("fourier_forward/N_65536", "cg_fourier_forward", (65536, 100, 4, 8, a, b, c, d, e, ws, BIG, None)),
        ("fourier_forward/workspace_small", "cg_fourier_forward",
         (3, 100, 4, 8, a, b, c, d, e, ws, ff - 1, None)),
        ("fourier_forward/workspace_null", "cg_fourier_forward",
         (3, 100, 4, 8, a, b, c, d, e, None, ff, None)),
        ("fourier_backward/null", "cg_fourier_backward", (3, 100, 4, 8, a, b, c, None, e, f, ws, BIG, None)),
        ("fourier_backward/workspace_small", "cg_fourier_backward",
         (3, 100, 4, 8, a, b, c, d, e, f, ws, fb - 1, None)),
        ("gft_workspace_bytes/M_0", "cg_gft_workspace_bytes", (0, None)),
        ("gft_prepare/null_U", "cg_gft_prepare", (100, None, b, gb, None)),
        ("gft_prepare/basis_small", "cg_gft_prepare", (100, a, b, gb - 1, None)),
        ("gft_prepare/basis_misaligned", "cg_gft_prepare", (100, a, ODD, gb, None)),
        ("gft/null_basis", "cg_gft", (0, 3, 100, 8, None, gb, b, c, None)),
        ("gft/in_is_out", "cg_gft", (0, 3, 100, 8, a, gb, b, b, None)),
        ("gft/2^31", "cg_gft", (0, 1 << 15, 1 << 10, 1 << 6, a, BIG, b, c, None)),
        ("fourier_mix/form", "cg_fourier_mix", (3, 3, 100, 4, 8, a, b, c, None, d, None)),
        ("fourier_mix/Cin_0", "cg_fourier_mix", (0, 3, 100, 0, 8, a, b, None, None, d, None)),
        ("fourier_mix/2^31", "cg_fourier_mix", (0, 1 << 20, 1 << 10, 4, 8, a, b, None, None, d, None)),
        ("fourier_mix/null_g", "cg_fourier_mix", (1, 3, 100, 4, 8, a, None, None, None, d, None)),
        ("fourier_mix/add_with_form_1", "cg_fourier_mix", (1, 3, 100, 4, 8, a, None, c, e, d, None)),
        ("flstm_supported/null", "cg_flstm_supported", (100, 8, 2, None)),
        ("flstm_supported/H_0", "cg_flstm_supported", (100, 0, 2, ctypes.byref(ctypes.c_int32()))),
        ("flstm_workspace_bytes/N_0", "cg_flstm_workspace_bytes", (0, 100, 8, None)),
        ("flstm_step/N_0", "cg_flstm_step", flstm(N=0)),
        ("flstm_step/H_12", "cg_flstm_step", flstm(H=12)),
        ("flstm_step/gates", "cg_flstm_step", flstm(gates=5)),
        ("flstm_step/basis_small", "cg_flstm_step", flstm(nb=gb - 1)),
        ("flstm_step/basis_misaligned", "cg_flstm_step", flstm(basis=ODD)),
        ("flstm_step/null_h_out", "cg_flstm_step", flstm(h_out=None)),
        ("flstm_step/h_prev_without_hhat", "cg_flstm_step", flstm(hhat=None)),
        ("flstm_step/workspace_small", "cg_flstm_step", flstm(n=fl - 1)),
        ("flstm_step/workspace_null", "cg_flstm_step", flstm(ws=None)),
        ("fres_forward/workspace_small", "cg_fres_forward",
         (3, 100, 4, 8, a, gb, b, c, None, 0, d, e, ws, rf - 1, None)),
        ("fres_backward/workspace_small", "cg_fres_backward",
         (3, 100, 4, 8, a, gb, b, c, d, None, 0, None, e, 0, f, ws, rb - 1, None)),
    ]
    return rows


def _flstm(gb, fl, N=3, H=8, gates=0, basis=P[0], nb=None, h_out=P[7], hhat=P[9], ws=P[11], n=None):
    return (N, 100, H, gates, basis, gb if nb is None else nb, P[1], P[2], P[3], P[4], P[5], P[6], h_out,
            P[8], hhat, ws, fl if n is None else n, None)


def run():
    """{case id: {"entry", "status", "message"}}"""
    h = _lib.lib()
    out = {}
    for name, entry, args in cases():
        st = getattr(h, entry)(*args)
        assert name not in out, name
        out[name] = {"entry": entry, "status": int(st), "message": h.cg_last_error().decode()}
    return out
