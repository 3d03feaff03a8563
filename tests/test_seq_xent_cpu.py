"""The float64 reference of the gconvRNN sequence model (tests/seq_model_ref.py)
against central finite differences, the loss as executed, and the argument
checks of cg_seq_xent_head / cg_seq_xent_workspace_bytes, which return before
anything touches a device."""
import ctypes

import numpy as np
import pytest

import seq_model_ref as R


def _problem(seed=3, N=2, M=6, F=2, T=3, H=3, K=2):
    rng = np.random.default_rng(seed)
    lap = R.ring_lap(M)
    params = [0.4 * rng.standard_normal((K * F, 4 * H)), 0.4 * rng.standard_normal((K * H, 4 * H)),
              0.2 * rng.standard_normal(4 * H), rng.standard_normal((H, 1)), rng.standard_normal(1)]
    x = rng.standard_normal((N, M, F, T))
    labels = rng.integers(0, M, (N, T))
    labels[0, 0], labels[1, 0] = 0, M - 1
    return x, labels, params, lap, K, H


def test_reference_backward_matches_finite_differences():
    x, labels, params, lap, K, H = _problem()
    loss, _, _, st = R.model_forward(x, labels, params, lap, K, H)
    g = R.model_backward(st, params, lap, K, H)
    names = ("Wx", "Wh", "b", "w", "bh")
    eps = 1e-6

    def f(params_, x_):
        return R.model_forward(x_, labels, params_, lap, K, H)[0]

    rng = np.random.default_rng(0)
    for k, name in enumerate(names + ("x",)):
        target = x if name == "x" else params[k]
        for _ in range(min(6, target.size)):
            idx = tuple(int(rng.integers(0, s)) for s in target.shape)
            vals = []
            for sgn in (1.0, -1.0):
                pert = np.array(target, np.float64)
                pert[idx] += sgn * eps
                vals.append(f(params, pert) if name == "x" else
                            f([pert if j == k else p for j, p in enumerate(params)], x))
            fd = (vals[0] - vals[1]) / (2 * eps)
            an = g[name].reshape(target.shape)[idx]
            if name == "bh":  # exact gradient 0: the analytic value is rounding noise
                assert abs(fd) < 1e-8 and abs(an) < 1e-12
            else:
                assert abs(fd - an) <= 1e-7 * max(1.0, abs(an)), (name, idx, fd, an)


def test_loss_is_batch_sum_time_mean():
    x, labels, params, lap, K, H = _problem(N=2, T=3)
    loss, _, ce, _ = R.model_forward(x, labels, params, lap, K, H)
    T, N = ce.shape
    assert (T, N) == (3, 2)
    assert abs(loss - ce.sum(axis=1).mean()) < 1e-14 * abs(loss)  # (1/T) sum_t sum_n
    assert abs(loss - ce.sum() / T) < 1e-14 * abs(loss)
    assert abs(loss - R.loss_as_named(ce)) > 0.1 * abs(loss)  # not the batch mean: N != T


def test_bias_gradient_is_zero_to_rounding():
    rng = np.random.default_rng(5)
    hd, w = rng.standard_normal((3, 2, 50, 8)), rng.standard_normal(8)
    labels = rng.integers(0, 50, (3, 2))
    logits, _, _ = R.head_forward(hd, w, 0.3, labels, 1 / 3)
    dlogit, _, _, db = R.head_backward(hd, w, logits, labels, 1 / 3)
    assert abs(db) <= 1e-14 * np.abs(dlogit).sum()


def test_host_labels_are_validated_before_upload():
    from cnn_graph_amd import ops
    for bad in ([[0, 5]], [[-1, 0]]):
        with pytest.raises(ValueError):
            ops.seq_xent_labels(np.array(bad, np.int64), 5, "cpu")
    with pytest.raises(TypeError):
        ops.seq_xent_labels(np.array([[0.0, 1.0]]), 5, "cpu")
    ok = ops.seq_xent_labels(np.array([[0, 4]], np.int64), 5, "cpu")
    assert ok.dtype.is_floating_point is False and ok.tolist() == [[0, 4]]


# ---- the C ABI's argument checks (no device is touched) -----------------------------------
def _head(h, **kw):
    a = dict(hs=64, w=64, b=64, labels=64, T=2, N=3, M=5, H=4, keep=1.0, seed=0, scale=0.5,
             logits=None, ce=None, loss=64, dhs=64, dw=64, db=64, ws=64, ws_bytes=1 << 20)
    a.update(kw)
    return h.cg_seq_xent_head(a["hs"], a["w"], a["b"], a["labels"], a["T"], a["N"], a["M"], a["H"],
                              a["keep"], a["seed"], a["scale"], a["logits"], a["ce"], a["loss"],
                              a["dhs"], a["dw"], a["db"], a["ws"], a["ws_bytes"], None)


def test_seq_xent_argument_errors(built_lib):
    from cnn_graph_amd import _lib
    h = _lib.lib()
    for name in ("hs", "w", "b", "labels", "loss", "ws"):  # required pointers
        assert _head(h, **{name: None}) == _lib.CG_ERR_ARG, name
    for name in ("dw", "db"):  # required with dhs
        assert _head(h, **{name: None}) == _lib.CG_ERR_ARG, name
    for name in ("T", "N", "M", "H"):
        for v in (0, -1):
            assert _head(h, **{name: v}) == _lib.CG_ERR_ARG, (name, v)
    for keep in (0.0, -0.5, 1.5, float("nan")):
        assert _head(h, keep=keep) == _lib.CG_ERR_ARG, keep
    need = ctypes.c_size_t()
    assert h.cg_seq_xent_workspace_bytes(2, 3, 5, 4, ctypes.byref(need)) == _lib.CG_OK
    assert need.value > 0
    assert _head(h, ws_bytes=need.value - 1) == _lib.CG_ERR_ARG
    assert b"workspace" in h.cg_last_error()
    # H past the supported width: the unsupported status, with a message
    assert _head(h, H=257) == _lib.CG_ERR_UNSUPPORTED
    assert b"256" in h.cg_last_error()
    assert h.cg_seq_xent_workspace_bytes(2, 3, 5, 257, ctypes.byref(need)) == _lib.CG_ERR_UNSUPPORTED
    assert h.cg_seq_xent_workspace_bytes(2, 3, 5, 4, None) == _lib.CG_ERR_ARG
    assert h.cg_seq_xent_workspace_bytes(0, 3, 5, 4, ctypes.byref(need)) == _lib.CG_ERR_ARG


def test_seq_xent_workspace_is_monotone_in_pairs(built_lib):
    from cnn_graph_amd import ops
    for M, H in ((100, 32), (1024, 32), (20000, 7)):  # the last keeps its logits in the workspace
        prev = 0
        for T, N in ((1, 1), (1, 2), (2, 2), (3, 2), (12, 128), (12, 129), (13, 129)):
            nb = ops.seq_xent_workspace_bytes(T, N, M, H)
            assert nb >= prev and nb >= (H + 2) * T * N * 4, (T, N, M, H)
            prev = nb
        assert prev > ops.seq_xent_workspace_bytes(1, 1, M, H)
