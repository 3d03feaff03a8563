"""What the class loss, the Momentum update and CGCNNModel refuse before anything
touches a device: the argument checks of cg_class_xent_ema /
cg_class_xent_workspace_bytes / cg_momentum_update, the host-side validators of
ops.py, and the constructor's checks."""
import ctypes

import numpy as np
import pytest
import scipy.sparse


def _xent(h, **kw):
    a = dict(logits=64, labels=64, N=3, C=10, params=64, rb=0, rn=8, scale=5e-4, loss=64, dlogits=128,
             ema=64, decay=0.9, pred=64, correct=64, status=64, ws=64, ws_bytes=1 << 20)
    a.update(kw)
    return h.cg_class_xent_ema(a["logits"], a["labels"], a["N"], a["C"], a["params"], a["rb"], a["rn"],
                               a["scale"], a["loss"], a["dlogits"], a["ema"], a["decay"], a["pred"],
                               a["correct"], a["status"], a["ws"], a["ws_bytes"], None)


def test_class_xent_argument_errors(built_lib):
    from cnn_graph_amd import _lib
    h = _lib.lib()
    for name in ("logits", "labels", "loss", "ws"):  # required pointers
        assert _xent(h, **{name: None}) == _lib.CG_ERR_ARG, name
    for name in ("N", "C"):
        for v in (0, -1):
            assert _xent(h, **{name: v}) == _lib.CG_ERR_ARG, (name, v)
    assert _xent(h, N=1 << 16, C=1 << 15) == _lib.CG_ERR_ARG  # N * C = 2^31
    assert b"2^31" in h.cg_last_error()
    assert _xent(h, rb=-1) == _lib.CG_ERR_ARG
    assert _xent(h, rn=-1) == _lib.CG_ERR_ARG
    assert _xent(h, params=None) == _lib.CG_ERR_ARG  # a range without a buffer
    for decay in (-0.1, 1.5, float("nan")):
        assert _xent(h, decay=decay) == _lib.CG_ERR_ARG, decay
    assert _xent(h, dlogits=64) == _lib.CG_ERR_ARG  # dlogits is logits
    need = ctypes.c_size_t()
    assert h.cg_class_xent_workspace_bytes(3, 10, 8, ctypes.byref(need)) == _lib.CG_OK
    assert need.value >= (2 * 3 + 1) * 4
    assert _xent(h, ws_bytes=need.value - 1) == _lib.CG_ERR_ARG
    assert b"workspace" in h.cg_last_error()
    assert h.cg_class_xent_workspace_bytes(3, 10, 8, None) == _lib.CG_ERR_ARG
    assert h.cg_class_xent_workspace_bytes(0, 10, 8, ctypes.byref(need)) == _lib.CG_ERR_ARG
    assert h.cg_class_xent_workspace_bytes(3, 0, 8, ctypes.byref(need)) == _lib.CG_ERR_ARG
    assert h.cg_class_xent_workspace_bytes(3, 10, -1, ctypes.byref(need)) == _lib.CG_ERR_ARG
    assert h.cg_class_xent_workspace_bytes(1 << 16, 1 << 15, 0, ctypes.byref(need)) == _lib.CG_ERR_ARG


def test_class_xent_workspace_grows_with_rows_and_range(built_lib):
    from cnn_graph_amd import ops
    prev = 0
    for N in (1, 3, 128, 4096):
        nb = ops.class_xent_workspace_bytes(N, 10, 0)
        assert nb >= prev and nb >= 2 * N * 4
        prev = nb
    assert ops.class_xent_workspace_bytes(4, 10, 1 << 24) > ops.class_xent_workspace_bytes(4, 10, 0)


def _mom(h, **kw):
    a = dict(param=64, grad=128, accum=192, n=16, lr=0.1, momentum=0.9, scale=1.0, reg=5e-4, rb=3, rn=5)
    a.update(kw)
    return h.cg_momentum_update(a["param"], a["grad"], a["accum"], a["n"], a["lr"], a["momentum"],
                                a["scale"], a["reg"], a["rb"], a["rn"], None)


def test_momentum_update_argument_errors(built_lib):
    from cnn_graph_amd import _lib
    h = _lib.lib()
    for name in ("param", "grad", "accum"):
        assert _mom(h, **{name: None}) == _lib.CG_ERR_ARG, name
    assert _mom(h, n=-1) == _lib.CG_ERR_ARG
    for m in (-0.5, float("nan")):
        assert _mom(h, momentum=m) == _lib.CG_ERR_ARG, m
    for rb, rn in ((-1, 2), (0, -1), (17, 0), (12, 5), (0, 17)):
        assert _mom(h, rb=rb, rn=rn) == _lib.CG_ERR_ARG, (rb, rn)
    assert b"range" in h.cg_last_error()
    assert _mom(h, grad=64) == _lib.CG_ERR_ARG   # grad is param
    assert _mom(h, accum=128) == _lib.CG_ERR_ARG  # accum is grad
    # nothing to do: no launch, so no device is needed
    assert _mom(h, n=0, rb=0, rn=0) == _lib.CG_OK
    assert _mom(h, n=0, rb=0, rn=0, momentum=0.0, accum=None) == _lib.CG_OK


def test_class_labels_are_validated_before_upload():
    from cnn_graph_amd import ops
    for bad in ([0, 5], [-1, 0]):
        with pytest.raises(ValueError):
            ops.class_labels(np.array(bad, np.int64), 5, "cpu")
    with pytest.raises(ValueError):
        ops.class_labels(np.array([[0, 1]], np.int64), 5, "cpu")  # [N] class ids, not one-hot rows
    with pytest.raises(TypeError):
        ops.class_labels(np.array([0.0, 1.0]), 5, "cpu")
    ok = ops.class_labels(np.array([0, 4], np.int64), 5, "cpu")
    assert str(ok.dtype) == "torch.int32" and ok.tolist() == [0, 4]


def test_momentum_update_validates_on_the_host():
    import torch
    from cnn_graph_amd import ops
    p = torch.zeros(8)
    with pytest.raises(ValueError):  # no CPU path
        ops.momentum_update(p, torch.zeros(8), torch.zeros(8))
    for rb, rn in ((-1, 1), (0, 9), (8, 1)):
        with pytest.raises(ValueError):
            ops._check_reg_range(8, rb, rn)
    assert ops._check_reg_range(8, 3, 5) == (3, 5)


def _pyramid(sizes=(8, 4, 2)):
    return [scipy.sparse.identity(m, format="csr", dtype=np.float32) for m in sizes]


def test_cgcnn_constructor_refusals():
    from cnn_graph_amd import CGCNNModel
    L = _pyramid()
    ok = dict(L=L, N=2, F=[2, 3], K=[2, 2], p=[2, 2], M=[4, 3], device="cpu")

    def refused(**kw):
        with pytest.raises(ValueError):
            CGCNNModel(**{**ok, **kw})

    refused(filter="fourier")
    refused(filter="lanczos2")
    refused(brelu="b1tanh")
    refused(pool="mpool2")
    refused(K=[2])                       # len(F) != len(K)
    refused(p=[2])                       # len(K) != len(p)
    refused(F=[2], K=[2, 2], p=[2, 2])
    refused(p=[4, 2])                    # needs 1 + 3 graph levels, there are 3
    refused(L=L[:2])                     # too few graph levels for p = [2, 2]
    refused(p=[3, 2])                    # not a power of 2
    refused(L=[])
    for d in (0.0, -0.5, 1.5):
        refused(dropout=d)
    refused(M=[])
    refused(F=[0, 3])
    refused(momentum=-0.1)
    refused(regularization=-1.0)
    refused(L=_pyramid((8, 5, 2)))       # level sizes that pooling does not connect


def test_weighted_f1_by_hand():
    from cnn_graph_amd.cgcnn import weighted_f1
    y = [0, 0, 0, 1, 1, 2]
    q = [0, 0, 1, 1, 2, 2]
    # class 0: tp 2 fp 0 fn 1 -> 0.8; class 1: tp 1 fp 1 fn 1 -> 0.5; class 2: tp 1 fp 1 fn 0 -> 2/3
    want = (3 * 0.8 + 2 * 0.5 + 1 * (2 / 3)) / 6
    assert abs(weighted_f1(y, q) - want) < 1e-15
    assert weighted_f1([1, 1], [0, 0]) == 0.0      # a class nobody predicted, one nobody has
    assert weighted_f1([2, 2, 2], [2, 2, 2]) == 1.0
