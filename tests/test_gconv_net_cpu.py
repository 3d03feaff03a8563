"""GConvNetModel's constructor refusals and the argument checks of the tanh
entries that need no device."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

from cnn_graph_amd import _lib, ops
from cnn_graph_amd.gconv_net import INFER_FUNCS, GConvNetModel

L = scipy.sparse.identity(8, dtype=np.float32, format="csr")


def test_unknown_infer_func_is_refused():
    with pytest.raises(ValueError, match="infer_func must be one of"):
        GConvNetModel(L, 2, infer_func="inference_glstm")
    assert INFER_FUNCS == ("inference_gconv", "inference_gconv_period_no_expand",
                           "inference_gconv_period_expand")


@pytest.mark.parametrize("infer_func", ["inference_gconv", "inference_gconv_period_expand"])
def test_fourier_filter_with_a_tanh_network_is_refused(infer_func):
    with pytest.raises(NotImplementedError, match="Fourier store has no tanh"):
        GConvNetModel(L, 2, infer_func=infer_func, filter="fourier_conv")


def test_unknown_filter_is_refused():
    with pytest.raises(ValueError, match="filter must be"):
        GConvNetModel(L, 2, filter="chebyshev5")


@pytest.mark.parametrize("T", [(3, 3), (3, 0, 3), 3, (1, 2, 3, 4)])
def test_bad_T_is_refused(T):
    with pytest.raises(ValueError, match="T must be"):
        GConvNetModel(L, 2, T=T, infer_func="inference_gconv_period_expand")


def test_in_features_of_the_branch_network_must_match_T():
    with pytest.raises(ValueError, match="in_features"):
        GConvNetModel(L, 2, T=(1, 1, 1), in_features=5, infer_func="inference_gconv_period_expand")
    with pytest.raises(ValueError, match="in_features"):
        GConvNetModel(L, 2, T=(1, 1, 1), in_features=0)


def test_tanh_is_an_activation_of_the_chebyshev_entries(built_lib):
    """Act 2 passes the activation check of the four entries (a null plan is what
    refuses the call next); act 3 is refused with the pinned wording."""
    h = _lib.lib()
    assert ops.ACTS == {"none": 0, "relu": 1, "tanh": 2}
    p = [ctypes.c_void_p(4096 * k) for k in range(1, 8)]

    def bwd_ex(act):
        return h.cg_cheb_backward_ex(None, 1, 1, 2, 1, p[0], p[1], act, p[2], p[3], p[4], 0, p[5], p[6],
                                     None, 0, None)

    def bwd_layout(act):
        return h.cg_cheb_backward_layout(None, 1, 1, 2, 1, p[0], p[1], act, _lib.CG_BASIS_ROWS, p[2], p[3],
                                         p[4], 0, p[5], p[6], None, 0, None)

    for call in (bwd_ex, bwd_layout):
        assert call(3) == _lib.CG_ERR_ARG
        assert h.cg_last_error().decode() == "unknown activation 3"
        assert call(-1) == _lib.CG_ERR_ARG
        assert h.cg_last_error().decode() == "unknown activation -1"
        assert call(_lib.CG_ACT_TANH) == _lib.CG_ERR_ARG
        assert "activation" not in h.cg_last_error().decode()
        assert "null plan" in h.cg_last_error().decode()


def test_act_forward_validates(built_lib):
    h = _lib.lib()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    assert "cg_act_forward" in _lib.header_symbols()
    assert h.cg_act_forward(0, p, None, 2, None) == _lib.CG_ERR_ARG
    assert h.cg_act_forward(16, None, None, 2, None) == _lib.CG_ERR_ARG
    assert h.cg_act_forward(16, p, q, 3, None) == _lib.CG_ERR_ARG
    assert h.cg_last_error().decode() == "unknown activation 3"
    assert h.cg_act_forward(16, p, p, 2, None) == _lib.CG_ERR_ARG
    assert "aliases" in h.cg_last_error().decode()
    assert h.cg_version() == 301  # additive
