"""What tests/test_gpu_gconv_net.py rests on, checked without a GPU: the float64
restatement's gradients (tests/gconv_net_ref.py) against central finite
differences of its own forward, the reference's variable names and creation
order, and the branches' column ranges."""
import json
import os

import numpy as np
import pytest

import gconv_net_ref as GR
import glstm_gconv_ref as GG
# the step and bar of the same check for the Fourier ResGNN restatement (derived there)
from test_fourier_resgnn_ref_cpu import FD_BAR, FD_STEP

M, N, T, H, K, R, OUT = 12, 2, (2, 1, 1), 3, 3, 1, 2
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "gconv_net_variables.json")


def _fd_check(f, weights, grads, rng):
    got, ref = [], []
    for i, (W, g) in enumerate(zip(weights, grads)):
        D = rng.standard_normal(W.shape)
        plus = [w + FD_STEP * D if j == i else w for j, w in enumerate(weights)]
        minus = [w - FD_STEP * D if j == i else w for j, w in enumerate(weights)]
        got.append((f(plus) - f(minus)) / (2 * FD_STEP))
        ref.append(float(np.sum(g * D)))
    got, ref = np.array(got), np.array(ref)
    scale = np.abs(got).max()
    assert scale > 1e-4
    err = np.abs(got - ref).max() / scale
    print(f"finite differences: directional derivatives {got}, relative error {err:.2e}")
    assert err < FD_BAR, (got, ref)


@pytest.mark.parametrize("infer_func", GR.INFER_FUNCS)
def test_reference_gradients_match_finite_differences(infer_func):
    rng = np.random.default_rng(11 + GR.INFER_FUNCS.index(infer_func))
    lap = GG.cheb_lap(GG.ring_chords_laplacian(M))
    params = GR.seeded_params(rng, infer_func, T, H, K, R, OUT, scale=0.3)
    x = rng.standard_normal((N, M, 2 * sum(T)))
    labels = rng.standard_normal((N, M, OUT))
    _, out, grads, fw = GR.loss_and_grads(x, labels, params, infer_func, lap, K, R, T)
    assert out.shape == (N, M, OUT)
    acts = {c[4] for cache in fw["caches"] for c in cache}
    assert acts == {"inference_gconv": {"tanh", "none"},
                    "inference_gconv_period_no_expand": {"relu", "none"},
                    "inference_gconv_period_expand": {"tanh", "relu"}}[infer_func]
    for cache in fw["caches"]:  # the ReLUs clamp some entries and pass others
        for _, _, pre, _, act in cache:
            if act == "relu":
                assert np.count_nonzero(pre < 0) > 0 and np.count_nonzero(pre > 0) > 0
    flat_w = GR.flat(params, infer_func)
    _fd_check(lambda w: GR.loss(x, labels, GR.unflat(w, infer_func), infer_func, lap, K, R, T),
              flat_w, GR.flat(grads, infer_func), rng)


@pytest.mark.parametrize("infer_func", GR.INFER_FUNCS)
def test_variable_names_and_order(infer_func):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert GR.variable_names(infer_func, 1) == golden[infer_func]
    from cnn_graph_amd import gconv_net
    assert gconv_net.variable_names(infer_func, 1) == golden[infer_func]
    assert gconv_net.variable_names(infer_func, 3) == GR.variable_names(infer_func, 3)
    assert len(GR.shapes(infer_func, T, H, K, 1, OUT)) == len(golden[infer_func])
    assert tuple(gconv_net.INFER_FUNCS) == tuple(GR.INFER_FUNCS) == tuple(k for k in golden if k[0] != "_")


def test_branch_columns():
    from cnn_graph_amd import gconv_net
    want = [(0, 6), (6, 10), (10, 12)]
    assert GR.branch_columns((3, 2, 1)) == want
    assert gconv_net.branch_columns((3, 2, 1)) == want


def test_train_step_composes_the_oracles():
    from oracle import cheb_oracle as O
    infer_func = GR.EXPAND
    rng = np.random.default_rng(5)
    lap = GG.cheb_lap(GG.ring_chords_laplacian(M))
    params = GR.seeded_params(rng, infer_func, T, H, K, R, OUT)
    x = rng.standard_normal((N, M, 2 * sum(T)))
    labels = rng.standard_normal((N, M, OUT))
    ws = GR.flat(params, infer_func)
    state = [(np.zeros_like(w), np.zeros_like(w)) for w in ws]
    l, gs, new, st2 = GR.train_step(x, labels, params, infer_func, lap, K, R, T, state, 1, 1e-2)
    assert l == GR.loss(x, labels, params, infer_func, lap, K, R, T)
    for w, g, w2 in zip(ws, gs, GR.flat(new, infer_func)):
        assert np.array_equal(w2, O.adam_step(w, g, np.zeros_like(w), np.zeros_like(w), 1, lr=1e-2)[0])
