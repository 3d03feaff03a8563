"""The float64 reference of the cgcnn classifier (tests/cgcnn_ref.py) against
central finite differences of its own forward, its Momentum update by hand, and
cgcnn.weighted_f1 against scikit-learn."""
import numpy as np
import pytest

import cgcnn_ref as R

MARGIN = 1e-3  # >> the 1e-6 perturbation: no ReLU or argmax changes side under it


def _problem(brelu, pool, seed, with_mask=False):
    rng = np.random.default_rng(seed)
    N, Fin, F, K, p, fc = 3, 2, [3, 2], [3, 2], [2, 2], [5, 4]
    Ms = [8, 4]
    net = dict(laps=[R.ring_lap(m, rng) for m in Ms], K=K, p=p, brelu=brelu, pool=pool, nfc=2,
               reg=5e-4)
    params = R.init_params(rng, net, Fin, F, Ms, [Ms[-1] // p[-1] * F[-1]] + fc)
    x = rng.standard_normal((N, Ms[0], Fin))
    labels = np.array([0, fc[-1] - 1, 1])
    masks = [np.where(rng.random((N, fc[0])) < 0.5, 2.0, 0.0)] if with_mask else None
    return x, labels, params, net, masks


def _well_separated(brelu, pool, with_mask=False):
    """The first seed whose forward keeps every ReLU input and pool gap MARGIN away from zero."""
    for seed in range(200):
        x, labels, params, net, masks = _problem(brelu, pool, seed, with_mask)
        _, _, st = R.forward(x, labels, params, net, masks)
        if R.margins_ok(st, MARGIN):
            return x, labels, params, net, masks
    raise AssertionError("no seed with the margin: change the shape, not the margin")


@pytest.mark.parametrize("brelu,pool,with_mask", [("b1relu", "mpool1", False), ("b2relu", "apool1", True),
                                                  ("b2relu", "mpool1", False)])
def test_reference_backward_matches_finite_differences(brelu, pool, with_mask):
    x, labels, params, net, masks = _well_separated(brelu, pool, with_mask)
    net0 = dict(net, reg=0.0)  # backward() is the data term's gradient
    _, _, st = R.forward(x, labels, params, net0, masks)
    assert R.margins_ok(st, MARGIN)
    grads, dx = R.backward(st, params, net0)
    assert len(grads) == len(params)
    eps = 1e-6
    rng = np.random.default_rng(0)

    def f(params_, x_):
        return R.forward(x_, labels, params_, net0, masks)[1]

    for k in range(len(params) + 1):
        target = x if k == len(params) else params[k]
        an_all = dx if k == len(params) else grads[k].reshape(target.shape)
        for _ in range(min(6, target.size)):
            idx = tuple(int(rng.integers(0, s)) for s in target.shape)
            vals = []
            for sgn in (1.0, -1.0):
                pert = np.array(target, np.float64)
                pert[idx] += sgn * eps
                vals.append(f(params, pert) if k == len(params) else
                            f([pert if j == k else q for j, q in enumerate(params)], x))
            fd, an = (vals[0] - vals[1]) / (2 * eps), an_all[idx]
            assert abs(fd - an) <= 1e-7 * max(1.0, abs(an)), (k, idx, fd, an)


def test_regularisation_term_and_its_gradient():
    x, labels, params, net, _ = _well_separated("b2relu", "mpool1")
    _, with_reg, _ = R.forward(x, labels, params, net)
    _, without, _ = R.forward(x, labels, params, dict(net, reg=0.0))
    mask = R.regularised(net, params)
    assert mask == [False] * 4 + [True] * 4  # conv weights and b2relu biases are not regularised
    want = net["reg"] * sum(0.5 * (v ** 2).sum() for v, r in zip(params, mask) if r)
    assert abs((with_reg - without) - want) <= 1e-15 * with_reg
    # one Momentum step from zero accumulators: w - lr (g + reg w) on the regularised ones
    grads = [np.ones_like(v) for v in params]
    new, acc = R.momentum_step(params, grads, [np.zeros_like(v) for v in params], 0.1, 0.9,
                               net["reg"], mask)
    assert np.array_equal(new[0], params[0] - 0.1 * grads[0])
    assert np.allclose(new[-1], params[-1] - 0.1 * (1.0 + net["reg"] * params[-1]), rtol=0, atol=1e-16)
    # the second step carries 0.9 of the first
    new2, acc2 = R.momentum_step(new, grads, acc, 0.1, 0.9, net["reg"], mask)
    assert np.allclose(acc2[0], 1.9 * grads[0], rtol=0, atol=1e-15)
    assert np.allclose(new2[0], params[0] - 0.1 * (1.0 + 1.9) * grads[0], rtol=0, atol=1e-15)


def test_pool_backwards_route_and_spread():
    x = np.array([[[1.0], [1.0], [0.0], [2.0]]])  # a tie in the first window
    y, arg = R.O.mpool1_forward(x, 2)
    assert arg.ravel().tolist() == [0, 3]      # the FIRST maximum
    dx = R.mpool_backward(np.array([[[5.0], [7.0]]]), arg, 4)
    assert dx.ravel().tolist() == [5.0, 0.0, 0.0, 7.0]
    assert R.apool_backward(np.array([[[4.0], [8.0]]]), 2).ravel().tolist() == [2.0, 2.0, 4.0, 4.0]
    assert R.apool_forward(x, 2).ravel().tolist() == [1.0, 1.0]


def test_weighted_f1_matches_sklearn():
    pytest.importorskip("sklearn")
    from sklearn import metrics
    from cnn_graph_amd.cgcnn import weighted_f1
    rng = np.random.default_rng(1)
    for C, n in ((2, 50), (10, 300), (5, 7)):
        y, q = rng.integers(0, C, n), rng.integers(0, C, n)
        assert abs(weighted_f1(y, q) - metrics.f1_score(y, q, average="weighted")) < 1e-12
    y, q = np.array([0, 0, 1, 1]), np.array([0, 0, 0, 0])  # a class that is never predicted
    assert abs(weighted_f1(y, q) - metrics.f1_score(y, q, average="weighted", zero_division=0)) < 1e-12
