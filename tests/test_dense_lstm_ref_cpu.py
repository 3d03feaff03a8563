"""tests/dense_lstm_ref.py pinned down without a GPU: its backward against central
finite differences of its forward on every parameter and on x, and the
known-answer checks that would catch a wrong restatement of
lib/gconvRNN.py::Model(model_type='lstm') / TF 1.x BasicLSTMCell."""
import numpy as np

import dense_lstm_ref as R

N, T, C, H = 3, 3, 5, 4


def problem(seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, T))
    labels = rng.integers(0, C, (N, T))
    labels[0, 0], labels[-1, -1] = 0, C - 1
    params = [rng.standard_normal((H, C)), rng.standard_normal((C,)),
              0.5 * rng.standard_normal((C + H, 4 * H)), 0.3 * rng.standard_normal((4 * H,))]
    return x, labels, params


def test_backward_matches_central_differences():
    x, labels, params = problem()
    mask = (np.random.default_rng(9).random((T, N, H)) < 0.8).astype(np.float64)
    assert 0 < mask.sum() < mask.size
    for m, keep in ((None, 1.0), (mask, 0.8)):
        _, _, st = R.model_forward(x, labels, params, 1.0, m, keep)
        g = R.model_backward(st, params)
        eps = 1e-6
        for k, p in list(zip(R.NAMES, params)) + [("x", x)]:
            num = np.zeros_like(p)
            for idx in np.ndindex(p.shape):
                old = p[idx]
                p[idx] = old + eps
                lp = R.model_forward(x, labels, params, 1.0, m, keep)[0]
                p[idx] = old - eps
                lm = R.model_forward(x, labels, params, 1.0, m, keep)[0]
                p[idx] = old
                num[idx] = (lp - lm) / (2 * eps)
            err = np.linalg.norm(num - g[k]) / np.linalg.norm(num)
            assert err < 1e-7, (k, err)


def test_cell_backward_matches_central_differences_of_the_cell():
    rng = np.random.default_rng(5)
    gx, Wh, b = rng.standard_normal((T, N, 4 * H)), rng.standard_normal((H, 4 * H)), rng.standard_normal(4 * H)
    dhs = rng.standard_normal((T, N, H))
    hs, cs, act = R.cell_forward(gx, Wh, b, 1.0)
    dpre = R.cell_backward(dhs, act, cs, Wh)
    f = lambda: (R.cell_forward(gx, Wh, b, 1.0)[0] * dhs).sum()  # noqa: E731
    num = np.zeros_like(gx)
    for idx in np.ndindex(gx.shape):
        old = gx[idx]
        gx[idx] = old + 1e-6
        lp = f()
        gx[idx] = old - 1e-6
        num[idx] = (lp - f()) / 2e-6
        gx[idx] = old
    assert np.linalg.norm(num - dpre) / np.linalg.norm(num) < 1e-7


def test_one_step_known_answer_and_gate_order():
    """T = 1, zero state: h = tanh(sigmoid(a_i) tanh(a_j)) sigmoid(a_o), the f
    block and forget_bias do not matter; columns are i | j | f | o."""
    a = np.array([[[0.3, -1.2, 0.7, 2.0]]])  # H = 1: a_i, a_j, a_f, a_o
    hs, cs, act = R.cell_forward(a, np.zeros((1, 4)), np.zeros(4), 1.0)
    c = R.sigmoid(0.3) * np.tanh(-1.2)
    assert np.allclose(cs, c, atol=1e-15) and np.allclose(hs, np.tanh(c) * R.sigmoid(2.0), atol=1e-15)
    assert np.allclose(act[0, 0], [R.sigmoid(0.3), np.tanh(-1.2), R.sigmoid(1.7), R.sigmoid(2.0)])
    # swapping the j and f blocks changes the output
    swapped = R.cell_forward(a, np.zeros((1, 4)), np.zeros(4), 1.0, order="ifjo")[0]
    assert abs(swapped - hs).max() > 0.05


def test_forget_bias_enters_f_only():
    rng = np.random.default_rng(2)
    gx, Wh, b = rng.standard_normal((2, N, 4 * H)), rng.standard_normal((H, 4 * H)), rng.standard_normal(4 * H)
    b2 = b.copy()
    b2[2 * H:3 * H] += 1.0  # forget_bias = 1 is a shift of the f block's bias ...
    ref = R.cell_forward(gx, Wh, b, 1.0)
    for a_, b_ in zip(ref, R.cell_forward(gx, Wh, b2, 0.0)):
        assert np.allclose(a_, b_, atol=1e-14)
    for blk in (0, 1, 3):  # ... and of no other block
        b3 = b.copy()
        b3[blk * H:(blk + 1) * H] += 1.0
        assert abs(R.cell_forward(gx, Wh, b3, 0.0)[0] - ref[0]).max() > 1e-3
    # step 0 has c = 0: the f gate and so forget_bias cannot matter there
    assert np.array_equal(R.cell_forward(gx[:1], Wh, b, 5.0)[0], R.cell_forward(gx[:1], Wh, b, 0.0)[0])


def test_loss_is_the_sum_over_the_batch_averaged_over_time():
    x, labels, params = problem()
    loss, logits, st = R.model_forward(x, labels, params)
    ce = st[8]  # [T, N]
    lse = np.log(np.exp(logits).sum(2))
    assert np.allclose(ce, lse - np.take_along_axis(logits, labels.T[:, :, None], 2)[:, :, 0])
    assert np.isclose(loss, ce.sum() / T, rtol=1e-14)
    assert not np.isclose(loss, ce.mean(), rtol=1e-3)  # not the batch mean


def test_pred_out_column_order():
    logits = np.arange(T * N * C, dtype=np.float64).reshape(T, N, C)
    p = R.pred_out(logits)
    assert p.shape == (N, T * C)
    for t in range(T):
        for c in range(C):
            assert np.array_equal(p[:, t * C + c], logits[t, :, c])


def test_clip_treats_the_kernel_as_one_variable():
    x, labels, params = problem()
    clip = 1e-3
    _, _, st = R.model_forward(x, labels, params)
    g = R.model_backward(st, params)
    p1, _, _ = R.sgd_steps(x, labels, params, 0.1, 1, clip=clip)
    step = (params[2] - p1[2]) / 0.1
    # (p - p') / lr cancels: |p| eps / lr ~ 2e-15 absolute against a step of norm 1e-3
    assert np.isclose(np.sqrt((step ** 2).sum()), clip, rtol=1e-9)  # ONE norm over [C + H, 4H]
    assert np.linalg.norm(step - R.clip_by_norm(g["kernel"], clip)) < 1e-9 * clip
    apart = np.concatenate([R.clip_by_norm(g["kernel"][:C], clip), R.clip_by_norm(g["kernel"][C:], clip)])
    assert np.linalg.norm(step - apart) > 0.1 * clip
    # a gradient under the norm passes unchanged
    assert np.array_equal(R.clip_by_norm(g["b"], 1e9), g["b"])


def test_t1_has_no_recurrent_weight_gradient():
    x, labels, params = problem()
    _, _, st = R.model_forward(x[:, :, :1], labels[:, :1], params)
    g = R.model_backward(st, params)
    assert np.array_equal(g["kernel"][C:], np.zeros((H, 4 * H))) and abs(g["kernel"][:C]).max() > 0
