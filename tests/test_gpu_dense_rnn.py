"""dense_rnn.LSTMRNNModel (lib/gconvRNN.py::Model, model_type='lstm') against the
float64 reference of tests/dense_lstm_ref.py at N 4, T 3, C 40, H 32: the loss
as executed ((1/T) sum_t sum_n ce), every gradient, pred_out, sgd / adam /
rmsprop steps, the per-variable clip, the output dropout, test_step and
predict.  Bar: 1e-5 normwise, the scalar loss 1e-5 relative."""
import numpy as np
import pytest

import dense_lstm_ref as R
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
N, T, C, H = 4, 3, 40, 32


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def make(dev, seed=11, **kw):
    from cnn_graph_amd import LSTMRNNModel
    kw.setdefault("keep_prob", 1.0)
    kw.setdefault("learning_rate", 0.01)
    m = LSTMRNNModel(N, T, C, num_hidden=H, device=dev, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, T)).astype(np.float32)
    labels = rng.integers(0, C, (N, T))
    labels[0, 0], labels[-1, -1] = 0, C - 1
    return m, x, labels


def params64(m):
    p = m.parameters()
    assert list(p) == ["gconv_model/weight", "gconv_model/bias", "gconv_model/rnn/basic_lstm_cell/kernel",
                       "gconv_model/rnn/basic_lstm_cell/bias"]  # the reference's creation order
    assert [tuple(a.shape) for a in p.values()] == [(H, C), (C,), (C + H, 4 * H), (4 * H,)]
    return [a.detach().cpu().numpy().astype(np.float64) for a in p.values()]


def grads64(m):
    return dict(zip(R.NAMES, (g.detach().cpu().numpy().astype(np.float64) for g in m.gradients().values())))


def check(got, ref, what):
    for k in R.NAMES:
        a, b = (got[k], ref[k]) if isinstance(got, dict) else (got[R.NAMES.index(k)], ref[R.NAMES.index(k)])
        err = O.normwise_err(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1))
        print(f"{what} {k}: {err:.2e}")
        assert err < TOL, (what, k, err)


def test_initial_values(dev):
    m, _, _ = make(dev)
    w, bh, kernel, b = params64(m)
    lim = np.sqrt(6.0 / ((C + H) + 4 * H))  # glorot-uniform over [C + H, 4H]
    assert abs(kernel).max() <= lim and abs(kernel).max() > 0.9 * lim and abs(kernel.mean()) < 0.1 * lim
    assert not b.any()
    assert 0.8 < w.std() < 1.2 and abs(bh).max() > 0.5  # random_normal(0, 1)
    assert m.Wx.data_ptr() == m.kernel.data_ptr() and m.Wh.data_ptr() == m.kernel.data_ptr() + 4 * C * 4 * H


@pytest.mark.parametrize("path", ["seq", "steps"])
def test_loss_gradients_pred_out_and_sgd_steps(dev, path):
    m, x, labels = make(dev, optimizer="sgd", path=path)
    assert m.path == path
    p0 = params64(m)
    xs = t(x, dev)
    loss, out = m.train_step(xs, labels, with_output=True)
    torch.cuda.synchronize()
    ref_loss, logits, st = R.model_forward(x, labels, p0)
    rel = abs(float(loss.item()) - ref_loss) / ref_loss
    print(f"{path}: loss {float(loss.item()):.6f} ref {ref_loss:.6f} rel {rel:.2e}")
    assert rel < TOL
    assert tuple(out.shape) == (N, T * C)
    assert O.normwise_err(out.cpu().numpy(), R.pred_out(logits)) < TOL
    check(grads64(m), R.model_backward(st, p0), path)
    for _ in range(2):
        m.train_step(xs, labels)
    torch.cuda.synchronize()
    assert m.step_count == 3
    ref_p, _, _ = R.sgd_steps(x, labels, p0, 0.01, 3)
    got = params64(m)
    check(got, ref_p, f"{path} after 3 sgd steps")
    for a, b in zip(got, p0):
        assert not np.array_equal(a, b)


@pytest.mark.parametrize("opt", ["adam", "rmsprop"])
def test_one_step_of_adam_and_rmsprop(dev, opt):
    """One step on the reference gradient through float64 restatements of TF
    1.x's training ops, as tests/test_gpu_optim.py has them (ApplyAdam: epsilon
    outside the bias correction, lr_t = lr sqrt(1 - b2^t) / (1 - b1^t);
    ApplyRMSProp: decay 0.9, eps 1e-10 inside the root, ms starting at one).
    torch.optim.Adam puts epsilon elsewhere -- lr g / (|g| + 1e-8) against TF's
    lr g / (|g| + 3.2e-7) on the first step -- which is 3e-5 of a kernel entry
    at |g| = 1e-3: it is not the reference's rule."""
    m, x, labels = make(dev, optimizer=opt)
    p0 = params64(m)
    m.train_step(t(x, dev), labels)
    torch.cuda.synchronize()
    _, _, st = R.model_forward(x, labels, p0)
    g = R.model_backward(st, p0)
    for k, p, got in zip(R.NAMES, p0, params64(m)):
        if opt == "adam":
            lr_t = 0.01 * np.sqrt(1 - 0.999) / (1 - 0.9)
            mom, v = 0.1 * g[k], 0.001 * g[k] ** 2
            ref = p - lr_t * mom / (np.sqrt(v) + 1e-8)
        else:
            ms = 0.9 * 1.0 + 0.1 * g[k] ** 2
            ref = p - 0.01 * g[k] / np.sqrt(ms + 1e-10)
        err = O.normwise_err(got.reshape(-1), ref.reshape(-1))
        print(f"{opt} {k}: {err:.2e}")
        assert err < TOL, (opt, k, err)
        assert not np.array_equal(got, p)


def test_clipping_is_per_variable_over_the_whole_kernel(dev):
    clip = 1e-3
    m, x, labels = make(dev, optimizer="sgd", max_grad_norm=clip)
    p0 = params64(m)
    xs = t(x, dev)
    m.train_step(xs, labels)
    torch.cuda.synchronize()
    _, _, st = R.model_forward(x, labels, p0)
    ref_g = R.model_backward(st, p0)
    for k in R.NAMES:
        assert np.sqrt((ref_g[k] ** 2).sum()) > 10 * clip, k  # the clip binds, on the kernel too
    got = grads64(m)
    check(got, {k: R.clip_by_norm(ref_g[k], clip) for k in R.NAMES}, "clipped")
    for k in R.NAMES:
        assert abs(np.sqrt((got[k] ** 2).sum()) - clip) < 1e-5 * clip
    check(params64(m), R.sgd_steps(x, labels, p0, 0.01, 1, clip=clip)[0], "clipped step")
    # a NaN in the exchanged gradient raises before the update
    flat, steps = m.flat.clone(), m.step_count
    clip_hook = m._after_exchange

    def poisoned(s):
        m.grad[3] = float("nan")
        clip_hook(s)
    m._after_exchange = poisoned
    with pytest.raises(FloatingPointError):
        m.train_step(xs, labels)
    assert torch.equal(m.flat, flat) and m.step_count == steps


def test_dropout_masks_the_outputs_only(dev):
    from cnn_graph_amd import ops
    m, x, labels = make(dev, optimizer="sgd", keep_prob=0.8, seed=11)
    p0 = params64(m)
    loss = m.train_step(t(x, dev), labels)
    torch.cuda.synchronize()
    ones = torch.ones((T, N, H), device=dev)
    mask = (ops.dropout(ones, 0.8, m.last_drop_seed) != 0).cpu().numpy().astype(np.float64)
    assert 0 < mask.sum() < mask.size  # drops at least one element and keeps at least one
    ref_loss, _, st = R.model_forward(x, labels, p0, 1.0, mask, float(np.float32(0.8)))
    assert abs(float(loss.item()) - ref_loss) < TOL * ref_loss
    check(grads64(m), R.model_backward(st, p0), "dropout")
    plain, _, _ = make(dev, optimizer="sgd", keep_prob=1.0, seed=11)
    assert not torch.equal(plain.train_step(t(x, dev), labels), loss)  # the mask is on


def test_test_step_changes_nothing(dev):
    m, x, labels = make(dev, keep_prob=0.8, optimizer="rmsprop")
    xs = t(x, dev)
    m.train_step(xs, labels)  # non-trivial slots
    torch.cuda.synchronize()
    snap = [a.clone() for a in (m.flat, m.s1, m.s2)]
    steps = m.step_count
    loss, out = m.test_step(xs, labels, with_output=True)
    loss2 = m.test_step(xs, labels)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and tuple(out.shape) == (N, T * C)
    assert not torch.equal(loss, loss2)  # the reference drops at test time too: a new mask
    assert m.step_count == steps
    for a, b in zip(snap, (m.flat, m.s1, m.s2)):
        assert torch.equal(a, b)
    bad = labels.copy()
    bad[1, 1] = C
    with pytest.raises(ValueError):
        m.test_step(xs, bad)
    with pytest.raises(NotImplementedError):
        m.evaluate(x, labels)


def test_predict_pads_the_last_batch(dev):
    m, x, labels = make(dev, keep_prob=0.8)
    size = 2 * N + 1
    data = np.random.default_rng(5).standard_normal((size, C, T)).astype(np.float32)
    flat = m.flat.clone()
    preds = m.predict(data)
    torch.cuda.synchronize()
    assert tuple(preds.shape) == (size, T * C)  # the padded rows are not returned
    assert torch.equal(m.predict(data), preds) and torch.equal(m.flat, flat)  # no dropout, no update
    for b0 in range(0, size, N):
        batch = np.zeros((N, C, T), np.float32)
        n = min(N, size - b0)
        batch[:n] = data[b0:b0 + n]
        out = m.forward(t(batch, dev), dropout=False)
        assert torch.equal(out[:n], preds[b0:b0 + n]), b0
    _, logits, _ = R.model_forward(data[:N], labels, params64(m))
    assert O.normwise_err(preds[:N].cpu().numpy(), R.pred_out(logits)) < TOL
    assert not torch.equal(m.predict(data, reference_dropout=True), preds)


def test_unsupported_hidden_size_is_an_error_not_a_fallback(dev):
    from cnn_graph_amd import LSTMRNNModel
    with pytest.raises(ValueError):
        LSTMRNNModel(N, T, C, num_hidden=24, device=dev, path="seq")
    with pytest.raises(ValueError):
        LSTMRNNModel(N, T, C, num_hidden=32, device=dev, path="eager")


def test_trains_on_the_graph_models_data(dev):
    """The same [N, num_node, T] data and [N, T] labels feed GConvRNNModel with
    feat_in = 1 (its [N, M, 1, T] view)."""
    import scipy.sparse
    from cnn_graph_amd.gconv_rnn import GConvRNNModel
    m, x, labels = make(dev, optimizer="sgd")
    ring = scipy.sparse.diags([np.ones(C - 1), np.ones(C - 1)], [-1, 1], format="csr", dtype=np.float32)
    ring = (scipy.sparse.identity(C, dtype=np.float32, format="csr") - 0.5 * ring).tocsr()
    g = GConvRNNModel(ring, N, T, 1, num_hidden=H, K=2, keep_prob=1.0, device=dev)
    xs = t(x, dev)
    a, b = m.train_step(xs, labels), g.train_step(xs.view(N, C, 1, T), labels)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
