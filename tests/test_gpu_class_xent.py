"""cg_class_xent_ema on the GPU against float64: the loss with its L2 term, dlogits,
the moving average, the prediction and the correct count.  Bars: 1e-5 normwise
for dlogits, |loss - ref| <= 1e-5 ref."""
import numpy as np
import pytest

from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
SHAPES = [(1, 1), (1, 2), (3, 10), (37, 10), (5, 65), (4, 300), (128, 20)]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _ref(logits, labels, params=None, rb=0, rn=0, scale=0.0):
    x = r32(logits)
    N = x.shape[0]
    z = x - x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=1))
    ce = lse - z[np.arange(N), labels]
    d = np.exp(z - lse[:, None])
    d[np.arange(N), labels] -= 1.0
    loss = ce.mean()
    if rn:
        loss += scale * 0.5 * (r32(params)[rb:rb + rn] ** 2).sum()
    return loss, d / N


def _case(N, C, seed, scale=1.0):
    """Logits whose float64 top-two gap is > 1e-4 in every row, labels with 0 and C - 1."""
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((N, C))).astype(np.float32)
    labels = rng.integers(0, C, N)
    labels[0] = 0
    labels[-1] = C - 1
    if C > 1:
        s = np.sort(r32(x), axis=1)
        assert (s[:, -1] - s[:, -2]).min() > 1e-4
    if N > 2:  # some rows are predicted right, so the count is not trivially 0
        labels[1:-1:2] = r32(x).argmax(axis=1)[1:-1:2]
    return x, labels


def _close(loss, ref):
    return abs(float(loss) - ref) <= TOL * abs(ref)


@pytest.mark.parametrize("N,C", SHAPES)
def test_loss_gradient_prediction_vs_float64(dev, N, C):
    from cnn_graph_amd import ops
    x, labels = _case(N, C, seed=N * 1000 + C)
    r = ops.class_xent_call(t(x, dev), ops.class_labels(labels, C, dev), want_pred=True, check=True)
    torch.cuda.synchronize()
    loss, d = _ref(x, labels)
    if (N, C) == (1, 1):
        assert float(r.loss) == 0.0 and float(r.dlogits.abs().max()) == 0.0
    else:
        assert _close(r.loss, loss), (float(r.loss), loss)
        assert O.normwise_err(r.dlogits.cpu().numpy(), d) < TOL
    want = r32(x).argmax(axis=1)
    assert np.array_equal(r.pred.cpu().numpy(), want)
    assert int(r.correct) == int((want == labels).sum())
    assert int(r.status) == 0


def test_large_logits_do_not_overflow(dev):
    from cnn_graph_amd import ops
    x, labels = _case(37, 10, seed=5, scale=50.0)
    with np.errstate(over="ignore"):
        assert np.exp(np.float32(x.max())) == np.inf  # an unshifted exp would overflow
    r = ops.class_xent_call(t(x, dev), ops.class_labels(labels, 10, dev), want_pred=True)
    torch.cuda.synchronize()
    loss, d = _ref(x, labels)
    assert np.isfinite(float(r.loss)) and _close(r.loss, loss)
    assert O.normwise_err(r.dlogits.cpu().numpy(), d) < TOL
    assert np.array_equal(r.pred.cpu().numpy(), r32(x).argmax(axis=1))


def test_first_maximum_wins_ties(dev):
    from cnn_graph_amd import ops
    x = np.zeros((3, 70), np.float32)
    x[0, [5, 69]] = 2.0     # both in lane 5's columns
    x[1, [66, 3]] = 1.0     # the later column sits in an earlier lane
    x[2, :] = -1.0          # all equal
    r = ops.class_xent_call(t(x, dev), ops.class_labels([5, 3, 1], 70, dev), want_pred=True)
    torch.cuda.synchronize()
    assert r.pred.cpu().tolist() == [5, 3, 0]
    assert int(r.correct) == 2


@pytest.mark.parametrize("rn", [0, 1, 1027])
def test_l2_term_over_an_unaligned_range(dev, rn):
    from cnn_graph_amd import ops
    x, labels = _case(37, 10, seed=11)
    rng = np.random.default_rng(rn)
    params = rng.standard_normal(1500).astype(np.float32)
    rb = 3  # odd: the range starts 12 bytes into the buffer
    r = ops.class_xent_call(t(x, dev), ops.class_labels(labels, 10, dev), params=t(params, dev),
                            reg_begin=rb, reg_n=rn, reg_scale=5e-4)
    torch.cuda.synchronize()
    loss, d = _ref(x, labels, params, rb, rn, 5e-4)
    plain, _ = _ref(x, labels)
    assert _close(r.loss, loss)
    if rn == 1027:
        assert not _close(r.loss, plain)  # the term is visible at the bar
    assert O.normwise_err(r.dlogits.cpu().numpy(), d) < TOL  # the gradient has no L2 part


def test_moving_average_over_three_calls(dev):
    from cnn_graph_amd import ops
    ema = torch.zeros(3, device=dev)
    biased, losses = 0.0, []
    for step in range(1, 4):
        x, labels = _case(37, 10, seed=20 + step)
        r = ops.class_xent_call(t(x, dev), ops.class_labels(labels, 10, dev), ema=ema)
        torch.cuda.synchronize()
        losses.append(_ref(x, labels)[0])
        biased = biased - (biased - losses[-1]) * 0.1
        avg = biased / (1.0 - 0.9 ** step)  # zero-debiased, as cg_mse_loss_ema
        e = ema.cpu().numpy().astype(np.float64)
        assert abs(e[0] - biased) <= TOL * biased and abs(e[1] - avg) <= TOL * avg
        assert e[2] == step


def test_two_calls_agree_bitwise(dev):
    from cnn_graph_amd import ops
    x, labels = _case(128, 20, seed=31)
    params = t(np.random.default_rng(2).standard_normal(5000), dev)
    xs, ls = t(x, dev), ops.class_labels(labels, 20, dev)
    a = ops.class_xent_call(xs, ls, params=params, reg_begin=1, reg_n=4999, reg_scale=1e-3)
    b = ops.class_xent_call(xs, ls, params=params, reg_begin=1, reg_n=4999, reg_scale=1e-3)
    torch.cuda.synchronize()
    assert torch.equal(a.loss, b.loss) and torch.equal(a.dlogits, b.dlogits)


def test_evaluation_form_and_autograd(dev):
    from cnn_graph_amd import ops
    x, labels = _case(37, 10, seed=41)
    xs, ls = t(x, dev), ops.class_labels(labels, 10, dev)
    full = ops.class_xent_call(xs, ls, want_pred=True)
    ev = ops.class_xent_call(xs, ls, need_grad=False, want_pred=True)  # dlogits == NULL
    torch.cuda.synchronize()
    assert ev.dlogits is None and torch.equal(ev.loss, full.loss) and torch.equal(ev.pred, full.pred)
    assert int(ev.correct) == int(full.correct)
    xg = xs.clone().requires_grad_(True)
    loss = ops.class_xent(xg, labels)
    (3.0 * loss).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), full.loss)
    assert O.normwise_err(xg.grad.cpu().numpy(), 3.0 * _ref(x, labels)[1]) < TOL
    with torch.no_grad():
        assert torch.equal(ops.class_xent(xs, labels), full.loss)


def test_out_of_range_label_is_reported_not_followed(dev):
    """A device label the host never saw: the row is NaN, the status word names
    it, and nothing outside the arguments is touched (the neighbours are intact)."""
    from cnn_graph_amd import ops
    x, labels = _case(5, 10, seed=51)
    bad = torch.tensor(labels.astype(np.int32), device=dev)
    bad[3], bad[4] = 10, -7
    guard = torch.full((3, 5, 10), 7.0, device=dev)
    r = ops.class_xent_call(t(x, dev), bad, out_dlogits=guard[1], want_pred=True)
    torch.cuda.synchronize()
    assert int(r.status) == 4  # the first such row + 1
    d = guard[1].cpu().numpy()
    assert np.isnan(d[3:]).all() and np.isfinite(d[:3]).all() and np.isnan(float(r.loss))
    assert float(guard[0].min()) == 7.0 and float(guard[2].max()) == 7.0
    assert O.normwise_err(d[:3], _ref(x, labels)[1][:3]) < TOL
    with pytest.raises(ValueError):
        ops.class_xent_call(t(x, dev), bad, check=True)
