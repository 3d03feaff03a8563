"""cgcnn.CGCNNModel on the GPU against the float64 restatement tests/cgcnn_ref.py:
every piece of one step on the inputs the GPU itself produced, two whole steps
end to end (logits, loss, every gradient, every parameter after the update), and
predict / evaluate / fit.  Bar: 1e-5 normwise.

Each case takes the first data seed below SEEDS whose float64 forward (both
steps) keeps every ReLU pre-activation and max-pool top-two gap further than
1e-6 of its layer's largest from zero (cgcnn_ref.margins_ok), and then asserts
that the GPU's ReLU masks and argmax agree with float64's everywhere."""
import numpy as np
import pytest
import scipy.sparse

import cgcnn_ref as R
from conftest import case, load_golden
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
SEEDS = 40
REG, MOM, LR = 5e-4, 0.9, 0.05


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def f64(x):
    return x.detach().cpu().numpy().astype(np.float64)


def err(a, ref):
    return O.normwise_err(f64(a).reshape(np.shape(ref)), ref)


_GRAPHS = {}


def graphs(name):
    """(Laplacians, raw input width, perm or None): 'B' the MNIST pyramid of golden_B
    (976 / 488 / 244 / 122 / 61 vertices), 'A' the one-level graph of golden_A (M 100)."""
    if name not in _GRAPHS:
        if name == "B":
            from cnn_graph_amd import coarsening, graph
            g = load_golden("golden_B.npz")
            A = scipy.sparse.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]),
                                        shape=tuple(g["A_shape"]))
            gs, perm = coarsening.coarsen(A, 4, rids=[g[f"rid{i}"] for i in range(4)], verbose=False)
            _GRAPHS[name] = ([graph.laplacian(G, normalized=True) for G in gs], A.shape[0], perm)
        else:
            c = case(load_golden("golden_A.npz"))
            M = c["M"]
            Lt = scipy.sparse.csr_matrix((c["Lt_val"], c["Lt_col"], c["Lt_rowptr"]), shape=(M, M))
            _GRAPHS[name] = ([(Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr()],
                             M, None)
    return _GRAPHS[name]


ARCHS = {
    "a_pyramid_mpool": dict(g="B", N=4, F=[4, 8], K=[3, 3], p=[4, 2], M=[16, 10], brelu="b1relu",
                            pool="mpool1", dropout=1.0),
    "a_pyramid_apool_drop": dict(g="B", N=4, F=[4, 8], K=[3, 3], p=[4, 2], M=[16, 10], brelu="b1relu",
                                 pool="apool1", dropout=0.5),
    "b_b2relu": dict(g="A", N=4, F=[4], K=[5], p=[1], M=[10], brelu="b2relu", pool="mpool1",
                     dropout=1.0),
    "c_softmax": dict(g="A", N=4, F=[], K=[], p=[], M=[10], brelu="b1relu", pool="mpool1",
                      dropout=1.0),
}


def make(dev, a, **kw):
    from cnn_graph_amd import CGCNNModel
    L, _, _ = graphs(a["g"])
    args = dict(regularization=REG, momentum=MOM, learning_rate=LR, decay_rate=0.95, decay_steps=1,
                dropout=a["dropout"], brelu=a["brelu"], pool=a["pool"], device=dev)
    args.update(kw)
    return CGCNNModel(L, a["N"], a["F"], a["K"], a["p"], a["M"], **args)


def net_of(model):
    return dict(laps=[(lv.filt.plan.rowptr, lv.filt.plan.col, lv.filt.plan.val) for lv in model.levels],
                K=model.K, p=model.p, brelu=model.brelu, pool=model.pool, nfc=len(model.fcs),
                reg=model.regularization)


def batch(a, seed):
    _, width, perm = graphs(a["g"])
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((a["N"], width))
    if perm is not None:
        from cnn_graph_amd import coarsening
        x = coarsening.perm_data(x, perm)
    labels = rng.integers(0, a["M"][-1], a["N"])
    labels[0], labels[-1] = 0, a["M"][-1] - 1
    return x.astype(np.float32), labels


def masks_of(model, dev, call):
    """The dropout multipliers the model draws in its training forward number
    ``call`` (0-based), read back through ops.dropout with the same (seed, offset)."""
    from cnn_graph_amd import cgcnn, ops
    if model.keep >= 1.0:
        return None, None
    seeds = [(b + cgcnn._STREAM_STEP * call) & ((1 << 64) - 1) for b in model._drop_base]
    ms = [f64(ops.dropout(torch.ones((model.N, fc.Mout), device=dev), model.keep, s, offset=0))
          for s, fc in zip(seeds, model.fcs[:-1])]
    for m in ms:
        assert set(np.unique(m)) <= {0.0, 1.0 / model.keep} and 0 < (m > 0).mean() < 1
    return ms, seeds


def lr_at(step):
    return LR * 0.95 ** step


def reference_steps(model, dev, x, labels, steps):
    """``steps`` float64 training steps from the model's current parameters:
    [(logits, loss, grads, params after, state)], or None when a margin fails."""
    net = net_of(model)
    params = [f64(v) for v in model.parameters().values()]
    acc = [np.zeros_like(v) for v in params]
    out = []
    for k in range(steps):
        masks, _ = masks_of(model, dev, model._drop_calls + k)
        logits, loss, st = R.forward(x.astype(np.float64), labels, params, net, masks)
        if not R.margins_ok(st, 1e-6):
            return None
        grads, _ = R.backward(st, params, net)
        params, acc = R.momentum_step(params, grads, acc, lr_at(k), MOM, REG, R.regularised(net, params))
        out.append((logits, loss, grads, params, st))
    return out


def pick(model, dev, a, steps):
    for seed in range(SEEDS):
        x, labels = batch(a, seed)
        ref = reference_steps(model, dev, x, labels, steps)
        if ref is not None:
            return x, labels, ref
    raise AssertionError(f"no data seed below {SEEDS} keeps the 1e-6 margin: change the shape")


def assert_no_flips(model, st):
    """The GPU's ReLU masks and pooling argmax are float64's, everywhere."""
    pres = list(st["pre"])
    for lv, rec in zip(model.levels, st["conv"]):
        act = lv.z if lv.z is not None else lv.y
        assert np.array_equal(f64(act) > 0, pres.pop(0) > 0)
        if lv.argmax is not None:
            assert np.array_equal(lv.argmax.cpu().numpy(), rec["arg"])
    for fc in model.fcs[:-1]:
        assert np.array_equal(f64(fc.y) > 0, pres.pop(0) > 0)


@pytest.mark.parametrize("name", list(ARCHS))
def test_two_steps_end_to_end(dev, name):
    a = ARCHS[name]
    model = make(dev, a)
    x, labels, ref = pick(model, dev, a, 2)
    xd = torch.from_numpy(x).to(dev)
    names = list(model.parameters())
    for k, (logits, loss, grads, params, st) in enumerate(ref):
        _, seeds = masks_of(model, dev, model._drop_calls)
        got = model.train_step(xd, labels)
        torch.cuda.synchronize()
        if seeds is not None:
            assert model.drop_seeds == seeds
        assert_no_flips(model, st)
        assert err(model.fcs[-1].y, logits) < TOL, (k, "logits")
        assert abs(float(got) - loss) <= TOL * loss, (k, float(got), loss)
        for n, g, r in zip(names, model.gradients().values(), grads):
            assert err(g, r) < TOL, (k, n, "grad")
        for n, p, r in zip(names, model.parameters().values(), params):
            assert err(p, r) < TOL, (k, n, "param")
    assert float(model.ema[2]) == 2.0 and model.step_count == 2
    # the L2 term reaches the regularised variables only: without it they end elsewhere
    assert model.reg_begin + model.reg_n == model.flat.numel()
    assert names[-2:] == ["logits/weights", "logits/bias"]


@pytest.mark.parametrize("name", list(ARCHS))
def test_every_piece_of_one_step(dev, name):
    """Forward, loss and backward launch by launch, each against float64 on the
    inputs the GPU itself produced (the per-filter method of test_gpu_model.py)."""
    a = ARCHS[name]
    model = make(dev, a)
    x, labels, ref = pick(model, dev, a, 1)
    net = net_of(model)
    convs, fcs = R.split_params(net, [f64(v) for v in model.parameters().values()])
    masks, _ = masks_of(model, dev, model._drop_calls)
    xd = torch.from_numpy(x).to(dev)
    s = model._stream(None)
    out = model.forward(xd, dropout=True)
    model._loss(out, labels, s)
    model.backward(model.dout, s)
    torch.cuda.synchronize()
    assert_no_flips(model, ref[0][4])
    mpool = model.pool == "mpool1"
    # ---- forward ----
    inp, inputs = x.astype(np.float64)[:, :, None], []
    bases = []
    for lv, (W, b), lap, K in zip(model.levels, convs, net["laps"], net["K"]):
        inputs.append(inp)
        A, y = R.conv_forward(inp, lap, W, K)
        bases.append(A)
        assert err(lv.y, y if b is not None else np.maximum(y, 0)) < TOL
        act = f64(lv.y)
        if b is not None:
            assert err(lv.z, np.maximum(act + b, 0)) < TOL
            act = f64(lv.z)
        if lv.p > 1:
            if mpool:
                py, parg = O.mpool1_forward(act, lv.p)
                assert np.array_equal(lv.argmax.cpu().numpy(), parg)
                assert np.array_equal(f64(lv.pooled), py)
            else:
                assert err(lv.pooled, R.apool_forward(act, lv.p)) < TOL
            act = f64(lv.pooled)
        inp = act
    for j, (fc, (W, b)) in enumerate(zip(model.fcs, fcs)):
        pre = f64(fc.x).reshape(model.N, -1) @ W + b
        assert err(fc.y, np.maximum(pre, 0) if fc.relu else pre) < TOL
        if fc.drop is not None:
            assert err(fc.drop, f64(fc.y) * masks[j]) < TOL
    ce, dlogits = R.softmax_xent(f64(out), labels)
    reg = sum(0.5 * (v ** 2).sum() for pair in fcs for v in pair)
    assert abs(float(model.loss) - (ce + REG * reg)) <= TOL * (ce + REG * reg)
    assert REG * reg > 10 * TOL * ce  # the term is visible at the bar
    # ---- backward ---- (the logits layer's dz is dlogits, in place)
    assert err(model.dout, dlogits) < TOL
    dy = f64(model.dout)
    for j in range(len(fcs) - 1, -1, -1):
        fc, (W, b) = model.fcs[j], fcs[j]
        if fc.ddrop is not None:
            assert err(fc.ddrop, dy * masks[j]) < TOL
            dy = f64(fc.ddrop)
        if fc.relu:
            assert err(fc.dz, dy * (f64(fc.y) > 0)) < TOL
            dy = f64(fc.dz)
        assert err(fc.dW, f64(fc.x).reshape(model.N, -1).T @ dy) < TOL
        assert err(fc.db, dy.sum(axis=0)) < TOL
        if fc.dx is not None:
            assert err(fc.dx, dy @ W.T) < TOL
            dy = f64(fc.dx)
        else:
            assert j == 0 and not model.levels
    for i in range(len(convs) - 1, -1, -1):
        lv, (W, b) = model.levels[i], convs[i]
        N, M, Fin = inputs[i].shape
        dy = dy.reshape(N, M // lv.p, lv.F)
        if lv.p > 1:
            want = (R.mpool_backward(dy, lv.argmax.cpu().numpy(), M) if mpool
                    else R.apool_backward(dy, lv.p))
            assert err(lv.dpool, want) < TOL
            dy = f64(lv.dpool)
        act = f64(lv.z if lv.z is not None else lv.y)
        assert err(lv.dz, dy * (act > 0)) < TOL
        dz = f64(lv.dz)
        if b is not None:
            assert err(lv.db, dz.sum(axis=0, keepdims=True)) < TOL
        dx, dW = R.conv_backward(dz, bases[i], W, net["laps"][i], net["K"][i], N, M, Fin)
        assert err(lv.dW, dW) < TOL
        if i > 0:
            assert err(lv.dx, dx) < TOL
            dy = f64(lv.dx)
        else:
            assert lv.dx is None  # conv1 reads data


def test_momentum_zero_paths(dev):
    """momentum == 0: cg_sgd_update without the L2 term, cg_momentum_update with it."""
    a = ARCHS["c_softmax"]
    for reg in (0.0, REG):
        model = make(dev, a, momentum=0.0, regularization=reg)
        x, labels = batch(a, 0)
        net = net_of(model)
        params = [f64(v) for v in model.parameters().values()]
        _, _, st = R.forward(x.astype(np.float64), labels, params, net)
        grads, _ = R.backward(st, params, net)
        want, _ = R.momentum_step(params, grads, [np.zeros_like(v) for v in params], LR, 0.0, reg,
                                  R.regularised(net, params))
        model.train_step(torch.from_numpy(x).to(dev), labels)
        torch.cuda.synchronize()
        for p, r in zip(model.parameters().values(), want):
            assert err(p, r) < TOL
        assert float(model.accum.abs().max()) == 0.0  # the slot is not touched


def test_predict_evaluate_shapes_with_a_ragged_last_batch(dev):
    a = ARCHS["b_b2relu"]
    model = make(dev, a)
    rng = np.random.default_rng(1)
    size = 2 * a["N"] + 1
    data = rng.standard_normal((size, 100)).astype(np.float32)
    labels = rng.integers(0, 10, size)
    before = model.flat.clone()
    preds = model.predict(data)
    assert preds.shape == (size,) and preds.dtype == np.int64
    preds2, loss = model.predict(data, labels)
    assert np.array_equal(preds, preds2) and np.isfinite(loss)
    # float64 on the same parameters: predictions, and the loss with its padded rows
    net = net_of(model)
    params = [f64(v) for v in model.parameters().values()]
    total, want = 0.0, []
    for b0 in range(0, size, a["N"]):
        xb = np.zeros((a["N"], 100))
        lb = np.zeros(a["N"], np.int64)
        n = min(a["N"], size - b0)
        xb[:n], lb[:n] = data[b0:b0 + n], labels[b0:b0 + n]
        logits, l, _ = R.forward(xb, lb, params, net)
        s = np.sort(logits, axis=1)
        assert (s[:n, -1] - s[:n, -2]).min() > 1e-4
        want += logits[:n].argmax(axis=1).tolist()
        total += l
    assert preds.tolist() == want
    assert abs(loss - total * a["N"] / size) <= TOL * loss
    string, acc, f1, loss2, preds3 = model.evaluate(data, labels)
    assert loss2 == loss and np.array_equal(preds3, preds)
    assert abs(acc - 100.0 * (np.array(want) == labels).mean()) < 1e-9
    assert 0.0 <= f1 <= 100.0 and string.startswith("accuracy: ")
    assert torch.equal(model.flat, before) and model.step_count == 0 and float(model.ema[2]) == 0.0


def test_fit_learns_a_two_class_problem(dev):
    from cnn_graph_amd import CGCNNModel
    L, M, _ = graphs("A")
    rng = np.random.default_rng(4)

    def dataset(n):
        y = rng.integers(0, 2, n)
        x = 0.3 * rng.standard_normal((n, M))
        x[:, :M // 2] += np.where(y == 1, 1.0, -1.0)[:, None]
        return x.astype(np.float32), y

    xt, yt = dataset(67)
    xv, yv = dataset(21)  # a ragged last validation batch
    model = CGCNNModel(L, 16, [4], [3], [1], [8, 2], regularization=REG, momentum=MOM,
                       learning_rate=0.02, decay_rate=0.95, decay_steps=10, dropout=0.5, device=dev)
    _, start, _, _, _ = model.evaluate(xv, yv)
    accs, losses, t_step = model.fit(xt, yt, xv, yv, num_epochs=10, eval_frequency=20, rng=3,
                                     verbose=False)
    num_steps = int(10 * 67 / 16)
    assert len(accs) == len(losses) == num_steps // 20 + (1 if num_steps % 20 else 0)
    assert model.step_count == num_steps and t_step > 0
    assert accs[-1] > start, (start, accs)
    assert all(np.isfinite(losses))
    with pytest.raises(ValueError):
        model.fit(xt, np.where(yt == 1, 2, 0), xv, yv, num_epochs=1, verbose=False)  # class 2 of 2
