"""GConvNetModel (cnn_graph_amd/gconv_net.py) on the GPU against the float64
restatement tests/gconv_net_ref.py: output, loss, every dW and the parameters
after Adam steps, at the project's 1e-5 normwise bar.

``inference_gconv`` is smooth everywhere, so three whole steps are compared
end to end.  The two networks with ReLU are compared end to end on a case whose
seed is chosen on the CPU so that no ReLU pre-activation of the float64 reference
lies within 1e-6 of zero relative to its layer's largest (asserted); the ReLU
masks of the GPU run are compared with the reference's and the flips counted
(asserted zero: a flip would pass or drop a whole upstream-gradient entry).

Adam's update lr_t g / (|g| + eps) is ill-conditioned in g where |g| is near eps =
1e-8: a rounding dg of a gradient entry moves its weight by lr_t eps dg / (|g| +
eps)^2.  The labels are scaled by 100 so that the gradients sit far above eps, and
every step asserts on the float64 side that a dg of 1e-6 max |g| (ten times fp32's
rounding) moves no weight by more than a fifth of the bar."""
import numpy as np
import pytest
import scipy.sparse

import gconv_net_ref as GR
from conftest import case, load_golden
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
MARGIN = 1e-6


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def f64(x):
    return x.detach().cpu().numpy().astype(np.float64)


_L = {}


def golden_L(name):
    """(L with rescale_L(L, 2) == the golden L~, (rowptr, col, val) of L~), built once:
    the plan cache keys on the matrix object."""
    if name not in _L:
        c = case(load_golden(name))
        M = c["M"]
        Lt = scipy.sparse.csr_matrix((c["Lt_val"], c["Lt_col"], c["Lt_rowptr"]), shape=(M, M))
        L = (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr()
        _L[name] = L
    return _L[name]


def make(dev, graph, infer_func, N, T, H, K, R, seed, lr=1e-3):
    from cnn_graph_amd.gconv_net import GConvNetModel
    model = GConvNetModel(golden_L(graph), N, T=T, num_hidden=H, K=K, conv_layer_num=R, out_features=2,
                          infer_func=infer_func, learning_rate=lr, decay_rate=0.95, decay_steps=2,
                          device=dev, seed=seed)
    lap = (model.plan.rowptr, model.plan.col, model.plan.val.astype(np.float64))
    assert model.names == GR.variable_names(infer_func, R)
    assert [tuple(w.shape) for w in model.W] == GR.shapes(infer_func, T, H, K, R, 2)
    return model, lap


def data(model, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((model.N, model.M, model.C)).astype(np.float32)
    labels = (100 * rng.standard_normal((model.N, model.M, 2))).astype(np.float32)
    return x, labels


def adam_condition(grads, weights, lr_t, eps=1e-8):
    """The largest weight change, relative to max |W| of its variable, that a
    gradient rounding of 1e-6 max |g| causes through Adam's first steps."""
    worst = 0.0
    for g, w in zip(grads, weights):
        dg = 1e-6 * np.abs(g).max()
        worst = max(worst, float((lr_t * eps * dg / (np.abs(g) + eps) ** 2).max() / np.abs(w).max()))
    return worst


def steps_vs_reference(model, lap, infer_func, x, labels, T, K, R, nsteps, dev, chain=True):
    """chain: the float64 reference runs its own chain of steps from the initial
    weights (the smooth network).  Otherwise tests/test_gpu_model.py's method for
    networks with ReLU: every step's reference starts from the GPU's weights, and
    the update is checked as the oracle's Adam of the GPU's gradient."""
    params = GR.unflat([f64(w) for w in model.W], infer_func)
    state = [(np.zeros_like(w), np.zeros_like(w)) for w in GR.flat(params, infer_func)]
    xd, ld = t(x, dev), t(labels, dev)
    for step in range(1, nsteps + 1):
        if not chain:
            params = GR.unflat([f64(w) for w in model.W], infer_func)
        prev, state0 = GR.flat(params, infer_func), state
        ref_out, _ = GR.forward(x.astype(np.float64), params, infer_func, lap, K, R, T)
        loss = model.train_step(xd, ld)
        torch.cuda.synchronize()
        out = model.out if infer_func == GR.EXPAND else model.nets[0].out[-1]
        e_out = O.normwise_err(f64(out), ref_out)
        rl, rg, params, state = GR.train_step(x.astype(np.float64), labels, params, infer_func, lap, K, R, T,
                                              state, step, model.learning_rate(step - 1))
        if chain:
            cond = adam_condition(rg, prev, 4 * model.learning_rate(step - 1))
            assert cond < 0.2 * TOL, (step, cond)
        else:
            upd = [O.adam_step(w0, f64(g), m, v, step, lr=model.learning_rate(step - 1))
                   for w0, g, (m, v) in zip(prev, model.dW, state0)]
            params = GR.unflat([u[0] for u in upd], infer_func)
            state = [(u[1], u[2]) for u in upd]
        e_g = {n: O.normwise_err(f64(g), r) for n, g, r in zip(model.names, model.dW, rg)}
        e_w = {n: O.normwise_err(f64(w), r) for n, w, r in zip(model.names, model.W, GR.flat(params, infer_func))}
        print(f"{infer_func} step {step}: out {e_out:.2e} loss {float(loss.item()):.6f} / {rl:.6f} "
              f"max dW {max(e_g.values()):.2e} max W {max(e_w.values()):.2e}")
        assert e_out < TOL, step
        assert abs(float(loss.item()) - rl) <= 1e-5 * rl, (step, float(loss.item()), rl)
        for n, e in e_g.items():
            assert e < TOL, (step, "dW", n, e)
        for n, e in e_w.items():
            assert e < TOL, (step, "W", n, e)


def test_inference_gconv_three_steps_vs_reference(dev):
    """Graph A, N 4, C 8, T (2, 1, 1), hidden 8, K 3, 2 residual layers: tanh everywhere."""
    infer_func, N, T, H, K, R = "inference_gconv", 4, (2, 1, 1), 8, 3, 2
    model, lap = make(dev, "golden_A.npz", infer_func, N, T, H, K, R, seed=5)
    assert model.C == 8 and model.M == 100
    x, labels = data(model, 9)
    steps_vs_reference(model, lap, infer_func, x, labels, T, K, R, 3, dev)


def _relu_case(model, lap, infer_func, T, K, R):
    """The first data seed whose float64 forward keeps every ReLU pre-activation
    further than MARGIN (relative to its layer's largest) from zero."""
    params = GR.unflat([f64(w) for w in model.W], infer_func)
    for seed in range(100, 140):
        x, labels = data(model, seed)
        _, fw = GR.forward(x.astype(np.float64), params, infer_func, lap, K, R, T)
        if GR.relu_margins(fw) > MARGIN:
            return x, labels, params, fw
    raise AssertionError("no seed keeps the ReLU pre-activations away from zero")


def _mask_flips(model, fw, infer_func):
    flips = total = 0
    for net, cache in zip(model.nets, fw["caches"]):
        for out, (_, _, _, ref_out, act) in zip(net.out, cache):
            if act == "relu":
                flips += int(np.count_nonzero((f64(out) > 0) != (ref_out > 0)))
                total += ref_out.size
    return flips, total


@pytest.mark.parametrize("infer_func,graph,N", [("inference_gconv_period_no_expand", "golden_A.npz", 4),
                                                ("inference_gconv_period_expand", "golden_A.npz", 4),
                                                ("inference_gconv_period_expand", "golden_B.npz", 2)])
def test_relu_networks_step_vs_reference(dev, infer_func, graph, N):
    """golden_B: M = 976 (the MNIST graph with its empty rows), N 2 -- the fast
    kernels' row classes, the ragged tile and the concat of three width-2 outputs."""
    T, H, K, R = (2, 1, 1), 8, 3, 2
    model, lap = make(dev, graph, infer_func, N, T, H, K, R, seed=7)
    x, labels, params, fw = _relu_case(model, lap, infer_func, T, K, R)
    assert GR.relu_margins(fw) > MARGIN
    out = model.forward(t(x, dev))
    torch.cuda.synchronize()
    flips, total = _mask_flips(model, fw, infer_func)
    print(f"{infer_func} {graph}: ReLU mask flips {flips} of {total}")
    assert flips == 0
    steps_vs_reference(model, lap, infer_func, x, labels, T, K, R, 2 if graph == "golden_A.npz" else 1, dev,
                       chain=False)
    assert tuple(out.shape) == (N, model.M, 2)


def test_fourier_no_expand_runs_and_tanh_networks_are_refused(dev):
    from cnn_graph_amd.gconv_net import GConvNetModel
    L = golden_L("golden_A.npz")
    model = GConvNetModel(L, 2, T=(1, 1, 1), num_hidden=4, conv_layer_num=1, filter="fourier_conv",
                          infer_func="inference_gconv_period_no_expand", device=dev)
    x, labels = data(model, 3)
    l0 = float(model.train_step(t(x, dev), t(labels, dev)).item())
    for _ in range(5):
        l1 = float(model.train_step(t(x, dev), t(labels, dev)).item())
    assert np.isfinite(l0) and l1 < l0
    assert [tuple(w.shape) for w in model.W] == [(100, 4, 6), (100, 4, 4), (100, 4, 4), (100, 2, 4)]


@pytest.mark.parametrize("infer_func", GR.INFER_FUNCS)
def test_predict_evaluate_fit(dev, infer_func):
    """FlatTrainer's predict / evaluate / fit through the new forward: the
    reference's tuple shapes (lib/graph_model.py:64-197)."""
    N, T = 4, (1, 1, 1)
    model, _ = make(dev, "golden_A.npz", infer_func, N, T, 4, 2, 1, seed=3)
    rng = np.random.default_rng(1)
    S = 10  # a ragged last batch
    d = rng.standard_normal((S, model.M, model.C)).astype(np.float32)
    l = rng.standard_normal((S, model.M, 2)).astype(np.float32)
    p = np.asarray(f64(torch.as_tensor(model.predict(d))))
    assert p.shape == (S, model.M, 2)
    p2, loss = model.predict(d, l)
    assert np.array_equal(p, f64(torch.as_tensor(p2))) and np.isfinite(loss)
    string, mse, zero, loss2, preds = model.evaluate(d, l)
    assert isinstance(string, str) and zero == 0 and tuple(preds.shape) == (S, model.M, 2)
    assert np.isfinite(mse) and loss2 == loss
    acc, losses, t_step = model.fit(d, l, d[:4], l[:4], num_epochs=1.6, eval_frequency=2, rng=0,
                                    verbose=False)
    assert model.step_count == 4 and len(acc) == len(losses) == 2 and t_step > 0


def _filter_inputs(net, x):
    """(input, residual) of every filter of a _ResNet as the GPU ran it: the net's
    own saved outputs (conv_init, R residual layers of two filters, the last filter)."""
    ins, res = [x], [None]
    h, li = net.out[0], 1
    for _ in range(net.R):
        ins += [h, net.out[li]]
        res += [None, h]
        h, li = net.out[li + 1], li + 2
    ins.append(h)
    res.append(None)
    return ins, res


@pytest.mark.parametrize("infer_func,graph,N", [("inference_gconv_period_no_expand", "golden_A.npz", 4),
                                                ("inference_gconv_period_expand", "golden_A.npz", 4),
                                                ("inference_gconv_period_expand", "golden_B.npz", 2)])
def test_relu_networks_per_filter_vs_reference(dev, infer_func, graph, N):
    """EVERY filter of one training step at the 1e-5 bar, each on the inputs,
    residuals and upstream gradients the GPU itself produced (the method of
    tests/test_gpu_model.py for ResGNN): y = act(cheb(x) W + res), dz = dy act'(y)
    where the schedule keeps it (every output_layer_j with its ReLU included), dW,
    and dx (accumulated where the schedule accumulates) against float64.  For the
    three-branch network also the seams: the concat and its split bit for bit, and
    the merge_layer filter's y, dx and dW."""
    T, H, K, R = (2, 1, 1), 8, 3, 2
    model, lap = make(dev, graph, infer_func, N, T, H, K, R, seed=7)
    M = model.M
    x, labels = data(model, 100)
    xt = t(x, dev)
    calls = {id(net): [] for net in model.nets}
    saved_b = {}
    for net in model.nets:
        saved_b[id(net)] = run_b = net._b

        def recording_b(li, dy, dz, dx, dx_acc, s, net=net, run_b=run_b):
            before = dx.clone() if (dx is not None and dx_acc) else None
            dy_in = dy.clone()
            run_b(li, dy, dz, dx, dx_acc, s)
            calls[id(net)].append((li, dy_in, None if dz is None else dz.clone(),
                                   None if dx is None else dx.clone(), before, net.dW[li].clone()))

        net._b = recording_b
    Wprev = [[f64(w) for w in net.W] for net in model.nets]
    Wm_prev = f64(model.merge_W) if infer_func == GR.EXPAND else None
    model.train_step(xt, t(labels, dev))
    torch.cuda.synchronize()
    worst = {}

    def bar(what, name, got, ref):
        err = O.normwise_err(f64(got), ref)
        worst[what] = max(worst.get(what, 0.0), err)
        assert err < TOL, (name, what, err)

    for j, net in enumerate(model.nets):
        xin = xt if infer_func != GR.EXPAND or model.x_b[j] is None else model.x_b[j]
        if infer_func == GR.EXPAND:
            a, b = model.columns[j]
            assert torch.equal(xin, xt[:, :, a:b].contiguous())
        ins, res = _filter_inputs(net, xin)
        As = []
        for li, (_, fi, fo, act) in enumerate(net.layers):
            A, y = GR.cheb_conv64(f64(ins[li]), lap, Wprev[j][li], K)
            pre = y + f64(res[li]) if res[li] is not None else y
            bar("y", net.names[li], net.out[li], GR._act(pre, act))
            As.append(A)
        assert [c[0] for c in calls[id(net)]] == list(range(len(net.layers) - 1, -1, -1))
        for li, dy, dz, dx, before, dW in calls[id(net)]:
            _, fi, fo, act = net.layers[li]
            dz_ref = GR._dact(f64(dy), f64(net.out[li]), act)
            if act != "none":
                assert dz is not None, net.names[li]  # (the last filter's dz_last too)
            if dz is not None and before is None:
                # (where dz doubles as the dx accumulator it holds dz + dx afterwards: checked as dx)
                if dx is None or dz.data_ptr() != dx.data_ptr():
                    bar("dz", net.names[li], dz, dz_ref)
            rdx, rdW = O.cheb_backward(dz_ref, As[li], Wprev[j][li], lap[0], lap[1], lap[2], N, M, fi, K)
            bar("dW", net.names[li], dW, rdW)
            if dx is not None:
                bar("dx", net.names[li], dx, rdx + (f64(before) if before is not None else 0.0))
        net._b = saved_b[id(net)]
    if infer_func == GR.EXPAND:
        F = model.Fout
        assert torch.equal(model.cat, torch.cat([n.out[-1] for n in model.nets], dim=2))
        A, y = GR.cheb_conv64(f64(model.cat), lap, Wm_prev, K)
        bar("merge y", "merge_layer", model.out, y)
        rdx, rdW = O.cheb_backward(f64(model.dout), A, Wm_prev, lap[0], lap[1], lap[2], N, M, 3 * F, K)
        bar("merge dx", "merge_layer", model.dcat, rdx)
        bar("merge dW", "merge_layer", model.merge_dW, rdW)
        for j, d in enumerate(model.d_b):
            assert torch.equal(d, model.dcat[:, :, j * F:(j + 1) * F].contiguous()), j
    print(f"{infer_func} {graph}: worst per-filter errors", {k: f"{v:.2e}" for k, v in worst.items()})


def test_single_network_on_another_column_count(dev):
    """inference_gconv reads all columns of x whatever T is: in_features = 5."""
    from cnn_graph_amd.gconv_net import GConvNetModel
    model = GConvNetModel(golden_L("golden_A.npz"), 2, T=(1, 1, 1), num_hidden=4, K=2, conv_layer_num=1,
                          in_features=5, device=dev)
    assert model.C == 5 and tuple(model.W[0].shape) == (10, 4)
    x, labels = data(model, 4)
    assert x.shape == (2, 100, 5)
    l0 = float(model.train_step(t(x, dev), t(labels, dev)).item())
    l1 = float(model.train_step(t(x, dev), t(labels, dev)).item())
    assert np.isfinite(l0) and l1 < l0
