"""The closeness / period / trend gconv-LSTM networks on device
(cnn_graph_amd.glstm_period.GLSTMPeriodModel) against the float64 restatement
(tests/glstm_period_ref.py), fed the model's own mask bits.

Bar: normwise error max|a - ref| / max|ref| <= 1e-5, the project's model-level
bar; every case asserts max|a_z| < AZ_MAX in the reference (the tan gate).  The
ReLU head needs no special care here, as in tests/test_gpu_glstm_gconv.py: the
normwise measure weighs a flipped pre-activation of size ~1e-7 against the
largest entry.  Shapes: ring-with-chords graphs of M = 17 and 40, N = 3,
T = (3, 2, 4) (unequal on purpose)."""
import numpy as np
import pytest

import dp_harness as DP
import fourier_edge_cases as FE
import glstm_gconv_ref as GR
import glstm_period_dp_worker as Wk
import glstm_period_ref as PR
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
N, T, F, OUT = 3, (3, 2, 4), 2, 2
r32 = GR.r32
EXPAND, GCONV1 = "inference_glstm_period_expand", "inference_glstm_period_expand_gconv1"
GCONV3, SPLIT = "inference_glstm_period_expand_gconv3", "inference_glstm_gconv_split"


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


_LAPS = {}


def laplacian(M):
    if M not in _LAPS:
        _LAPS[M] = GR.ring_chords_laplacian(M)
    return _LAPS[M]


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def npy(a):
    return a.detach().cpu().numpy()


def f64(a):
    return npy(a).astype(np.float64)


def check(name, got, ref):
    err = O.normwise_err(npy(got) if torch.is_tensor(got) else got, ref)
    print(f"{name}: normwise err {err:.3e}")
    assert err <= TOL, (name, err)


def make_model(dev, infer_func, filter, M, H, K=2, layers=1, R=1, keep=0.8, seed=5, Ts=T, **kw):
    from cnn_graph_amd import GLSTMPeriodModel
    return GLSTMPeriodModel(laplacian(M), N, Ts, F, num_hidden=H, K=K, layer_count=layers,
                            conv_layer_num=R, out_features=OUT, keep_prob=keep, filter=filter,
                            infer_func=infer_func, device=dev, seed=seed, **kw)


def ref_parts(m):
    """(filt, mode, branches, merge) of a model as float64."""
    filt = ("fourier_conv", f64(m.U)) if m.filter == "fourier_conv" else \
        ("cheby_conv", GR.cheb_lap(laplacian(m.M)), m.K)
    branches = [[tuple(f64(p) for p in (c.Wx, c.Wh, c.b)) for c in cells] for cells in m.cells]
    if m.concat:
        return filt, "concat", branches, [f64(w) for w in m.head_W]
    return filt, "weights", branches, [(f64(W), f64(w)) for W, w in zip(m.fc_W, m.merge_w)]


def next_mults(m):
    """The multipliers the NEXT dropped forward will apply, from the wrappers' own seeds."""
    from cnn_graph_amd.gconv_lstm import DropoutWrapper
    if not isinstance(m.wrapped[0][0], DropoutWrapper):
        return None
    out = []
    for wrapped, tb in zip(m.wrapped, m.T):
        ms = []
        for li, w in enumerate(wrapped):
            seed = GR.wrapper_call_seed(w._seed, w._calls + 1)
            if li < len(wrapped) - 1:
                ms.append(GR.drop_mult(seed, (tb, m.N, m.M, m.H), w.output_keep_prob))
            else:
                ms.append(GR.drop_mult(seed, (m.N, m.M, m.H), w.output_keep_prob,
                                       offset=(tb - 1) * m.N * m.M * m.H))
        out.append(ms)
    return out


def batch(m, seed=3, extra=0):
    rng = np.random.default_rng(seed)
    x = r32(0.5 * rng.standard_normal((m.N, m.M, m.C + extra)))
    labels = r32(rng.standard_normal((m.N, m.M, OUT)))
    return x, labels


def model_vs_reference(dev, m):
    filt, mode, branches, merge = ref_parts(m)
    x, _ = batch(m, 9)
    dout = r32(np.random.default_rng(10).standard_normal((m.N, m.M, OUT)) / (m.N * m.M))
    mults = next_mults(m)
    xt = t(x, dev).requires_grad_(True)
    out = m.forward(xt).clone()
    m.backward(t(dout, dev))
    torch.cuda.synchronize()
    ref_out, fw = PR.forward(x, m.T, F, branches, merge, filt, mode, m.R, "reference", mults)
    az = PR.max_az(fw, "reference")
    print(f"max|a_z| = {az:.3f}")
    assert az < FE.AZ_MAX
    dx, dbr, dm = PR.backward(dout, fw, m.T, F, branches, merge, filt, mode, m.R, "reference", mults)
    check("out", out, ref_out)
    grads = m.gradients()
    refs = PR.flat_params(dbr, dm, mode)
    assert list(grads) == m.names and len(refs) == len(m.names)
    for (name, g), ref in zip(grads.items(), refs):
        check(name, g, ref)
    check("dL/dx", xt.grad, dx)
    if mults is not None:  # the masks are the branches' own: no two branches share bits
        last = [ms[-1] for ms in mults]
        assert not np.array_equal(last[0], last[1]) and not np.array_equal(last[0], last[2])


CASES = [  # (filter, H, K, cell path)
    ("cheby_conv", 32, 2, "seq"), ("cheby_conv", 8, 2, "step"), ("fourier_conv", 8, 2, "fourier")]


@pytest.mark.parametrize("layers,R", [(1, 0), (2, 2)], ids=["1layer_R0", "2layers_R2"])
@pytest.mark.parametrize("filter,H,K,path", CASES, ids=[c[3] for c in CASES])
@pytest.mark.parametrize("infer_func", [EXPAND, GCONV3], ids=["weights", "concat"])
@pytest.mark.parametrize("M", [17, 40])
def test_model_matches_reference(dev, M, infer_func, filter, H, K, path, layers, R):
    m = make_model(dev, infer_func, filter, M, H, K, layers, R)
    c0 = m.cells[0][0]
    assert (path == "seq") == bool(c0.seq) and m.B == 3 and m.T == T
    if m.concat:  # the head's width is num_hidden
        want = (M, H, 3 * H) if filter == "fourier_conv" else (K * 3 * H, H)
        assert tuple(m.head_W[0].shape) == want and len(m.head_W) == 2 * R + 2
    model_vs_reference(dev, m)


def test_split_mode_ignores_the_columns_past_2FTc(dev):
    m = make_model(dev, SPLIT, "cheby_conv", 17, 8, keep=1.0)
    assert m.T == (3, 3) and m.B == 2 and m.C == 2 * F * 3
    model_vs_reference(dev, m)
    x, _ = batch(m, 4, extra=5)
    a = m.forward(t(x, dev)).clone()
    x2 = x.copy()
    x2[:, :, m.C:] = 7.5
    b = m.forward(t(x2, dev)).clone()
    assert torch.equal(a, b)
    assert torch.equal(a, m.forward(t(x[:, :, :m.C], dev)))
    with pytest.raises(ValueError):
        m.forward(t(x[:, :, :m.C - 1], dev))
    with pytest.raises(ValueError):  # the expand modes need C == F sum(T)
        e = make_model(dev, EXPAND, "cheby_conv", 17, 8)
        e.forward(t(np.zeros((N, 17, e.C + 1)), dev))


def test_the_two_weight_merge_names_are_one_network(dev):
    a, b = (make_model(dev, f, "cheby_conv", 17, 8, layers=2) for f in (EXPAND, GCONV1))
    assert torch.equal(a.flat, b.flat)
    x, labels = batch(a)
    assert torch.equal(a.forward(t(x, dev)), b.forward(t(x, dev)))
    for m in (a, b):
        m.train_step(t(x, dev), t(labels, dev))
    torch.cuda.synchronize()
    assert torch.equal(a.flat, b.flat)
    diff = [(p, q) for p, q in zip(a.names, b.names) if p != q]
    assert diff == [(f"merge_{i}/conv_init/weights", f"merge_{i}/weights") for i in range(3)]


def test_variable_names_follow_the_reference_scopes(dev):
    m = make_model(dev, EXPAND, "cheby_conv", 17, 8, layers=2)
    cell = "gconv_lstm_layer/rnn/multi_rnn_cell/cell_{}/{}"
    want = []
    for b in range(3):
        want += [f"merge_{b}/" + cell.format(li, n) for li in range(2) for n in ("Wx", "Wh", "b")]
        want += [f"merge_{b}/conv_init/weights", f"merge_{b}/weight_{b}/weights"]
    assert m.names == want
    c = make_model(dev, GCONV3, "fourier_conv", 17, 8, R=1)
    assert c.names[:9] == [f"merge_{b}/" + cell.format(0, n) for b in range(3) for n in ("Wx", "Wh", "b")]
    assert c.names[9:] == ["conv_init/weights", "conv_layer_0/residual_layer_0/sublayer0/weights",
                           "conv_layer_0/residual_layer_0/sublayer1/weights", "output_layer/weights"]
    for mm in (m, c):
        p = mm.parameters()
        lo = mm.flat.data_ptr()
        ptrs = [v.data_ptr() for v in p.values()]
        assert ptrs == sorted(ptrs) and ptrs[0] == lo  # carved in this order
        # M out = 34 floats of merge weight: the next branch's cells are moved up to 16 bytes
        pad = mm.flat.numel() - sum(v.numel() for v in p.values())
        assert pad == (0 if mm.concat else 4) and all(c.b.data_ptr() % 16 == 0 for cs in mm.cells for c in cs)
    # _weight_variable / the filters: truncated_normal(0, 0.1)
    for w in m.merge_w + m.fc_W + c.head_W:
        assert float(w.detach().abs().max()) <= 0.2 and float(w.detach().std()) > 0.05


def test_refused_and_unknown_names(dev):
    with pytest.raises(NotImplementedError, match="tf.transpose"):
        make_model(dev, "inference_glstm_period_expand_gconv2", "cheby_conv", 17, 8)
    with pytest.raises(ValueError):
        make_model(dev, "inference_glstm", "cheby_conv", 17, 8)


@pytest.mark.parametrize("infer_func,filter", [(EXPAND, "cheby_conv"), (GCONV3, "fourier_conv")],
                         ids=["weights", "concat"])
def test_three_adam_steps_match_reference(dev, infer_func, filter):
    """At the trainer's default learning rate, 1e-3.  Adam moves an entry by
    lr * m / (sqrt(v) + eps), so an fp32 gradient error d on an entry of gradient g
    becomes a parameter error of ~lr * d / |g| per step, whatever the code: with
    d = 1e-7 max|g| (what the gradients above measure) an entry 1000 times below
    its tensor's largest gradient errs by lr * 1e-4 per step.  Against max|p| ~ 0.1
    that stays below the 1e-5 bar for three steps only while lr < 3e-3.  (Measured
    at lr = 1e-2: every tensor <= 2.7e-6 but one second-layer Wh at 1.7e-5.)"""
    m = make_model(dev, infer_func, filter, 17, 8, layers=2, R=1)
    assert m.lr == 1e-3
    filt, mode, branches, merge = ref_parts(m)
    flat0 = PR.flat_params(branches, merge, mode)
    state = [(np.zeros_like(p), np.zeros_like(p)) for p in flat0]
    ema = (0.0, 0.0, 0)
    for step in (1, 2, 3):
        x, labels = batch(m, 20 + step)
        mults = next_mults(m)
        loss = m.train_step(t(x, dev), t(labels, dev))
        torch.cuda.synchronize()
        l, branches, merge, state, ema = PR.train_step(x, labels, m.T, F, branches, merge, filt, mode,
                                                       m.R, "reference", mults, state, step, m.lr, ema)
        assert abs(float(loss) - l) <= TOL * l
        assert abs(float(m.loss_average) - ema[1]) <= TOL * ema[1]
    lo, n = m.grad.data_ptr(), 4 * m.grad.numel()
    assert all(lo <= p.grad.data_ptr() < lo + n for p in m.params)
    for (name, p), ref, p0 in zip(m.parameters().items(), PR.flat_params(branches, merge, mode), flat0):
        check(name, p, ref)
        assert not np.array_equal(npy(p), p0.astype(np.float32)), name
    assert m.step_count == 3


@pytest.mark.parametrize("infer_func", [GCONV1, GCONV3], ids=["weights", "concat"])
def test_predict_on_a_ragged_size(dev, infer_func):
    m = make_model(dev, infer_func, "cheby_conv", 17, 8)
    filt, mode, branches, merge = ref_parts(m)
    size = 2 * N + 1
    rng = np.random.default_rng(17)
    data = r32(0.5 * rng.standard_normal((size, m.M, m.C)))
    labels = r32(rng.standard_normal((size, m.M, OUT)))
    slots = [s.clone() for s in (m.flat, m.ema, m.s1, m.s2)]
    preds, loss = m.predict(data, labels)
    _, mse, zero, loss2, preds2 = m.evaluate(data, labels)
    torch.cuda.synchronize()
    assert tuple(preds.shape) == (size, m.M, OUT) and torch.equal(preds, preds2) and loss == loss2

    def fwd(b):
        return PR.forward(b, m.T, F, branches, merge, filt, mode, m.R, "reference", None)[0]

    ref_preds, ref_loss = GR.predict(fwd, data, labels, N)
    check("predictions", preds, ref_preds)
    assert abs(loss - ref_loss) <= TOL * ref_loss
    assert abs(mse - GR.evaluate_mse(labels, f64(preds))) <= 1e-12 * mse and zero == 0
    assert all(torch.equal(a, b) for a, b in zip(slots, (m.flat, m.ema, m.s1, m.s2))) and m.step_count == 0
    # the reference's graph also drops when it evaluates: available on request
    mults = next_mults(m)
    dropped = m.predict(data[:N], reference_dropout=True)
    assert not torch.equal(dropped, preds[:N])
    check("reference_dropout", dropped,
          PR.forward(data[:N], m.T, F, branches, merge, filt, mode, m.R, "reference", mults)[0])


@pytest.mark.timeout(300)
def test_world2_over_gloo(dev, tmp_path):
    """Two ranks share the GPU over gloo (tests/glstm_period_dp_worker.py), one sample
    pair each of a 4-sample batch: replicas bitwise equal after two steps and
    within 1e-5 of the one-process full batch (keep_prob 1: the ranks' masks
    differ by design, so a dropped run has no full-batch equal); with dropout
    on, the ranks' wrappers draw distinct masks."""
    d = DP.launch_world2("glstm_period_dp_worker", tmp_path / "period_dp.npz", 280)
    for mode in Wk.MODES:
        assert np.array_equal(d[f"{mode}_P"], d[f"{mode}_P_r1"]), f"{mode}: replicas diverged"
        L, x, labels = Wk.problem()
        P = Wk.run(mode, L, x, labels, dev, None)
        print(mode)
        DP.assert_tracks_full_batch(d[f"{mode}_P"], P, Wk.STEPS)  # the second update ran, too
        seeds = d[f"{mode}_seeds"]  # [rank][wrapper]
        assert len(set(seeds.reshape(-1).tolist())) == seeds.size == 2 * 3 * Wk.LAYERS
