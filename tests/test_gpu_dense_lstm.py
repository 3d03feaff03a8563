"""cg_dlstm_seq_forward / _backward and cg_class_xent_sum through the C ABI
against the float64 reference of tests/dense_lstm_ref.py, at the smallest shapes
where the tiling can go wrong: N 1 / 5 / 33 (33 = two full 16-row tiles and a
ragged third), T 1 / 3, H 16 / 48 (Wh in LDS, row stride H), 32 (stride H + 16),
80 and 96 (either side of the LDS-resident / streamed line) and 128 (streamed,
eight waves), C 7 / 40.  Bar: 1e-5 normwise."""
import ctypes

import numpy as np
import pytest

import dense_lstm_ref as R
from cnn_graph_amd import _lib
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
CASES = [(1, 1, 16, 7), (5, 3, 16, 7), (33, 3, 16, 40), (5, 1, 48, 40), (33, 3, 48, 7), (33, 3, 32, 7),
         (5, 3, 80, 7), (33, 3, 96, 7), (1, 3, 128, 7), (33, 3, 128, 40), (33, 1, 128, 7)]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def n64(a):
    return a.detach().cpu().numpy().astype(np.float64)


_problems = {}


def problem(N, T, H, C):
    """The fp32 inputs (as float64) and the reference's results, computed once per shape."""
    key = (N, T, H, C)
    if key not in _problems:
        rng = np.random.default_rng(1000 * N + 100 * T + H + C)
        f = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)  # noqa: E731
        xs, Wx, Wh, b = f(T, N, C), f(C, 4 * H) / np.sqrt(C), f(H, 4 * H) / np.sqrt(H), 0.1 * f(4 * H)
        dhs = f(T, N, H)
        gx = (xs @ Wx).astype(np.float32).astype(np.float64)
        hs, cs, act = R.cell_forward(gx, Wh, b, 1.0)
        dpre = R.cell_backward(dhs, act, cs, Wh)
        _problems[key] = dict(xs=xs, Wh=Wh, b=b, dhs=dhs, gx=gx, hs=hs, cs=cs, act=act, dpre=dpre,
                              grads=R.weight_grads(xs, hs, dpre))
    return _problems[key]


def forward(h, dev, p, N, T, H, with_act=True):
    f32 = dict(device=dev, dtype=torch.float32)
    gx, Wh, b = t(p["gx"], dev), t(p["Wh"], dev), t(p["b"], dev)
    hs, cs = torch.full((T, N, H), float("nan"), **f32), torch.full((T, N, H), float("nan"), **f32)
    act = torch.full((T, N, 4 * H), float("nan"), **f32) if with_act else None
    s = torch.cuda.current_stream(dev).cuda_stream
    _lib.check("cg_dlstm_seq_forward",
               h.cg_dlstm_seq_forward(T, N, H, gx.data_ptr(), Wh.data_ptr(), b.data_ptr(), ctypes.c_float(1.0),
                                      hs.data_ptr(), cs.data_ptr(), act.data_ptr() if with_act else None,
                                      None, 0, s))
    return hs, cs, act, Wh


def backward(h, dev, p, N, T, H, act, cs, Wh):
    dhs = t(p["dhs"], dev)
    dpre = torch.full((T, N, 4 * H), float("nan"), device=dev, dtype=torch.float32)
    s = torch.cuda.current_stream(dev).cuda_stream
    _lib.check("cg_dlstm_seq_backward",
               h.cg_dlstm_seq_backward(T, N, H, dhs.data_ptr(), act.data_ptr(), cs.data_ptr(), Wh.data_ptr(),
                                       ctypes.c_float(1.0), dpre.data_ptr(), None, 0, s))
    return dpre


@pytest.mark.parametrize("N,T,H,C", CASES)
def test_sequence_entries_vs_reference(dev, N, T, H, C):
    from cnn_graph_amd import ops
    h = _lib.lib()
    p = problem(N, T, H, C)
    hs, cs, act, Wh = forward(h, dev, p, N, T, H)
    dpre = backward(h, dev, p, N, T, H, act, cs, Wh)
    torch.cuda.synchronize()
    for name, got in (("hs", hs), ("cs", cs), ("act", act), ("dpre", dpre)):
        err = O.normwise_err(n64(got), p[name])
        print(f"N {N} T {T} H {H} {name}: {err:.2e}")
        assert err < TOL, (name, err)
    # the three weight gradients, on the existing entries over the kernels' dpre
    xs2, d2 = t(p["xs"], dev).view(T * N, C), dpre.view(T * N, 4 * H)
    dWx = ops.gemm(xs2, d2, trans_a=True)
    db = ops.bias_grad(d2)
    if T > 1:
        dWh = ops.gemm(hs.view(T * N, H)[:(T - 1) * N], d2[N:], trans_a=True)
    else:  # no zero-row GEMM: the autograd wrapper writes zeros
        xg = t(p["xs"], dev).view(T * N, C)
        k = torch.cat([t(np.zeros((C, 4 * H)), dev), Wh]).requires_grad_(True)
        out = ops.dense_lstm_seq(xg, k, t(p["b"], dev), T, N, 1.0, "seq")
        out.backward(t(p["dhs"], dev))
        dWh = k.grad[C:]
        assert torch.equal(dWh, torch.zeros_like(dWh))  # exactly zero
    torch.cuda.synchronize()
    for name, got, ref in zip(("dWx", "dWh", "db"), (dWx, dWh, db), p["grads"]):
        if name == "dWh" and T == 1:
            assert not ref.any()
            continue
        err = O.normwise_err(n64(got), ref)
        print(f"N {N} T {T} H {H} {name}: {err:.2e}")
        assert err < TOL, (name, err)


@pytest.mark.parametrize("N,T,H,C", [(33, 3, 48, 7), (33, 3, 32, 7), (5, 3, 128, 7)])
def test_inference_forward_and_repeat_calls_are_bitwise(dev, N, T, H, C):
    h = _lib.lib()
    p = problem(N, T, H, C)
    hs, cs, act, Wh = forward(h, dev, p, N, T, H)
    hs_i, cs_i, _, _ = forward(h, dev, p, N, T, H, with_act=False)  # act = NULL
    hs2, cs2, act2, _ = forward(h, dev, p, N, T, H)
    dpre = backward(h, dev, p, N, T, H, act, cs, Wh)
    dpre2 = backward(h, dev, p, N, T, H, act, cs, Wh)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(hs).all())
    assert torch.equal(hs_i, hs) and torch.equal(cs_i, cs)
    assert torch.equal(hs2, hs) and torch.equal(cs2, cs) and torch.equal(act2, act)
    assert bool(torch.isfinite(dpre).all()) and torch.equal(dpre2, dpre)


@pytest.mark.parametrize("path", ["seq", "steps"])
def test_autograd_wrapper_both_paths(dev, path):
    """ops.dense_lstm_seq over xs and TF's single kernel: the one-launch path
    and the per-step composition give the reference's hs and gradients."""
    from cnn_graph_amd import ops
    N, T, H, C = 5, 3, 48, 7
    p = problem(N, T, H, C)
    rng = np.random.default_rng(4)
    Wx = (rng.standard_normal((C, 4 * H)) / np.sqrt(C)).astype(np.float32).astype(np.float64)
    kern = np.concatenate([Wx, p["Wh"]])
    gx = p["xs"] @ Wx
    hs, cs, act = R.cell_forward(gx, p["Wh"], p["b"], 1.0)
    dpre = R.cell_backward(p["dhs"], act, cs, p["Wh"])
    dWx, dWh, db = R.weight_grads(p["xs"], hs, dpre)
    k, b = t(kern, dev).requires_grad_(True), t(p["b"], dev).requires_grad_(True)
    x = t(p["xs"], dev).view(T * N, C).requires_grad_(True)
    out = ops.dense_lstm_seq(x, k, b, T, N, 1.0, path)
    out.backward(t(p["dhs"], dev))
    torch.cuda.synchronize()
    for name, got, ref in (("hs", out, hs), ("dkernel", k.grad, np.concatenate([dWx, dWh])), ("db", b.grad, db),
                           ("dx", x.grad, (dpre @ Wx.T).reshape(T * N, C))):
        err = O.normwise_err(n64(got), ref)
        print(f"{path} {name}: {err:.2e}")
        assert err < TOL, (name, err)


@pytest.mark.parametrize("rows,C", [(5, 7), (99, 40), (3, 130)])
def test_class_xent_sum_vs_reference_and_the_mean_entry(dev, rows, C):
    from cnn_graph_amd import ops
    rng = np.random.default_rng(rows + C)
    x = (3 * rng.standard_normal((rows, C))).astype(np.float32)
    labels = rng.integers(0, C, rows)
    labels[0], labels[-1] = 0, C - 1  # labels 0 and C - 1 are present
    lab = ops.class_labels(labels, C, dev)
    scale = 1.0 / 3
    r = ops.class_xent_sum(t(x, dev), lab, scale, want_ce=True, want_pred=True)
    torch.cuda.synchronize()
    loss, dlogits, ce = R.xent_sum(x.astype(np.float64), labels, float(np.float32(scale)))
    assert abs(float(r.loss.item()) - loss) < TOL * abs(loss)
    assert O.normwise_err(n64(r.dlogits), dlogits) < TOL
    assert O.normwise_err(n64(r.ce), ce) < TOL
    assert np.array_equal(r.pred.cpu().numpy(), x.argmax(1))
    assert int(r.correct.item()) == int((x.argmax(1) == labels).sum()) and int(r.status.item()) == 0
    # evaluation form: the same loss bits, no gradient
    e = ops.class_xent_sum(t(x, dev), lab, scale, need_grad=False)
    assert e.dlogits is None and torch.equal(e.loss, r.loss)
    # loss_scale = 1/rows and no regularisation: the mean entry, bit for bit
    inv = float(np.float32(1.0 / rows))
    a = ops.class_xent_sum(t(x, dev), lab, inv)
    m = ops.class_xent_call(t(x, dev), lab)
    torch.cuda.synchronize()
    assert torch.equal(a.loss, m.loss) and torch.equal(a.dlogits, m.dlogits)
