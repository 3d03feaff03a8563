"""inference_glstm_gconv on device (cnn_graph_amd.glstm_gconv.GLSTMGconvModel), its
LSTM -> head seam kernels (cg_fres_forward_drop / cg_fres_backward_drop) and
predict / evaluate of the four model classes.

Bars.  The seam kernels: BITWISE against the composition of the kernels they
replace.  The model against the float64 restatement (tests/glstm_gconv_ref.py):
normwise error < 1e-5, the bar of tests/test_gpu_fourier_lstm.py and
tests/test_gpu_lstm.py for their model-level comparisons; every case with
z = tan(a_z) asserts max|a_z| < 1.3 in the reference."""
import ctypes
import functools
import itertools
import os
import sys

import numpy as np
import pytest

import fourier_edge_cases as FE
import glstm_gconv_ref as GR
from conftest import GOLDEN, case, load_golden
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
M64 = (1 << 64) - 1
r32 = GR.r32


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def npy(a):
    return a.detach().cpu().numpy()


def f64(a):
    return npy(a).astype(np.float64)


def check(name, got, ref):
    err = O.normwise_err(npy(got) if torch.is_tensor(got) else got, ref)
    print(f"{name}: normwise err {err:.3e}")
    assert err < TOL, (name, err)


@functools.lru_cache(maxsize=None)
def laplacian(name):
    if name == "grid32":  # config E's 32 x 32 grid graph: L = L~ + I (lmax = 2)
        import scipy.sparse
        c = case(load_golden("golden_E.npz"))
        M = c["M"]
        Lt = scipy.sparse.csr_matrix((c["Lt_val"], c["Lt_col"], c["Lt_rowptr"]), shape=(M, M))
        return (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr()
    return GR.ring_chords_laplacian(int(name))


# ===== a. the seam kernels, bitwise against the composition =====================================
SEAM_M = [1, 15, 17, 128, 129, 200]
SEAM_NC = [(1, 1), (3, 8), (2, 33), (1, 128), (3, 50)]
SEAM_INNER = list(itertools.product([1, 32], [0.8, 0.5, 1.0], [("none", False), ("relu", True),
                                                                 ("none", True), ("relu", False)]))


def _dropout_backward(dy, keep, seed):
    from cnn_graph_amd import _lib
    dx = torch.empty_like(dy)
    _lib.call("cg_dropout_backward", dy.data_ptr(), dy.numel(), float(keep), int(seed), dx.data_ptr(),
              torch.cuda.current_stream(dy.device).cuda_stream)
    return dx


def _seam_case(dev, M, N, Fin, x3_label=""):
    from cnn_graph_amd import ops
    g = torch.Generator(device=dev)
    g.manual_seed(1000 * M + 10 * N + Fin)
    U = torch.randn((M, M), device=dev, generator=g) / max(M, 1) ** 0.5
    B = ops.gft_prepare(U)
    x = torch.randn((N, M, Fin), device=dev, generator=g)
    x[x == 0] = 1.0
    base, offset = 0xC0FFEE1234567 + M, 7 * N * M * Fin  # a slice of a larger dropped tensor
    seed = (base + ops.DROP_WEYL * offset) & M64
    dropped_something = False
    for Fout, keep, (act, with_res) in SEAM_INNER:
        W = torch.randn((M, Fout, Fin), device=dev, generator=g)
        res = torch.randn((N, M, Fout), device=dev, generator=g) if with_res else None
        dy = torch.randn((N, M, Fout), device=dev, generator=g)
        xd = ops.dropout(x, keep, base, offset=offset)
        if keep < 1.0:
            dropped_something |= bool(((xd == 0) & (x != 0)).any())
        xhat0, y0 = ops.fres_forward(B, W, xd, res, act)
        xhat1, y1 = ops.fres_forward_drop(B, W, x, keep, seed, res, act)
        tag = (x3_label, M, N, Fin, Fout, keep, act, with_res)
        assert torch.equal(xhat0, xhat1), ("xhat",) + tag
        assert torch.equal(y0, y1), ("y",) + tag
        dx0, dW0, dz0 = ops.fres_backward(B, W, xhat0, dy, y0, act)
        if keep < 1.0:
            dx0 = _dropout_backward(dx0, keep, seed)
        dx1, dW1, dz1 = ops.fres_backward_drop(B, W, xhat1, dy, keep, seed, y1, act)
        assert torch.equal(dx0, dx1), ("dx",) + tag
        assert torch.equal(dW0, dW1), ("dW",) + tag
        assert torch.equal(dz0, dz1), ("dz",) + tag
        assert bool(torch.isfinite(dx1).all())
        if x.numel() >= 64 and act == "none":  # (a ReLU may legitimately pass nothing at Fout 1)
            assert int(torch.count_nonzero(dx1)) > 0, ("dx is all zero",) + tag
        if keep < 1.0 and x.numel() >= 64:
            assert bool((dx1 == 0).any()), ("the backward mask drops nothing",) + tag
    torch.cuda.synchronize()
    # 0.8^64 < 1e-6: a mask that keeps every one of >= 64 elements is a broken mask
    if x.numel() >= 64:
        assert dropped_something, "keep < 1 dropped nothing: the dropped x has no new zeros"


@pytest.mark.parametrize("N,Fin", SEAM_NC)
@pytest.mark.parametrize("M", SEAM_M)
def test_seam_kernels_bitwise(dev, M, N, Fin):
    _seam_case(dev, M, N, Fin)


@pytest.mark.parametrize("M,N,Fin", [(17, 3, 8), (129, 2, 33), (200, 3, 50)])
def test_seam_kernels_bitwise_f32_transform(dev, cg_opts, M, N, Fin):
    cg_opts("gemm_x3", 0)
    _seam_case(dev, M, N, Fin, "f32")


def test_seam_argument_errors(dev):
    from cnn_graph_amd import _lib, ops
    h = _lib.lib()
    N, M, Fin, Fout = 2, 17, 8, 4
    U = torch.eye(M, device=dev)
    B = ops.gft_prepare(U)
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    W, x, xhat, y, dy, dx, dW = (z(M, Fout, Fin), z(N, M, Fin), z(N, M, Fin), z(N, M, Fout),
                                 z(N, M, Fout), z(N, M, Fin), z(M, Fout, Fin))
    fb, bb = ops.fres_workspace_bytes(N, M, Fin, Fout)
    ws = torch.empty(max(fb, bb), device=dev, dtype=torch.uint8)
    p = lambda a: a.data_ptr()  # noqa: E731

    def fwd(keep):
        return h.cg_fres_forward_drop(N, M, Fin, Fout, p(B), B.numel(), p(W), p(x), ctypes.c_float(keep),
                                      5, None, 0, p(xhat), p(y), p(ws), ws.numel(), None)

    def bwd(keep, dxp):
        return h.cg_fres_backward_drop(N, M, Fin, Fout, p(B), B.numel(), p(W), p(xhat), p(dy), None, 0,
                                       ctypes.c_float(keep), 5, None, dxp, p(dW), p(ws), ws.numel(),
                                       None)

    E = _lib.CG_ERR_ARG
    assert fwd(0.0) == E and fwd(1.5) == E and bwd(0.0, p(dx)) == E and bwd(1.5, p(dx)) == E
    assert bwd(0.8, None) == E and bwd(1.0, None) == E
    assert fwd(0.8) == _lib.CG_OK and bwd(0.8, p(dx)) == _lib.CG_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.fres_forward_drop(B, W, x, 0.0, 1)


# ===== b. the model against the float64 reference ==============================================
def make_model(dev, filter, M, N, T, F, H, C, K, R, layers, keep, seam="auto", gates="reference",
               seed=5, graph=None, **kw):
    from cnn_graph_amd.glstm_gconv import GLSTMGconvModel
    L = laplacian(graph if graph is not None else str(M))
    return GLSTMGconvModel(L, N, T, F, num_hidden=H, num_hidden_conv=C, K=K, layer_count=layers,
                           conv_layer_num=R, out_features=2, keep_prob=keep, filter=filter, seam=seam,
                           gates=gates, device=dev, seed=seed, **kw), L


def ref_parts(m, L):
    """(filt, layers, head) of a model as float64."""
    if m.filter == "fourier_conv":
        filt = ("fourier_conv", f64(m.U))
    else:
        filt = ("cheby_conv", GR.cheb_lap(L), m.K)
    layers = [tuple(f64(p) for p in (c.Wx, c.Wh, c.b)) for c in m.cells]
    return filt, layers, [f64(w) for w in m.head_W]


def next_mults(m):
    """The multipliers the NEXT dropped forward of the model will apply."""
    from cnn_graph_amd.gconv_lstm import DropoutWrapper
    T, N, M, H = m.T, m.N, m.M, m.H
    if not isinstance(m.wrapped[0], DropoutWrapper):
        return None
    mults = []
    for li, w in enumerate(m.wrapped):
        seed = GR.wrapper_call_seed(w._seed, w._calls + 1)
        if li < len(m.wrapped) - 1:
            mults.append(GR.drop_mult(seed, (T, N, M, H), w.output_keep_prob))
        else:
            mults.append(GR.drop_mult(seed, (N, M, H), w.output_keep_prob, offset=(T - 1) * N * M * H))
    return mults


def model_vs_reference(dev, m, L, x_scale=0.5, seed=9):
    filt, layers, head = ref_parts(m, L)
    rng = np.random.default_rng(seed)
    xs = r32(x_scale * rng.standard_normal((m.T, m.N, m.M, m.F)))
    dout = r32(rng.standard_normal((m.N, m.M, 2)) / (m.N * m.M))
    mults = next_mults(m)
    xt = t(xs, dev).requires_grad_(True)
    out = m.forward(xt).clone()
    m.backward(t(dout, dev))
    torch.cuda.synchronize()
    ref_out, fw = GR.forward(xs, layers, head, filt, m.R, m.cells[0].gates, mults)
    az = GR.max_az(fw, m.cells[0].gates)
    print(f"max|a_z| = {az:.3f}")
    assert az < FE.AZ_MAX
    dxs, dl, dh = GR.backward(dout, fw, layers, head, filt, m.R, m.cells[0].gates, mults)
    check("out", out, ref_out)
    grads = m.gradients()
    assert list(grads) == m.names and len(m.names) == 3 * len(layers) + len(head)
    for (name, g), ref in zip(grads.items(), GR.flat_params(dl, dh)):
        check(name, g, ref)
    check("dL/dx", xt.grad, dxs)


FOURIER_CASES = list(itertools.product([0, 2], [1, 2], [0.8, 1.0], ["fused", "unfused"]))


@pytest.mark.parametrize("R,layers,keep,seam", FOURIER_CASES)
@pytest.mark.parametrize("H", [8, 12], ids=["H8_fused_step", "H12_unfused_cell"])
def test_fourier_model_matches_reference(dev, H, R, layers, keep, seam):
    m, L = make_model(dev, "fourier_conv", 40, 3, 3, 2, H, 8, 2, R, layers, keep, seam)
    assert m.cells[0].fused == (H == 8) and m.seam == seam
    assert tuple(m.head_W[0].shape) == (40, 8, H) and tuple(m.head_W[-1].shape) == (40, 2, 8)
    model_vs_reference(dev, m, L)


@pytest.mark.parametrize("H,K,layers", [(32, 2, 1), (32, 2, 2), (8, 3, 1), (8, 3, 2)],
                         ids=["seq_kernel", "seq_kernel_2", "step_path", "step_path_2"])
def test_cheby_model_matches_reference(dev, H, K, layers):
    m, L = make_model(dev, "cheby_conv", 40, 3, 3, 2, H, 8, K, 1, layers, 0.8)
    assert m.cells[0].seq == (H == 32) and m.seam == "unfused"
    assert tuple(m.head_W[0].shape) == (K * H, 8)
    model_vs_reference(dev, m, L)
    with pytest.raises(ValueError):
        make_model(dev, "cheby_conv", 40, 3, 3, 2, H, 8, K, 1, layers, 0.8, seam="fused")


def test_model_on_the_grid_at_the_drivers_widths(dev):
    """M 1024 (the 32 x 32 grid), H 128, C 32: the driver's widths at the smallest
    batch (most of its seconds are the float64 reference's transforms)."""
    m, L = make_model(dev, "fourier_conv", 1024, 2, 2, 2, 128, 32, 2, 1, 1, 0.8, "fused",
                      graph="grid32")
    model_vs_reference(dev, m, L)


def test_variable_names_follow_the_reference_scopes(dev):
    m, _ = make_model(dev, "fourier_conv", 40, 3, 3, 2, 8, 8, 2, 2, 1, 0.8)
    assert m.names[3:] == ["conv_init/weights",
                           "conv_layer_0/residual_layer_0/sublayer0/weights",
                           "conv_layer_0/residual_layer_0/sublayer1/weights",
                           "conv_layer_1/residual_layer_1/sublayer0/weights",
                           "conv_layer_1/residual_layer_1/sublayer1/weights",
                           "output_layer/weights"]
    # truncated_normal(0, 0.1) (lib/filter.py:39): nothing beyond two standard deviations
    for w in m.head_W:
        assert float(w.abs().max()) <= 0.2 and float(w.std()) > 0.05
    p = m.parameters()
    assert all(m.flat.data_ptr() <= v.data_ptr() < m.flat.data_ptr() + 4 * m.flat.numel()
               for v in p.values())
    assert sum(v.numel() for v in p.values()) == m.flat.numel()


# ===== c. fused against unfused ==================================================================
def _batch(m, seed=3):
    rng = np.random.default_rng(seed)
    x = r32(0.5 * rng.standard_normal((m.N, m.M, m.F * m.T)))
    labels = r32(rng.standard_normal((m.N, m.M, 2)))
    return x, labels


def test_fused_and_unfused_seams_train_bitwise_equal(dev):
    ms = [make_model(dev, "fourier_conv", 40, 3, 3, 2, 8, 8, 2, 1, 2, 0.8, seam)[0]
          for seam in ("fused", "unfused")]
    x, labels = _batch(ms[0])
    assert torch.equal(ms[0].flat, ms[1].flat)
    start = ms[0].flat.clone()
    for m in ms:
        for _ in range(3):
            m.train_step(t(x, dev), t(labels, dev))
    torch.cuda.synchronize()
    assert torch.equal(ms[0].flat, ms[1].flat) and torch.equal(ms[0].ema, ms[1].ema)
    assert not torch.equal(ms[0].flat, start)


# ===== d. train_step =============================================================================
@pytest.mark.parametrize("filter,seam", [("fourier_conv", "fused"), ("cheby_conv", "auto")])
def test_adam_step_matches_reference(dev, filter, seam):
    m, L = make_model(dev, filter, 40, 3, 3, 2, 8, 8, 2, 1, 1, 0.8, seam, learning_rate=1e-2)
    filt, layers, head = ref_parts(m, L)
    x, labels = _batch(m)
    mults = next_mults(m)
    loss = m.train_step(t(x, dev), t(labels, dev))
    torch.cuda.synchronize()
    for p in m.params:  # every gradient lives in the flat bucket
        assert m.grad.data_ptr() <= p.grad.data_ptr() < m.grad.data_ptr() + 4 * m.grad.numel()
    for g in m.head_dW:
        assert m.grad.data_ptr() <= g.data_ptr() < m.grad.data_ptr() + 4 * m.grad.numel()
    flat0 = GR.flat_params(layers, head)
    state = [(np.zeros_like(p), np.zeros_like(p)) for p in flat0]
    xs = np.ascontiguousarray(np.moveaxis(x.reshape(m.N, m.M, m.F, m.T), 3, 0))
    l, _, new_p, _, ema = GR.train_step(xs, labels, layers, head, filt, m.R, "reference", mults, state,
                                        1, 1e-2, (0.0, 0.0, 0))
    assert abs(float(loss) - l) < TOL * l
    assert abs(float(m.loss_average) - ema[1]) < TOL * ema[1]
    for (name, p), ref, p0 in zip(m.parameters().items(), new_p, flat0):
        check(name, p, ref)
        assert not np.array_equal(npy(p), p0.astype(np.float32)), name


MODELS = ["GLSTMGconvModel", "GLSTMModel", "ResGNN", "StackedResGNN"]


def _build(dev, which, **kw):
    """One of the four model classes at the small shapes; each reads x [3, 40, 6]."""
    from cnn_graph_amd.gconv_lstm import GLSTMModel
    from cnn_graph_amd.model import ResGNN, StackedResGNN
    L = laplacian("40")
    if which == "GLSTMGconvModel":
        return make_model(dev, "fourier_conv", 40, 3, 3, 2, 8, 8, 2, 1, 2, 0.8, "fused", **kw)[0]
    if which == "GLSTMModel":
        return GLSTMModel(L, 3, 3, 2, num_hidden=8, K=2, layer_count=2, out_features=2, keep_prob=0.8,
                          device=dev, seed=5, **kw)
    if which == "ResGNN":
        return ResGNN(L, 3, 6, 8, 3, 1, 2, device=dev, seed=5, **kw)
    return StackedResGNN(L, 3, 6, 8, 3, 1, groups=((0, 4), (4, 6)), device=dev, seed=5, filter="fourier",
                         **kw)


class _DoublingComm:
    """world 2 with both ranks holding the same gradient: the sum is 2 g."""
    world, rank = 2, 0

    def __init__(self):
        self.calls = []

    def allreduce_sum_(self, tensor, stream):
        self.calls.append((tensor.data_ptr(), tensor.numel()))
        tensor.mul_(2.0)


@pytest.mark.parametrize("which", MODELS)
def test_comm_contract_one_allreduce_and_grad_scale(dev, which):
    comm = _DoublingComm()
    a, b = _build(dev, which), _build(dev, which, comm=comm)
    rng = np.random.default_rng(3)
    x = r32(0.5 * rng.standard_normal((3, 40, 6)))
    labels = r32(rng.standard_normal((3, 40, 2)))
    assert torch.equal(a.flat, b.flat)
    start = a.flat.clone()
    for m in (a, b):
        m.train_step(t(x, dev), t(labels, dev))
    torch.cuda.synchronize()
    # exactly one all-reduce, of the whole bucket
    assert comm.calls == [(b.grad.data_ptr(), b.grad.numel())] and b.world == 2 and a.world == 1
    assert b.grad.numel() == b.flat.numel()
    assert torch.equal(a.flat, b.flat)  # (2 g) * 1/2 is exact
    assert not torch.equal(a.flat, start)


@pytest.mark.parametrize("optimizer", ["sgd", "rmsprop"])
def test_other_optimizers_step(dev, optimizer):
    m, _ = make_model(dev, "cheby_conv", 40, 3, 3, 2, 8, 8, 2, 1, 1, 0.8, optimizer=optimizer)
    x, labels = _batch(m)
    before = m.flat.clone()
    m.train_step(t(x, dev), t(labels, dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(m.flat).all())
    lstm_n = sum(p.numel() for p in m.params)
    assert not torch.equal(m.flat[:lstm_n], before[:lstm_n])
    assert not torch.equal(m.flat[lstm_n:], before[lstm_n:])
    assert m.step_count == 1 and m.learning_rate(0) == m.lr


# ===== e. predict and evaluate ===================================================================
_plain = lambda m, b: m.forward(b)  # noqa: E731
_undropped = lambda m, b: m.forward(b, dropout=False)  # noqa: E731
# the per-batch forward that predict's default (no dropout) must equal bitwise
_PREDICT_FORWARD = {"GLSTMGconvModel": _undropped, "GLSTMModel": _undropped, "ResGNN": _plain,
                    "StackedResGNN": _plain}


def _state(m):
    slots = [m.flat, m.ema, m.s1, m.s2]
    return [s.clone() for s in slots], m.step_count


@pytest.mark.parametrize("which", MODELS)
def test_predict_and_evaluate(dev, which):
    m, fwd = _build(dev, which), _PREDICT_FORWARD[which]
    N, M = m.N, m.M
    size = 2 * N + 1
    rng = np.random.default_rng(17)
    data = r32(0.5 * rng.standard_normal((size, M, 6)))
    labels = r32(rng.standard_normal((size, M, 2)))
    m.train_step(t(data[:N], dev), t(labels[:N], dev))  # non-trivial optimizer state and EMA
    torch.cuda.synchronize()
    slots, steps = _state(m)
    preds, loss = m.predict(data, labels)
    string, mse, zero, loss2, preds2 = m.evaluate(data, labels)
    torch.cuda.synchronize()
    assert tuple(preds.shape) == (size, M, 2)  # the padded rows are not returned
    assert torch.equal(preds, preds2) and loss == loss2 and zero == 0  # two calls agree bitwise
    assert torch.equal(m.predict(data), preds)
    # per-batch forward, bitwise; the reference formulae on those very predictions
    ref_loss = 0.0
    with torch.no_grad():
        for b0 in range(0, size, N):
            batch, bl = np.zeros((N, M, 6)), np.zeros((N, M, 2))
            n = min(N, size - b0)
            batch[:n], bl[:n] = data[b0:b0 + n], labels[b0:b0 + n]
            out = fwd(m, t(batch, dev)).clone()
            assert torch.equal(out[:n], preds[b0:b0 + n]), (which, b0)
            ref_loss += float(np.mean((bl - f64(out)) ** 2))
    ref_loss = ref_loss * N / size
    print(f"{which}: loss {loss:.6e} ref {ref_loss:.6e} mse {mse:.6e}")
    assert abs(loss - ref_loss) < TOL * ref_loss
    ref_mse = GR.evaluate_mse(labels, f64(preds))
    assert abs(mse - ref_mse) < 1e-12 * ref_mse and string.startswith("mse: ")
    slots2, steps2 = _state(m)
    assert steps2 == steps and all(torch.equal(a, b) for a, b in zip(slots, slots2))


def test_predict_with_the_reference_dropout(dev):
    m, L = make_model(dev, "fourier_conv", 40, 3, 3, 2, 8, 8, 2, 1, 2, 0.8, "fused")
    filt, layers, head = ref_parts(m, L)
    rng = np.random.default_rng(23)
    data = r32(0.5 * rng.standard_normal((m.N, m.M, 6)))
    plain = m.predict(data)
    mults = next_mults(m)
    dropped = m.predict(data, reference_dropout=True)
    torch.cuda.synchronize()
    assert not torch.equal(plain, dropped)
    xs = np.ascontiguousarray(np.moveaxis(data.reshape(m.N, m.M, m.F, m.T), 3, 0))
    check("plain", plain, GR.forward(xs, layers, head, filt, m.R, "reference", None)[0])
    ref, fw = GR.forward(xs, layers, head, filt, m.R, "reference", mults)
    assert GR.max_az(fw, "reference") < FE.AZ_MAX
    check("reference_dropout", dropped, ref)


# ===== f. ResGNN unchanged =======================================================================
@pytest.mark.parametrize("filter", ["chebyshev5", "fourier"])
def test_resgnn_unchanged(dev, filter):
    """tests/golden/resgnn_steps.npz holds ResGNN's flat parameters and loss after
    two train_steps as the commit before the ``_ResNet`` ``input_grad`` switch
    computed them (tests/golden/make_resgnn_steps.py says how it was made)."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_resgnn_steps as G
    finally:
        sys.path.remove(GOLDEN)
    gold = load_golden("resgnn_steps.npz")
    flat, loss = G.run_steps(filter)
    assert np.array_equal(flat, gold[f"{filter}_flat"])
    assert np.array_equal(loss, gold[f"{filter}_loss"])
    assert os.path.getsize(os.path.join(GOLDEN, "resgnn_steps.npz")) < (1 << 20)


# ===== g. the other three models unchanged =====================================================
def _golden_steps():
    sys.path.insert(0, GOLDEN)
    try:
        import make_resgnn_steps as G
    finally:
        sys.path.remove(GOLDEN)
    return G


@pytest.mark.parametrize("name", list(_golden_steps().MODEL_CASES))
def test_models_unchanged(dev, name):
    """tests/golden/model_steps.npz holds flat, loss and the loss moving average of
    StackedResGNN, GLSTMModel and GLSTMGconvModel after two train_steps (the second
    at the decayed learning rate) as the commit before trainer.FlatTrainer computed
    them (tests/golden/make_resgnn_steps.py --models).  branch_model_steps.npz holds
    the same for GLSTMPeriodModel, GConvNetModel and GConvRNNModel (BRANCH_CASES;
    the last one's loss is its own, its moving average stays zero) as the commit
    before the models' shared pieces moved into trainer.py computed them
    (--branch-models)."""
    G = _golden_steps()
    fixture = "branch_model_steps.npz" if name in G.BRANCH_CASES else "model_steps.npz"
    gold = load_golden(fixture)
    flat, loss, ema = G.run_model_steps(name)
    assert np.array_equal(flat, gold[f"{name}_flat"])
    assert np.array_equal(loss, gold[f"{name}_loss"])
    assert np.array_equal(ema, gold[f"{name}_ema"])
    assert os.path.getsize(os.path.join(GOLDEN, fixture)) < (1 << 20)
