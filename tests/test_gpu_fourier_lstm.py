"""gconv-LSTM with the Fourier filter (GConvLSTMCell(filter_type="fourier_conv"),
lib/gconv_lstm.py:59, :116-133, :183-221) on the HIP path against the float64
restatement (tests/fourier_lstm_ref.py).  Bar: normwise error < 1e-5 on every
forward quantity and every gradient, for both CG_OPT_GEMM_X3 settings.  Every
test with z = tan(a_z) also asserts max|a_z| < 1.3 in the float64 reference, so
a pole can neither inflate nor mask an error."""
import functools

import numpy as np
import pytest
import scipy.sparse

import fourier_edge_cases as FE
import fourier_lstm_ref as FR
from conftest import case, load_golden
from oracle import cheb_oracle as O
from oracle import fourier_oracle as FO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
r32 = FR.r32


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


@pytest.fixture(params=[1, 0], ids=["x3", "f32"])
def x3(request, cg_opts):
    cg_opts("gemm_x3", request.param)
    return request.param


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def npy(a):
    return a.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def laplacian(name):
    """The Laplacian L = L~ + I (lmax = 2) of a golden graph, or of one of
    fourier_edge_cases' synthetic k-NN graphs, kept per name so the cells of a
    test share one cached Fourier basis."""
    if name in FE.SYNTHETIC_GRAPHS:
        return FE.synthetic_laplacian(name)
    c = case(load_golden(f"golden_{name}.npz"))
    M = c["M"]
    Lt = scipy.sparse.csr_matrix((c["Lt_val"], c["Lt_col"], c["Lt_rowptr"]), shape=(M, M))
    return (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr(), M


def basis(name, dev):
    """(device U fp32, the same values as float64, prepared transform operand)."""
    from cnn_graph_amd import filter as F
    from cnn_graph_amd import ops
    L, M = laplacian(name)
    U = F.fourier_basis(L, dev)
    return U, npy(U).astype(np.float64), ops.gft_prepare(U)


def make_cell(name, feat_in, H, gates, dev, seed, hconv="auto", params=None):
    """A Fourier cell on the graph `name`; params = (Wx, Wh, b) replaces the
    seeded initial values (inputs that a test without a GPU can rebuild)."""
    from cnn_graph_amd.gconv_lstm import GConvLSTMCell
    L, M = laplacian(name)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cell = GConvLSTMCell(H, laplacian=L, lmax=2, K=3, feat_in=feat_in, gates=gates, device=dev,
                         generator=g, hconv=hconv, filter_type="fourier_conv")
    if params is not None:
        with torch.no_grad():
            for p, v in zip(cell.parameters(), params):
                p.copy_(t(v, dev).view_as(p))
    return cell


def params_np(cell):
    return [npy(p).astype(np.float64) for p in (cell.Wx, cell.Wh, cell.b)]


def check(name, got, ref):
    err = O.normwise_err(npy(got) if torch.is_tensor(got) else got, ref)
    print(f"{name}: normwise err {err:.3e}")
    assert err < TOL, (name, err)


# -- the batched transform ------------------------------------------------------------
@pytest.mark.parametrize("name,N,C", [("A", 3, 1), ("A", 3, 2), ("A", 3, 8), ("A", 3, 32),
                                      ("A", 3, 128), ("E", 2, 32)])
def test_gft_analysis_and_synthesis(dev, x3, name, N, C):
    from cnn_graph_amd import ops
    U, U64, B = basis(name, dev)
    M = U64.shape[0]
    x = r32(np.random.default_rng(7).standard_normal((N, M, C)))
    xt = t(x, dev)
    xh = ops.gft(B, xt)
    y = ops.gft(B, xt, inverse=True)
    back = ops.gft(B, xh, inverse=True)
    torch.cuda.synchronize()
    check("analysis", xh, np.einsum("vm,nvc->nmc", U64, x))
    check("synthesis", y, np.einsum("vm,nmc->nvc", U64, x))
    check("round trip", back, x)


# -- the per-frequency contraction ------------------------------------------------------
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("Cin", [1, 2, 3, 32])
def test_fourier_mix_forms(dev, R, Cin):
    from cnn_graph_amd import ops
    _, M = laplacian("A")
    Cout = 128
    rng = np.random.default_rng(R * 10 + Cin)
    W = r32(rng.uniform(-0.1, 0.1, (M, Cout, Cin)))
    x = r32(rng.standard_normal((R, M, Cin)))
    g = r32(rng.standard_normal((R, M, Cout)))
    add = r32(rng.standard_normal((R, M, Cout)))
    Wt, xt, gt, addt = (t(a, dev) for a in (W, x, g, add))
    fwd = ops.fourier_mix("fwd", Wt, x=xt)
    acc = ops.fourier_mix("fwd", Wt, x=xt, add=addt)
    inplace = addt.clone()
    ops.fourier_mix("fwd", Wt, x=xt, add=inplace, out=inplace)
    tr = ops.fourier_mix("t", Wt, g=gt)
    dw = ops.fourier_mix("dw", x=xt, g=gt)
    dw2 = ops.fourier_mix("dw", x=xt, g=gt)
    torch.cuda.synchronize()
    ref = np.einsum("moi,rmi->rmo", W, x)
    check("forward", fwd, ref)
    check("forward + add", acc, ref + add)
    assert torch.equal(acc, inplace)
    check("transposed", tr, np.einsum("moi,rmo->rmi", W, g))
    check("weight gradient", dw, np.einsum("rmo,rmi->moi", g, x))
    assert torch.equal(dw, dw2)  # fixed-order reduction


# -- one cell step ------------------------------------------------------------------------
@pytest.mark.parametrize("hconv", ["fused", "unfused"])
@pytest.mark.parametrize("gates", ["reference", "standard"])
@pytest.mark.parametrize("H", [8, 32])
def test_cell_step_autograd_vs_restatement(dev, x3, H, gates, hconv):
    N, Fin = 3, 2
    cell = make_cell("A", Fin, H, gates, dev, seed=11, hconv=hconv)
    assert cell.fused == (hconv == "fused")
    M = cell._nNode
    U64 = npy(cell.U).astype(np.float64)
    rng = np.random.default_rng(2)
    x, c0, h0 = r32(rng.standard_normal((N, M, Fin))), r32(0.5 * rng.standard_normal((N, M, H))), \
        r32(0.5 * rng.standard_normal((N, M, H)))
    gh, gc = r32(rng.standard_normal((N, M, H))), r32(rng.standard_normal((N, M, H)))
    xt, ct, ht = (t(a, dev).requires_grad_() for a in (x, c0, h0))
    new_h, (new_c, new_h2) = cell(xt, (ct, ht))
    assert new_h2 is new_h
    ((new_h * t(gh, dev)).sum() + (new_c * t(gc, dev)).sum()).backward()
    torch.cuda.synchronize()
    Wx, Wh, b = params_np(cell)
    cn, hn, cache = FR.cell_forward(x, c0, h0, Wx, Wh, b, U64, gates)
    assert FR.max_az([cache]) < 1.3
    dx, dc, dh, dWx, dWh, db = FR.cell_backward(gh, gc, cache, Wx, Wh, U64, gates)
    for name, got, ref in (("c", new_c, cn), ("h", new_h, hn), ("dx", xt.grad, dx), ("dc", ct.grad, dc),
                           ("dh", ht.grad, dh), ("dWx", cell.Wx.grad, dWx), ("dWh", cell.Wh.grad, dWh),
                           ("db", cell.b.grad, db)):
        check(name, got, ref)


# -- layers -----------------------------------------------------------------------------
def _run_layers(dev, name, T, N, Fin, H, layers, given_state, seed, gates="reference", inputs=None):
    """static_rnn over `layers` Fourier cells against the restatement: outputs,
    every layer's c_T and every gradient.  inputs = fourier_edge_cases.layer_inputs
    gives the parameters and the data; None draws them here from `seed`."""
    from cnn_graph_amd.gconv_lstm import static_rnn
    cells = [make_cell(name, Fin if li == 0 else H, H, gates, dev, seed=seed + li,
                       params=None if inputs is None else inputs["params"][li])
             for li in range(layers)]
    assert all(c.fused for c in cells)
    M = cells[0]._nNode
    U64 = npy(cells[0].U).astype(np.float64)
    if inputs is None:
        rng = np.random.default_rng(seed)
        xs = r32(rng.standard_normal((T, N, M, Fin)))
        G = r32(rng.standard_normal((T, N, M, H)))
        GC = r32(rng.standard_normal((layers, N, M, H)))
        st = [(r32(0.5 * rng.standard_normal((N, M, H))), r32(0.5 * rng.standard_normal((N, M, H))))
              for _ in range(layers)] if given_state else None
    else:
        xs, G, GC, st = (inputs[k] for k in ("xs", "G", "GC", "st"))
        assert xs.shape == (T, N, M, Fin) and G.shape == (T, N, M, H) and (st is not None) == given_state
    xt = t(xs, dev).requires_grad_()
    st_t = None if st is None else [tuple(t(a, dev).requires_grad_() for a in s) for s in st]
    outs, states = static_rnn(cells, xt, st_t)
    loss = (torch.stack(outs) * t(G, dev)).sum()
    for li in range(layers):
        loss = loss + (states[li].c * t(GC[li], dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    P = [params_np(c) for c in cells]
    inp, fw = xs, []
    for li in range(layers):
        c0, h0 = (None, None) if st is None else st[li]
        hs, cs, caches = FR.layer_forward(inp, P[li], U64, c0, h0, gates)
        if gates == "reference":
            assert FR.max_az(caches) < 1.3
        fw.append((hs, cs, caches))
        inp = hs
    check("outputs", torch.stack(outs), fw[-1][0])
    d = G
    for li in range(layers - 1, -1, -1):
        check(f"c_T[{li}]", states[li].c, fw[li][1][-1])
        check(f"h_T[{li}]", states[li].h, fw[li][0][-1])
        d, dc0, dh0, dWx, dWh, db = FR.layer_backward(d, GC[li], fw[li][2], P[li], U64, gates)
        check(f"dWx[{li}]", cells[li].Wx.grad, dWx)
        check(f"dWh[{li}]", cells[li].Wh.grad, dWh)
        check(f"db[{li}]", cells[li].b.grad, db)
        if st is not None:
            check(f"dc0[{li}]", st_t[li][0].grad, dc0)
            check(f"dh0[{li}]", st_t[li][1].grad, dh0)
    check("dxs", xt.grad, d)


@pytest.mark.parametrize("given_state", [False, True], ids=["zero_state", "given_state"])
def test_two_layer_static_rnn(dev, x3, given_state):
    _run_layers(dev, "A", T=4, N=2, Fin=2, H=32, layers=2, given_state=given_state, seed=21)


def test_fused_layer_on_the_grid_graph(dev, x3):
    """M = 1024 (config E's 32 x 32 grid): eight row tiles, no tile tails."""
    _run_layers(dev, "E", T=2, N=2, Fin=2, H=32, layers=1, given_state=False, seed=31)


def test_layer_without_final_c(dev):
    """layer(..., final_c=False): an empty c_T that autograd does not
    differentiate, and the gradients of the final_c=True call, bitwise."""
    from cnn_graph_amd.gconv_lstm import layer
    cell = make_cell("A", 2, 32, "reference", dev, seed=41, hconv="fused")
    assert cell.fused
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    xs = torch.randn((3, 2, cell._nNode, 2), device=dev, generator=g)
    grads = {}
    for final_c in (True, False):
        for p in cell.parameters():
            p.grad = None
        hs, state = layer(cell, xs, final_c=final_c)
        if not final_c:
            assert state.c.numel() == 0 and state.c.requires_grad is False
        hs.sum().backward()
        grads[final_c] = [p.grad.clone() for p in cell.parameters()]
    torch.cuda.synchronize()
    for a, b in zip(grads[True], grads[False]):
        assert int(torch.count_nonzero(a)) > 0 and torch.equal(a, b)


# -- the model ---------------------------------------------------------------------------
def test_glstm_model_fourier_train_step(dev, x3):
    from cnn_graph_amd.gconv_lstm import GLSTMModel
    L, M = laplacian("A")
    N, T, Fin, H, Fout = 2, 3, 2, 32, 2
    kw = dict(num_hidden=H, K=3, layer_count=1, out_features=Fout, keep_prob=1.0, device=dev, seed=5,
              filter="fourier_conv")
    m1, m2 = GLSTMModel(L, N, T, Fin, **kw), GLSTMModel(L, N, T, Fin, **kw)
    assert tuple(m1.W_fc.shape) == (M, Fout, H) and m1.cells[0].fused
    assert m1.flat.numel() == M * 4 * H * (Fin + H) + 4 * H + M * Fout * H
    U64 = npy(m1.U).astype(np.float64)
    P = params_np(m1.cells[0])
    Wfc = npy(m1.W_fc).astype(np.float64)
    rng = np.random.default_rng(9)
    xs, labels = r32(rng.standard_normal((T, N, M, Fin))), r32(rng.standard_normal((N, M, Fout)))
    for m in (m1, m2):
        loss = m.train_step(t(xs, dev), t(labels, dev))
    torch.cuda.synchronize()
    hs, cs, caches = FR.layer_forward(xs, P, U64)
    assert FR.max_az(caches) < 1.3
    out, hhat = FO.fourier_forward(hs[-1], Wfc, U64)
    ref_loss = np.mean((labels - out) ** 2)
    assert abs(float(loss) - ref_loss) < TOL * ref_loss
    dh, dWfc = FO.fourier_backward(2 * (out - labels) / out.size, Wfc, U64, hhat)
    _, _, _, dWx, dWh, db = FR.layer_backward(np.zeros_like(hs), None, caches, P, U64, dhT=dh)
    grads = m1.gradients()
    for p in m1.params:  # every gradient lives in the flat bucket
        assert m1.grad.data_ptr() <= p.grad.data_ptr() < m1.grad.data_ptr() + 4 * m1.grad.numel()
    for (name, g), ref in zip(grads.items(), (dWx, dWh, db, dWfc)):
        check(name, g, ref)
    assert torch.equal(m1.flat, m2.flat)  # same seed, same step: bitwise-equal parameters
    assert not torch.equal(m1.flat[:8], t(P[0].reshape(-1)[:8], dev))  # and the step moved them


# -- the constructor ------------------------------------------------------------------------
def test_fourier_cell_constructs_and_rejects(dev):
    from cnn_graph_amd.gconv_lstm import GConvLSTMCell
    L, M = laplacian("A")
    H, Fin = 32, 2
    cell = make_cell("A", Fin, H, "reference", dev, seed=1)
    assert tuple(cell.Wx.shape) == (M, 4 * H, Fin) and tuple(cell.Wh.shape) == (M, 4 * H, H)
    v = cell.variables
    assert tuple(v["Wzht"].shape) == (M, H, H) and tuple(v["Woxt"].shape) == (M, H, Fin)
    assert tuple(v["bft"].shape) == (H,)
    assert v["Wiht"].data_ptr() == cell.Wh[:, H:2 * H, :].data_ptr()
    assert tuple(cell.U.shape) == (M, M) and cell.fused and not hasattr(cell, "plan")
    assert float(cell.Wx.detach().abs().max()) <= 0.1 and float(cell.Wh.detach().abs().max()) <= 0.1
    odd = make_cell("A", Fin, 12, "reference", dev, seed=1)  # H % 8 != 0: the composition
    assert not odd.fused
    with pytest.raises(ValueError):
        make_cell("A", Fin, H, "reference", dev, seed=1, hconv="seq")
    with pytest.raises(ValueError):
        make_cell("A", Fin, 12, "reference", dev, seed=1, hconv="fused")
    with pytest.raises(NotImplementedError):
        GConvLSTMCell(H, laplacian=L, feat_in=Fin, filter_type="nope", device=dev)
