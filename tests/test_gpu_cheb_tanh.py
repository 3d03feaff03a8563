"""tanh in the Chebyshev epilogue, y = tanh(basis W + residual) (CG_ACT_TANH of
cg_cheb_forward_layout / cg_cheb_backward_layout): one case per forward kernel
class that stores y, each with and without a residual.

Every case first asserts the class it names (ChebPlan.query_path /
stream_dispatch, as tests/test_gpu_stream_geometry.py does), then:
  * W is scaled so that the float64 pre-activations z have a standard deviation of
    6: asserted on the float64 side to hold |z| < 0.625 (gate_tanh's polynomial),
    0.625 < |z| < 4 (its exp / rcp arm) and |z| > 9 (saturation);
  * y within 1e-5 (max |y - y_ref| / max |y_ref|) of float64;
  * dz, dx, dW of the backward within 1e-5 of float64 computed on the GPU's own
    saved y, for dx = and dx += (nothing excluded);
  * y BITWISE equal to a second route: the same call with act = none (same
    kernels, so the same pre-activation, residual added), then cg_act_forward's
    k_act_fwd with tanh.  Every kernel applies cg::gate_tanh.
"""
import numpy as np
import pytest
import scipy.sparse

import resident_cases as RC
import stream_cases as S
from conftest import case, load_golden
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
SIGMA = 6.0


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _stream_case(name):
    c = next(c for c in S.CASES if c["name"] == name)
    return dict(c, csr=S.graph(c["graph"]), path="stream", kind="stream")


def _group_case(name):
    c = next(c for c in RC.GROUP_CASES if c["name"] == name)
    return dict(c, csr=RC.graph(c["graph"]), path="stream", variant="auto", kind="group")


def _golden_case(gname, kind, variant="auto", **shape):
    g = case(load_golden(gname))
    c = dict(name=f"{kind}_{gname[7]}", csr=(g["Lt_rowptr"], g["Lt_col"], g["Lt_val"]), path="auto",
             variant=variant, kind=kind, layout="rows", N=g["N"], Fin=g["Fin"], K=g["K"], Fout=g["Fout"])
    c.update(shape)
    return c


def _chord_case():
    return dict(name="fast_chord100", csr=RC.graph("chord100"), path="auto", variant="auto", kind="fast",
                layout="rows", N=4, Fin=1, K=5, Fout=8)


# id -> case.  The fast kernels take rows of at most 16 entries: chord100 (M 100 =
# 3 * 32 + 4) and graph B (M 976 = 30 * 32 + 16) both end in a ragged 32-row tile,
# Fout 8 < 32 lanes (8, not 4, so that the orders-layout query below can tell
# whether the fast kernels apply).  Graph A (M 100, N 4, K 5, Fin 1, Fout 4) has a row of 21
# entries, so it runs the kernels of cheb_resident.hip under variant auto too.
# The streaming shapes and graphs are the tables' own.
CASES = {
    "fast_chord100": _chord_case,
    "fast_B_ragged_tile": lambda: _golden_case("golden_B.npz", "fast", N=2, Fin=2, K=3, Fout=8),
    "resident_A": lambda: _golden_case("golden_A.npz", "resident", N=4, K=5, Fin=1, Fout=4),
    "resident_B_ragged_tile": lambda: _golden_case("golden_B.npz", "resident", variant="classic", N=2, Fin=1,
                                                   K=3, Fout=4),
    "group_grp16": lambda: _group_case("g_dir101_f16k5o2"),
    "group_grp16_off": lambda: dict(_group_case("g_hub301_f16k7o32"), grp16=0),
    "group_two_tiles": lambda: _group_case("g_hub301_f16k2o64"),
    "rowgemm_rows": lambda: _stream_case("n_fin3"),
    "rowgemm_rows_f32_mfma": lambda: dict(_stream_case("n_fin5"), gemm_x3=0),
    "rowgemm_planes": lambda: _stream_case("n_hub_fin16_planes"),
    "rowgemm_planes_f32_mfma": lambda: dict(_stream_case("n_fin64_planes"), gemm_x3=0),
    "wide_fused_last": lambda: _stream_case("w_b4_fin1"),
    "wide_assemble": lambda: _stream_case("w_b16_fin4"),
    "act_kernel_k1": lambda: _stream_case("w_b32_k1"),
}


def _plan(c):
    from cnn_graph_amd.plan import ChebPlan
    rp, ci, v = c["csr"]
    M = len(rp) - 1
    Lt = scipy.sparse.csr_matrix((v, ci, rp), shape=(M, M))
    return ChebPlan(Lt, device=0, path=c["path"], variant=c["variant"])


def _assert_class(plan, c):
    shape = (c["N"], c["Fin"], c["K"], c["Fout"])
    kind = c["kind"]
    if kind in ("fast", "resident"):
        # variant auto takes the fast kernels where the resident path applies, classic
        # the kernels of cheb_resident.hip
        assert plan.query_path(*shape) == "resident", c["name"]
        # the library's own answer: the orders basis layout is offered exactly where
        # the fast forward (and the fused-dW fast backward: Fin <= 2, Fout % 8 == 0)
        # runs -- asked at Fout 8 where the case's Fout is not a multiple of 8
        assert c["Fin"] <= 2
        fo = c["Fout"] if c["Fout"] % 8 == 0 else 8
        fast = plan.basis_elems(c["N"], c["Fin"], c["K"], fo, "orders") is not None
        assert fast == (kind == "fast"), c["name"]
        if kind == "fast":
            assert fo == c["Fout"]
        return
    assert plan.query_path(*shape) == "stream", c["name"]
    d = plan.stream_dispatch(*shape, layout=c["layout"])
    if kind == "group":
        assert c["fwd"] is not None and c["layout"] == "planes" and d["group_fwd"] == 1, (c["name"], d)
    else:
        assert d == c["expect"], (c["name"], d)


def _inputs(c, with_res):
    rp, ci, v = c["csr"]
    M = len(rp) - 1
    N, Fin, K, Fout = c["N"], c["Fin"], c["K"], c["Fout"]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) + int(with_res))
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    W = rng.standard_normal((Fin * K, Fout)).astype(np.float32)
    res = rng.standard_normal((N, M, Fout)).astype(np.float32) if with_res else None
    ob, z0 = O.cheb_forward(x, rp, ci, v, W, K)
    W = (W * np.float32(SIGMA / np.asarray(z0, np.float64).std())).astype(np.float32)
    ob, z = O.cheb_forward(x, rp, ci, v, W, K)
    z = np.asarray(z, np.float64).reshape(N, M, Fout)
    if with_res:
        z = z + res
    az = np.abs(z)
    # both arms of gate_tanh and its saturation are exercised
    assert np.count_nonzero(az < 0.625) > 0, c["name"]
    assert np.count_nonzero((az > 0.625) & (az < 4)) > 0, c["name"]
    assert np.count_nonzero(az > 9) > 0, c["name"]
    dy = rng.standard_normal((N, M, Fout)).astype(np.float32)
    dx0 = rng.standard_normal((N, M, Fin)).astype(np.float32)
    return x, W, res, ob, z, dy, dx0


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("cid", list(CASES))
def test_tanh_store_and_backward(dev, cg_opts, cid, with_res):
    from cnn_graph_amd import ops
    c = CASES[cid]()
    for opt in ("grp16", "gemm_x3"):
        if opt in c:
            cg_opts(opt, c[opt])
    plan = _plan(c)
    _assert_class(plan, c)
    rp, ci, v = c["csr"]
    M = len(rp) - 1
    N, Fin, K, Fout, lay = c["N"], c["Fin"], c["K"], c["Fout"], c["layout"]
    x, W, res, ob, z, dy, dx0 = _inputs(c, with_res)
    xd, Wd, dyd = t(x, dev), t(W, dev), t(dy, dev)
    rd = t(res, dev) if with_res else None

    basis, y = ops.cheb_forward(plan, xd, Wd, K, residual=rd, act="tanh", layout=lay)
    # the second route: the same kernels without the activation, then k_act_fwd
    _, y2 = ops.cheb_forward(plan, xd, Wd, K, residual=rd, act="none", layout=lay)
    ops.act_forward_(y2, None, "tanh")
    torch.cuda.synchronize()
    yg = y.cpu().numpy()
    y_ref = np.tanh(z)
    err_y = np.abs(yg - y_ref).max() / np.abs(y_ref).max()
    print(f"{cid} res={with_res}: y error {err_y:.2e}, max |y| {np.abs(yg).max():.6f}")
    assert err_y <= TOL
    assert np.abs(yg).max() <= 1.0
    assert torch.equal(y, y2), f"{cid}: the fused store and k_act_fwd differ on the same pre-activation"

    # backward on the GPU's own saved y
    y64 = yg.astype(np.float64)
    dz_ref = dy.astype(np.float64) * (1.0 - y64 * y64)
    odx, odW = O.cheb_backward(dz_ref, ob, W, rp, ci, v, N, M, Fin, K)
    dx, dW, dz = ops.cheb_backward_ex(plan, dyd, y, "tanh", basis, Wd, K, layout=lay)
    dxa = t(dx0, dev)
    _, dW2, dz2 = ops.cheb_backward_ex(plan, dyd, y, "tanh", basis, Wd, K, dx=dxa, dx_accumulate=True,
                                       layout=lay)
    torch.cuda.synchronize()
    errs = dict(dz=O.normwise_err(dz.cpu().numpy(), dz_ref), dx=O.normwise_err(dx.cpu().numpy(), odx),
                dW=O.normwise_err(dW.cpu().numpy(), odW),
                dx_acc=O.normwise_err(dxa.cpu().numpy(), odx + dx0))
    print(f"{cid} res={with_res}:", {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= TOL, f"{cid}: {k} normwise error {e:.3e}"
    assert torch.equal(dz, dz2) and torch.equal(dW, dW2)


def test_fast_orders_layout_tanh_equals_rows(dev):
    """The orders-layout instantiations of the fast forward (Fin <= 2): y and, read
    back through the fused-dW backward, dx bitwise equal to the rows layout's, as the
    header states for every activation."""
    from cnn_graph_amd import _lib, ops
    c = _golden_case("golden_B.npz", "fast", N=2, Fin=1, K=4, Fout=8)
    plan = _plan(c)
    N, Fin, K, Fout = c["N"], c["Fin"], c["K"], c["Fout"]
    M = plan.M
    assert plan.query_path(N, Fin, K, Fout) == "resident"
    n_ob = plan.basis_elems(N, Fin, K, Fout, "orders")
    assert n_ob is not None and n_ob > N * M * Fin * K  # M = 976 is no multiple of 32
    x, W, res, _, _, dy, _ = _inputs(c, True)
    xd, Wd, rd, dyd = t(x, dev), t(W, dev), t(res, dev), t(dy, dev)
    basis, y = ops.cheb_forward(plan, xd, Wd, K, residual=rd, act="tanh")
    dx, dW, dz = ops.cheb_backward_ex(plan, dyd, y, "tanh", basis, Wd, K)
    f = dict(device=dev, dtype=torch.float32)
    b_o, y_o = torch.empty(n_ob, **f), torch.empty((N, M, Fout), **f)
    dx_o, dW_o, dz_o = torch.empty_like(dx), torch.empty_like(dW), torch.empty_like(dz)
    fwd_ws, bwd_ws = plan.workspace_bytes(N, Fin, K, Fout)
    ws = torch.empty(max(fwd_ws, bwd_ws, 1), device=dev, dtype=torch.uint8)
    s = torch.cuda.current_stream().cuda_stream
    h = _lib.lib()
    _lib.check("cg_cheb_forward_layout", h.cg_cheb_forward_layout(
        plan.handle, N, Fin, K, Fout, xd.data_ptr(), Wd.data_ptr(), rd.data_ptr(), _lib.CG_ACT_TANH,
        _lib.CG_BASIS_ORDERS, b_o.data_ptr(), y_o.data_ptr(), ws.data_ptr(), ws.numel(), s))
    _lib.check("cg_cheb_backward_layout", h.cg_cheb_backward_layout(
        plan.handle, N, Fin, K, Fout, dyd.data_ptr(), y_o.data_ptr(), _lib.CG_ACT_TANH, _lib.CG_BASIS_ORDERS,
        b_o.data_ptr(), Wd.data_ptr(), dx_o.data_ptr(), 0, dW_o.data_ptr(), dz_o.data_ptr(), ws.data_ptr(),
        ws.numel(), s))
    torch.cuda.synchronize()
    assert torch.equal(y_o, y) and torch.equal(dz_o, dz) and torch.equal(dx_o, dx)
    assert O.normwise_err(dW_o.cpu().numpy(), dW.cpu().numpy().astype(np.float64)) < TOL


@pytest.mark.parametrize("cid", ["fast_chord100", "group_grp16", "rowgemm_rows", "wide_assemble"])
def test_cheb_conv_tanh_autograd_equals_the_explicit_backward(dev, cid):
    """ops.cheb_conv(..., act='tanh'): y and the gradients of x, W and the residual
    bitwise equal cg_cheb_backward_layout called by hand on the same tensors."""
    from cnn_graph_amd import ops
    c = CASES[cid]()
    plan = _plan(c)
    K = c["K"]
    x, W, res, _, _, dy, _ = _inputs(c, True)
    xd, Wd, rd, dyd = (t(a, dev).requires_grad_() for a in (x, W, res, dy))
    y = ops.cheb_conv(xd, Wd, plan, K, residual=rd, act="tanh")
    y.backward(dyd.detach())
    lay = ops.basis_layout_for(plan, c["N"], c["Fin"], K, c["Fout"])
    basis, y_e = ops.cheb_forward(plan, xd.detach(), Wd.detach(), K, residual=rd.detach(), act="tanh",
                                  layout=lay)
    dx, dW, dz = ops.cheb_backward_ex(plan, dyd.detach(), y_e, "tanh", basis, Wd.detach(), K, layout=lay)
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), y_e)
    assert torch.equal(xd.grad, dx) and torch.equal(Wd.grad, dW) and torch.equal(rd.grad, dz)


def test_relu_mask_is_unchanged_and_tanh_mask_paths_agree(dev):
    """The one mask kernel of the backward: ReLU's dz is y > 0 ? dy : 0 exactly, and
    the float4 and the scalar form (an n that is no multiple of 4) give tanh's
    dy (1 - y^2) with the same bits (torch computes the expected values on the CPU)."""
    from cnn_graph_amd import ops
    c = CASES["fast_chord100"]()
    plan = _plan(c)
    K = c["K"]
    for N in (4, 3):  # N * 100 * Fout floats; Fout = 1 at N = 3 is no multiple of 4
        Fout = 4 if N == 4 else 1
        rng = np.random.default_rng(N)
        x = t(rng.standard_normal((N, 100, 1)), dev)
        W = t(rng.standard_normal((K, Fout)), dev)
        dy = t(rng.standard_normal((N, 100, Fout)), dev)
        for act in ("relu", "tanh"):
            basis, y = ops.cheb_forward(plan, x, W, K, act=act)
            _, _, dz = ops.cheb_backward_ex(plan, dy, y, act, basis, W, K)
            torch.cuda.synchronize()
            yc, dc = y.cpu(), dy.cpu()
            want = torch.where(yc > 0, dc, torch.zeros_like(dc)) if act == "relu" else dc * (1 - yc * yc)
            assert torch.equal(dz.cpu(), want), (N, act)


def test_tanh_backward_needs_y_and_dz(dev):
    from cnn_graph_amd import _lib
    c = CASES["fast_chord100"]()
    plan = _plan(c)
    N, Fin, K, Fout = c["N"], c["Fin"], c["K"], c["Fout"]
    M = plan.M
    f = dict(device=dev, dtype=torch.float32)
    dy, y, dz = (torch.zeros((N, M, Fout), **f) for _ in range(3))
    basis, W = torch.zeros((N * M, Fin * K), **f), torch.zeros((Fin * K, Fout), **f)
    dx, dW = torch.zeros((N, M, Fin), **f), torch.zeros((Fin * K, Fout), **f)
    h = _lib.lib()
    for yp, zp in ((None, dz.data_ptr()), (y.data_ptr(), None)):
        st = h.cg_cheb_backward_layout(plan.handle, N, Fin, K, Fout, dy.data_ptr(), yp, _lib.CG_ACT_TANH,
                                       _lib.CG_BASIS_ROWS, basis.data_ptr(), W.data_ptr(), dx.data_ptr(), 0,
                                       dW.data_ptr(), zp, None, 0, None)
        assert st == _lib.CG_ERR_ARG
        assert h.cg_last_error().decode() == "tanh backward needs y (its output) and dz"
    st = h.cg_cheb_forward_layout(plan.handle, N, Fin, K, Fout, dy.data_ptr(), W.data_ptr(), None, 3,
                                  _lib.CG_BASIS_ROWS, basis.data_ptr(), y.data_ptr(), None, 0, None)
    assert st == _lib.CG_ERR_ARG and h.cg_last_error().decode() == "unknown activation 3"
