"""Row-class, ragged-tile and directed-graph parity of the kernels that keep
L~ (or L~^T) as CSR in LDS (csrc/lds_spmm.h): k_lstm_seq, k_xbasis, k_lstm_bstep
(lstm_seq.hip), k_lstm_hstep (lstm_fused.hip) and the channel-group kernels of
cheb_group.hip, on the small graphs and shapes of tests/resident_cases.py (whose
coverage claims tests/test_resident_cases_cpu.py checks without a GPU).

Every test first asserts that the kernel under test is the one that runs (the
*_supported queries, ChebPlan.stream_dispatch, the plan's CSR), then the
project's bars: Chebyshev planes, pre-filled with NaN, BITWISE equal to the
oracle's fp32 CSR-order recurrence (a wrong row class, parity select, padding
row or row order cannot hide behind MFMA rounding there); states and gradients
within 1e-5 (normwise) of the float64 oracles on the directed L~ / L~^T; the
bitwise and 1e-6 cross-path identities of test_gpu_lstm.py / test_gpu_group.py."""
import numpy as np
import pytest

import resident_cases as RC
from oracle import cheb_oracle as O
from oracle import lstm_oracle as LO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
H = RC.H
NAN = float("nan")


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


_PLANS = {}


def plan_for(gname, path="auto", variant="auto"):
    """ChebPlan straight from the graph's CSR (cached)."""
    key = (gname, path, variant)
    if key not in _PLANS:
        from cnn_graph_amd.plan import ChebPlan
        _PLANS[key] = ChebPlan(RC.csr(gname), device=0, path=path, variant=variant)
        for a, b in zip((_PLANS[key].rowptr, _PLANS[key].col, _PLANS[key].val), RC.graph(gname)):
            assert np.array_equal(a, b)
    return _PLANS[key]


def t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def lap64(gname):
    rp, ci, v = RC.graph(gname)
    return rp, ci, v.astype(np.float64)


def nans(dev, *shape):
    return torch.full(shape, NAN, device=dev, dtype=torch.float32)


def fp32_planes(gname, x, K):
    """The oracle's fp32 CSR-order recurrence of x [B, M, F]: [K, B*M, F]."""
    rp, ci, v = RC.graph(gname)
    B, M, F = x.shape
    A, _ = O.cheb_forward(x, rp, ci, v, np.zeros((F * K, 1), np.float32), K)
    return np.ascontiguousarray(A.reshape(B * M, F, K).transpose(2, 0, 1))


def check_err(name, got, ref, tol=TOL):
    err = O.normwise_err(got.detach().cpu().numpy(), ref)
    print(f"{name}: normwise err {err:.3e}")
    assert err < tol, (name, err)


_SEQ_REFS = {}


def seq_ref(c):
    """(inputs, hs, cs, caches) of the float64 oracle on one forward case, once."""
    if c["name"] not in _SEQ_REFS:
        d = RC.lstm_inputs(c)
        p = [f64(d[k]) for k in ("Wx", "Wh", "b")]
        hs, cs, caches = LO.layer_forward(f64(d["xs"]), p, lap64(c["graph"]), c["K"], H, f64(d["c0"]),
                                          f64(d["h0"]), c["gates"])
        _SEQ_REFS[c["name"]] = (d, p, hs, cs, caches)
    return _SEQ_REFS[c["name"]]


def run_seq(plan, c, d, dev, mode, planes_fill=NAN):
    """One k_lstm_seq launch.  mode "gx": the x-conv precomputed; "x": fused in
    (the caller sets seq_xpre).  Returns (hs, cs, act, h planes or None, x planes
    or None), every output pre-filled with NaN."""
    from cnn_graph_amd import ops
    Tn, N, M, Fin, K = c["T"], c["N"], plan.M, c["Fin"], c["K"]
    R = Tn * N * M
    xs, Wx, Wh, b, c0, h0 = (t(d[k], dev) for k in ("xs", "Wx", "Wh", "b", "c0", "h0"))
    hs, cs, act = nans(dev, Tn, N, M, H), nans(dev, Tn, N, M, H), nans(dev, R, 4 * H)
    pl = torch.full((K - 1, R, H), planes_fill, device=dev) if K > 1 else None
    kw = dict(h0=h0, c0=c0, out_hs=hs, out_cs=cs, out_act=act, planes=None if pl is None else pl[0],
              plane_stride=R * H if K > 1 else 0)
    xpl = None
    if mode == "gx":
        _, gx = ops.cheb_forward(plan, xs.view(Tn * N, M, Fin), Wx, K)
        ops.lstm_seq_forward(plan, gx.view(Tn, N, M, 4 * H), Wh, b, K, Tn, N, c["gates"], **kw)
    else:
        xpl = nans(dev, K, R, Fin)
        ops.lstm_seq_forward_x(plan, xs, Wx, Wh, b, K, c["gates"], xplanes=xpl, **kw)
    torch.cuda.synchronize()
    assert ops.lstm_seq_fault(plan, wait=True) is False
    for name, a in (("hs", hs), ("cs", cs), ("act", act)):
        assert not bool(torch.isnan(a).any()), f"{name} not fully written: {c['name']} {mode}"
    return hs, cs, act, pl, xpl


def check_h_planes(c, d, hs, pl, what):
    """T_k(h_{t-1}), k >= 1, of every step with an h-conv: bitwise the fp32
    recurrence of the h the kernel itself returned."""
    Tn, N, K = c["T"], c["N"], c["K"]
    if K == 1:
        return
    M = hs.shape[2]
    hs_np, pl_np = hs.cpu().numpy(), pl.cpu().numpy().reshape(K - 1, Tn, N * M, H)
    for step in range(Tn):
        hprev = d["h0"] if step == 0 else hs_np[step - 1]
        if hprev is None:
            continue   # a zero state's step 0 has no h-conv
        ref = fp32_planes(c["graph"], hprev, K)
        got = pl_np[:, step]
        assert not np.isnan(got).any(), f"h planes not fully written: {c['name']} {what} t={step}"
        assert np.array_equal(got, ref[1:]), f"h planes not bit-exact: {c['name']} {what} t={step}"


def check_x_planes(c, d, xpl, what):
    Tn, N, Fin, K = c["T"], c["N"], c["Fin"], c["K"]
    M = d["xs"].shape[2]
    got = xpl.cpu().numpy()
    assert not np.isnan(got).any(), f"x planes not fully written: {c['name']} {what}"
    ref = fp32_planes(c["graph"], d["xs"].reshape(Tn * N, M, Fin), K)
    assert np.array_equal(got, ref), f"x planes not bit-exact: {c['name']} {what}"


@pytest.mark.parametrize("c", RC.SEQ_CASES, ids=[c["name"] for c in RC.SEQ_CASES])
def test_seq_forward_vs_oracle(dev, cg_opts, c):
    """k_lstm_seq three ways -- precomputed gx, the x-conv fused in with the x
    recurrence inside the kernel (CG_OPT_SEQ_XPRE = 0) and with the default
    pre-pass: hs and cs against the float64 layer oracle, h and x planes
    bitwise, nothing left NaN, no hand-off fault."""
    from cnn_graph_amd import ops
    plan = plan_for(c["graph"])
    assert ops.lstm_seq_supported(plan, H, c["K"])
    assert ops.lstm_seq_x_supported(plan, c["Fin"], H, c["K"])
    d, _, r_hs, r_cs, _ = seq_ref(c)
    for what, mode, xpre in (("gx", "gx", None), ("x in-kernel", "x", 0), ("x pre-pass", "x", 1)):
        if xpre is not None:
            cg_opts("seq_xpre", xpre)
        hs, cs, _, pl, xpl = run_seq(plan, c, d, dev, mode)
        check_err(f"{c['name']} {what} hs", hs, r_hs)
        check_err(f"{c['name']} {what} cs", cs, r_cs)
        check_h_planes(c, d, hs, pl, what)
        if xpl is not None:
            check_x_planes(c, d, xpl, what)


@pytest.mark.parametrize("c", RC.XBASIS_CASES, ids=[c["name"] for c in RC.XBASIS_CASES])
def test_xbasis_prepass(dev, cg_opts, c):
    """The one-launch LDS pre-pass k_xbasis (CG_OPT_SEQ_XPRE = 1; rows of
    exactly kXL = 16 entries, values that differ between L~ and L~^T) against
    one streaming launch per order (= 2): x planes bitwise the fp32 recurrence
    in both modes, hs / cs / act / h planes bitwise equal between them, hs
    against the oracle.  On dir101 (a 17-entry row) mode 1 falls back to the
    streaming launches: the same assertions hold."""
    from cnn_graph_amd import ops
    plan = plan_for(c["graph"])
    rp = plan.rowptr
    assert ops.lstm_seq_x_supported(plan, c["Fin"], H, c["K"])
    assert RC.xbasis_applies(plan.M, c["Fin"], c["K"], int(np.diff(rp).max())) == c["xbasis"]
    d, _, r_hs, _, _ = seq_ref(c)
    out = {}
    for xpre in (1, 2):
        cg_opts("seq_xpre", xpre)
        hs, cs, act, pl, xpl = run_seq(plan, c, d, dev, "x", planes_fill=0.0)
        check_x_planes(c, d, xpl, f"seq_xpre={xpre}")
        out[xpre] = (hs, cs, act, pl, xpl)
    for name, a, b in zip(("hs", "cs", "act", "h planes", "x planes"), out[1], out[2]):
        assert torch.equal(a, b), f"{name} differs between seq_xpre 1 and 2: {c['name']}"
    check_err(f"{c['name']} hs", out[1][0], r_hs)
    check_h_planes(c, d, out[1][0], out[1][3], "seq_xpre=1")


@pytest.mark.parametrize("c", RC.HSTEP_CASES, ids=[c["name"] for c in RC.HSTEP_CASES])
def test_hstep_vs_oracle(dev, c):
    """k_lstm_hstep: c' and h' against LO.cell_forward (gx from the float64
    x-conv, rounded to fp32), its planes bitwise."""
    from cnn_graph_amd import ops
    plan = plan_for(c["graph"])
    K, N, M = c["K"], c["N"], plan.M
    assert ops.lstm_hconv_supported(plan, H, K)
    d = RC.lstm_inputs(c)
    p = [f64(d[k]) for k in ("Wx", "Wh", "b")]
    x = f64(d["xs"][0])
    _, gx = LO.cheb_conv64(x, lap64(c["graph"]), p[0], K)
    cn, hn, _ = LO.cell_forward(x, f64(d["c0"]), f64(d["h0"]), *p, lap64(c["graph"]), K, H, c["gates"])
    pl = nans(dev, K - 1, N * M, H) if K > 1 else None
    oc, oh, oa = nans(dev, N, M, H), nans(dev, N, M, H), nans(dev, N, M, 4 * H)
    ops.lstm_hconv_step(plan, t(d["h0"], dev), t(d["c0"], dev), t(gx, dev), t(d["Wh"], dev), t(d["b"], dev),
                        K, c["gates"], out_c=oc, out_h=oh, out_act=oa,
                        planes=None if pl is None else pl[0], plane_stride=N * M * H if K > 1 else 0)
    torch.cuda.synchronize()
    for name, a in (("c'", oc), ("h'", oh), ("act", oa)):
        assert not bool(torch.isnan(a).any()), f"{name} not fully written: {c['name']}"
    check_err(f"{c['name']} c'", oc, cn)
    check_err(f"{c['name']} h'", oh, hn)
    if K > 1:
        got = pl.cpu().numpy()
        assert not np.isnan(got).any()
        assert np.array_equal(got, fp32_planes(c["graph"], d["h0"], K)[1:]), f"planes not bit-exact: {c['name']}"


@pytest.mark.parametrize("c", RC.BSTEP_CASES, ids=[c["name"] for c in RC.BSTEP_CASES])
def test_bstep_vs_oracle(dev, c):
    """k_lstm_bstep over L~^T in tlorder: dpre and dc_prev bitwise equal to
    lstm_cell_backward, dh_prev within 1e-5 of LO.cell_backward (float64, the
    directed L~^T) and within 1e-6 of the dx-only chebyshev5 backward of the
    same dpre; both act layouts and the pointwise-only call bitwise; every
    optional input present and absent.  A kernel that read L~ for L~^T would
    pass on hub301 (symmetric) and fail on the dir* graphs.  The row ORDER is
    not checkable by results: the kernel takes each switch's bound from the rows
    it was dealt, so any permutation (lorder for tlorder, say) gives the same
    bits and only costs time."""
    from cnn_graph_amd import ops
    plan = plan_for(c["graph"])
    K, N, M, gates = c["K"], c["N"], plan.M, c["gates"]
    assert ops.lstm_seq_supported(plan, H, K)
    d = RC.bstep_inputs(c)
    g = {k: t(v, dev) for k, v in d.items()}
    act, Wh, c_out = g["act"], g["Wh"], g["c_out"]
    act_um = act.view(N, M, 4, H).transpose(-1, -2).contiguous()
    a64 = f64(d["act"])
    zeros = np.zeros((N, M, H))
    for opt in (("dh", "dh_rec", "dc", "c_prev"), ("dh",), ("dh_rec", "dc", "c_prev")):
        a_dh, a_dhr, a_dc, a_cp = (g[k] if k in opt else None for k in ("dh", "dh_rec", "dc", "c_prev"))
        dpre, dcp, dhp = ops.lstm_bwd_step(plan, a_dh, a_dhr, a_dc, act, a_cp, c_out, Wh, K, gates,
                                           out_dpre=nans(dev, N, M, 4 * H), out_dh_prev=nans(dev, N, M, H))
        rdpre, rdcp = ops.lstm_cell_backward(a_dh, a_dhr, a_dc, act, a_cp, c_out, H, gates)
        rdhp, _ = ops.cheb_backward(plan, rdpre.view(N, M, 4 * H), None, Wh, K, need_dW=False)
        torch.cuda.synchronize()
        what = f"{c['name']} {'+'.join(opt)}"
        assert not bool(torch.isnan(dhp).any()), f"dh_prev not fully written: {what}"
        assert torch.equal(dpre, rdpre), f"dpre: {what}"
        assert torch.equal(dcp, rdcp), f"dc_prev: {what}"
        n64 = lambda k: f64(d[k]) if k in opt else zeros  # noqa: E731
        cache = dict(z=a64[..., :H], i=a64[..., H:2 * H], f=a64[..., 2 * H:3 * H], o=a64[..., 3 * H:],
                     c=n64("c_prev"), cn=f64(d["c_out"]), x=np.zeros((N, M, 1)), Ax=np.zeros((N * M, K)),
                     Ah=np.zeros((N * M, H * K)), N=N, M=M)
        ref = LO.cell_backward(n64("dh") + n64("dh_rec"), n64("dc"), cache, np.zeros((K, 4 * H)),
                               f64(d["Wh"]), lap64(c["graph"]), K, H, gates)
        check_err(f"{what} dpre", dpre, ref[6])
        check_err(f"{what} dc_prev", dcp, ref[1])
        check_err(f"{what} dh_prev", dhp, ref[2])
        check_err(f"{what} dh_prev of cheb_backward", rdhp, ref[2])
        check_err(f"{what} dh_prev across paths", dhp, rdhp.cpu().numpy().astype(np.float64), 1e-6)
        d2, c2, h2 = ops.lstm_bwd_step(plan, a_dh, a_dhr, a_dc, act_um, a_cp, c_out, Wh, K, gates,
                                       act_unit_major=True)
        assert torch.equal(d2, dpre) and torch.equal(c2, dcp) and torch.equal(h2, dhp), what
        for a, um in ((act, False), (act_um, True)):
            d3, c3, h3 = ops.lstm_bwd_step(plan, a_dh, a_dhr, a_dc, a, a_cp, c_out, Wh, K, gates,
                                           act_unit_major=um, need_dh_prev=False)
            assert h3 is None and torch.equal(d3, dpre) and torch.equal(c3, dcp), what


_LAYER_REFS = {}


def layer_ref(c):
    if c["name"] not in _LAYER_REFS:
        d, p, hs, cs, caches = seq_ref(c)
        rng = np.random.default_rng(len(c["name"]))
        gh = rng.standard_normal(hs.shape).astype(np.float32)
        gc = rng.standard_normal(cs[-1].shape).astype(np.float32)
        dxs, dc0, dh0, dWx, dWh, db = LO.layer_backward(f64(gh), f64(gc), caches, p, lap64(c["graph"]),
                                                        c["K"], H, c["gates"])
        _LAYER_REFS[c["name"]] = (d, gh, gc, dict(hs=hs, cT=cs[-1], dxs=dxs, dc0=dc0, dh0=dh0, dWx=dWx,
                                                  dWh=dWh, db=db))
    return _LAYER_REFS[c["name"]]


_LAPLACIANS = {}


@pytest.mark.parametrize("hconv", ["seq", "fused", "unfused"])
@pytest.mark.parametrize("c", RC.LAYER_CASES, ids=[c["name"] for c in RC.LAYER_CASES])
def test_layer_autograd_vs_oracle(dev, c, hconv):
    """layer(cell, xs, (c0, h0)) under autograd on a graph whose L~^T differs
    from L~ (and on the hub graph): states and every gradient against
    LO.layer_backward.  The cell's plan holds the CSR as given."""
    from cnn_graph_amd.gconv_lstm import GConvLSTMCell, layer
    L = _LAPLACIANS.setdefault(c["graph"], RC.laplacian_for(c["graph"]))
    cell = GConvLSTMCell(H, laplacian=L, lmax=2, K=c["K"], feat_in=c["Fin"], gates=c["gates"], device=dev,
                         hconv=hconv)
    for a, b in zip((cell.plan.rowptr, cell.plan.col, cell.plan.val), RC.graph(c["graph"])):
        assert np.array_equal(a, b), "the cell's plan does not hold the graph as given"
    assert cell.seq == (hconv == "seq") and cell.fused == (hconv != "unfused")
    assert cell.seq_x == (hconv == "seq")
    d, gh, gc, ref = layer_ref(c)
    with torch.no_grad():
        cell.Wx.copy_(t(d["Wx"], dev))
        cell.Wh.copy_(t(d["Wh"], dev))
        cell.b.copy_(t(d["b"], dev))
    xs, c0, h0 = (t(d[k], dev).requires_grad_() for k in ("xs", "c0", "h0"))
    hs, (cT, _) = layer(cell, xs, (c0, h0))
    ((hs * t(gh, dev)).sum() + (cT * t(gc, dev)).sum()).backward()
    torch.cuda.synchronize()
    got = dict(hs=hs, cT=cT, dxs=xs.grad, dc0=c0.grad, dh0=h0.grad, dWx=cell.Wx.grad, dWh=cell.Wh.grad,
               db=cell.b.grad)
    for name in ("hs", "cT", "dxs", "dc0", "dh0", "dWx", "dWh", "db"):
        check_err(f"{c['name']} {hconv} {name}", got[name], ref[name])


def _group_run(plan, c, dev, xd, Wd, dyd):
    from cnn_graph_amd import ops
    r = ops.ChebRunner(plan, c["N"], c["Fin"], c["K"], c["Fout"], dev, basis_layout=c["layout"])
    r.basis.fill_(NAN)
    r.dx.fill_(NAN)
    r.forward(xd, Wd)
    r.backward(dyd, Wd)
    torch.cuda.synchronize()
    return r.basis_rows().cpu().numpy(), r.y.cpu().numpy(), r.dx.cpu().numpy(), r.dW.cpu().numpy(), r


@pytest.mark.parametrize("c", RC.GROUP_CASES, ids=[c["name"] for c in RC.GROUP_CASES])
def test_group_kernels(dev, cg_opts, c):
    """k_grp16_fwd / k_grp_fwd (planes layout) and k_grp_clen_dy / k_grp_clen
    against variant 'steps' and the oracle, with the bars of test_gpu_group.py:
    basis bitwise equal to 'steps' and to the fp32 recurrence; with the steps
    path on the f32-MFMA row GEMM (CG_OPT_GEMM_X3 = 0) y within 1e-6 and dx
    BITWISE equal; dx and dW within 1e-5 of O.cheb_backward, under either row
    GEMM; a grp16 case again with CG_OPT_GRP16 = 0 (k_grp_fwd<1>); the
    accumulate case dx0 + dx exactly."""
    from cnn_graph_amd import _lib, ops
    N, Fin, K, Fout = (c[k] for k in ("N", "Fin", "K", "Fout"))
    shape = (N, Fin, K, Fout)
    auto, steps = plan_for(c["graph"], "stream"), plan_for(c["graph"], "stream", "steps")
    assert auto.query_path(*shape) == "stream" and steps.query_path(*shape) == "stream"
    da, ds = auto.stream_dispatch(*shape, layout=c["layout"]), steps.stream_dispatch(*shape, layout=c["layout"])
    assert (da["wide"], da["group_fwd"], da["group_bwd"]) == (0, 1 if c["fwd"] else 0, c["bwd"]), da
    assert (ds["wide"], ds["group_fwd"], ds["group_bwd"]) == (0, 0, 0), ds
    rp, ci, v = RC.graph(c["graph"])
    M = auto.M
    x, W, dy, dx0 = RC.group_inputs(c)
    ob, oy = O.cheb_forward(x, rp, ci, v, W, K)
    odx, odW = O.cheb_backward(dy, ob, W, rp, ci, v, N, M, Fin, K)
    xd, Wd, dyd = t(x, dev), t(W, dev), t(dy, dev)
    runs = [("auto x3", auto, None, None), ("auto", auto, 0, None), ("steps", steps, 0, None)]
    if c["fwd"] == "grp16":
        runs.append(("auto grp16=0", auto, 0, 0))
    out = {}
    for what, plan, x3, g16 in runs:
        if x3 is not None:
            cg_opts("gemm_x3", x3)
        if g16 is not None:
            cg_opts("grp16", g16)
        basis, y, dx, dW, runner = out[what] = _group_run(plan, c, dev, xd, Wd, dyd)
        assert not np.isnan(basis).any() and not np.isnan(dx).any(), f"{c['name']} {what}: not fully written"
        assert np.array_equal(basis, ob), f"{c['name']} {what}: basis not bit-exact"
        errs = {n: O.normwise_err(a, b) for n, a, b in (("y", y, oy), ("dx", dx, odx), ("dW", dW, odW))}
        print(c["name"], what, {n: f"{e:.2e}" for n, e in errs.items()})
        for n, e in errs.items():
            assert e < TOL, f"{c['name']} {what}: {n} normwise error {e:.3e}"
    for what in [w for w in out if w.startswith("auto") and w != "auto x3"]:
        assert np.array_equal(out[what][0], out["steps"][0])
        assert np.array_equal(out[what][2], out["steps"][2]), f"{c['name']} {what}: dx differs from the steps path"
        err = O.normwise_err(out[what][1], out["steps"][1].astype(np.float64))
        assert err < 1e-6, f"{c['name']} {what}: y differs from the steps path by {err:.3e}"
    if c["accumulate"]:
        r = out["steps"][4]   # (the options are still those of the last run: gemm_x3 = 0)
        ra = ops.ChebRunner(auto, N, Fin, K, Fout, dev, basis_layout=c["layout"])
        ra.forward(xd, Wd)
        ra.backward(dyd, Wd)
        dxa = t(dx0, dev)
        dWa = torch.empty_like(Wd)
        _lib.check("cg_cheb_backward_layout", _lib.lib().cg_cheb_backward_layout(
            auto.handle, N, Fin, K, Fout, dyd.data_ptr(), None, _lib.CG_ACT_NONE,
            _lib.BASIS_LAYOUTS[c["layout"]], ra.basis.data_ptr(), Wd.data_ptr(), dxa.data_ptr(), 1,
            dWa.data_ptr(), None, ra.bws.data_ptr(), ra.bwd_bytes, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(dxa, t(dx0, dev) + ra.dx) and torch.equal(ra.dx, r.dx)
        assert torch.equal(dWa, ra.dW)
