"""The residual GraphConv block with the Fourier filter on the MFMA transforms
(cg_fres_forward / cg_fres_backward: k_gft's activation store and masked
staging, k_fmix) and ResGNN / StackedResGNN(filter="fourier") on top of them.

  * every filter option against float64 at tile-edge shapes, outputs between
    NaN guard bands: the project's bar, normwise error < 1e-5;
  * integer operands compared BITWISE with float64, the ReLU-clamped entries
    and the ``dx +=`` form included;
  * three Adam steps against tests/fourier_resgnn_ref.py;
  * determinism, and the same gradients from GraphConv under autograd.
Inputs and shapes: tests/fourier_res_cases.py (premises checked without a GPU
in tests/test_fourier_resgnn_ref_cpu.py)."""
import functools
import itertools

import numpy as np
import pytest

import fourier_edge_cases as FE
import fourier_res_cases as FC
import fourier_resgnn_ref as RR
from oracle import cheb_oracle as O
from oracle import model_oracle as MO
from test_gpu_fourier_edges import Guarded, t64
from test_gpu_fourier_lstm import laplacian, t

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5


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


def f64(x):
    return x.detach().cpu().numpy().astype(np.float64)


def err_of(got, ref):
    return O.normwise_err(f64(got) if torch.is_tensor(got) else got, ref)


@functools.lru_cache(maxsize=None)
def parity_forward_ref(shape, act, residual):
    c = FC.parity_case(*shape)
    return FC.parity_ref(c, act, residual)


# -- 1. every option of one filter against float64 ----------------------------------------
@pytest.mark.parametrize("M,N,Fin,Fout", FC.SHAPES)
def test_filter_options_vs_float64(dev, x3, M, N, Fin, Fout):
    """act x residual x {dx NULL, assigned, accumulated onto a non-zero buffer}
    x dz, every output inside NaN guard bands.  The backward's reference takes
    the ReLU mask from the GPU's own y (a pre-activation within rounding of 0
    may clamp either way; the forward's y itself is held to the bar)."""
    from cnn_graph_amd import ops
    shape = (M, N, Fin, Fout)
    c = FC.parity_case(*shape)
    B = ops.gft_prepare(t(c["U"], dev))
    W, x, res, dy = (t(c[k], dev) for k in ("W", "x", "res", "dy"))
    worst = 0.0
    for act, residual in itertools.product(("none", "relu"), (False, True)):
        ry, rxhat = parity_forward_ref(shape, act, residual)
        rxhat = RR.spectrum_nmc(rxhat)
        gx, gy = Guarded((N, M, Fin), dev), Guarded((N, M, Fout), dev)
        ops.fres_forward(B, W, x, res if residual else None, act, out_xhat=gx.flat, out_y=gy.flat)
        torch.cuda.synchronize()
        xhat, y = gx.verify("xhat"), gy.verify("y")
        errs = {"xhat": err_of(xhat, rxhat), "y": err_of(y, ry)}
        mask = (f64(y) > 0) if act == "relu" else 1.0
        rdz = c["dy"] * mask
        rdx, rdW, _ = RR.filter_backward(rdz, None, "none", c["W"], c["U"],
                                         np.transpose(rxhat, (0, 2, 1)))
        for dxmode, want_dz in itertools.product(("null", "assign", "accumulate"), (False, True)):
            name = f"{act} res={residual} dx={dxmode} dz={want_dz}"
            gW = Guarded((M, Fout, Fin), dev)
            gz = Guarded((N, M, Fout), dev) if want_dz else None
            gd = None
            if dxmode != "null":
                gd = Guarded((N, M, Fin), dev, t(c["dx0"], dev) if dxmode == "accumulate" else None)
            ops.fres_backward(B, W, xhat, dy, y if act == "relu" else None, act, need_dz=want_dz,
                              dx=None if gd is None else gd.out, dx_accumulate=dxmode == "accumulate",
                              need_dx=gd is not None, out_dz=None if gz is None else gz.out,
                              out_dW=gW.out)
            torch.cuda.synchronize()
            errs[name + " dW"] = err_of(gW.verify("dW"), rdW)
            if gz is not None:  # a select of dy: bitwise
                assert torch.equal(gz.verify("dz").double(), t64(RR.r32(rdz), dev)), name
            if gd is not None:
                ref = rdx + (c["dx0"] if dxmode == "accumulate" else 0.0)
                errs[name + " dx"] = err_of(gd.verify("dx"), ref)
        bad = {k: v for k, v in errs.items() if not v < TOL}
        assert not bad, bad
        worst = max(worst, max(errs.values()))
    print(f"fres {shape} x3={x3}: worst normwise error {worst:.2e}")


# -- 2. bitwise on integers -----------------------------------------------------------------
@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("M,N,Fin,Fout", FC.SHAPES)
def test_filter_is_exact_on_integers(dev, x3, M, N, Fin, Fout, kind):
    """y, xhat, dz, dx (assigned and accumulated) and dW equal float64 bit for
    bit; every fifth pre-activation is exactly 0 (y == 0: dz == 0 and nothing
    of it in dW), and the perm cases carry 23 significant bits through the
    synthesis' on-the-fly split."""
    from cnn_graph_amd import ops
    c = FC.exact_case(M, N, Fin, Fout, kind)
    ref = {k: t64(v, dev) for k, v in FC.exact_ref(c).items() if k != "bound"}
    B = ops.gft_prepare(t(c["U"], dev))
    W, x, res, dy = (t(c[k], dev) for k in ("W", "x", "res", "dy"))
    gx, gy = Guarded((N, M, Fin), dev), Guarded((N, M, Fout), dev)
    ops.fres_forward(B, W, x, res, "relu", out_xhat=gx.flat, out_y=gy.flat)
    torch.cuda.synchronize()
    xhat, y = gx.verify("xhat"), gy.verify("y")
    assert torch.equal(xhat.double(), ref["xhat"])
    assert torch.equal(y.double(), ref["y"])
    assert bool((y[ref["pre"] <= 0] == 0).all())
    for acc in (False, True):
        gz, gW = Guarded((N, M, Fout), dev), Guarded((M, Fout, Fin), dev)
        gd = Guarded((N, M, Fin), dev, t(c["dx0"], dev) if acc else None)
        ops.fres_backward(B, W, xhat, dy, y, "relu", dx=gd.out, dx_accumulate=acc, out_dz=gz.out,
                          out_dW=gW.out)
        torch.cuda.synchronize()
        dz = gz.verify("dz")
        assert torch.equal(dz.double(), ref["dz"]), acc
        assert bool((dz[y == 0] == 0).all())
        assert torch.equal(gW.verify("dW").double(), ref["dW"]), acc
        assert torch.equal(gd.verify("dx").double(), ref["dx_acc" if acc else "dx"]), acc


# -- 3. training steps against the reference ---------------------------------------------
def _filter_inputs(net, x):
    """(input, residual) of every filter of a network as the GPU ran it."""
    ins, res = [x], [None]
    h, li = net.out[0], 1
    for _ in range(net.o.R):
        ins += [h, net.out[li]]
        res += [None, h]
        h, li = net.out[li + 1], li + 2
    ins.append(h)
    res.append(None)
    return ins, res


def _record(net, calls):
    run_b = net._b

    def recording_b(li, dy, dz, dx, dx_acc, s):  # the schedule's own calls, snapshotted
        before = dx.clone() if (dx is not None and dx_acc) else None
        dy_in = dy.clone()
        run_b(li, dy, dz, dx, dx_acc, s)
        calls.append((li, dy_in, None if dx is None else dx.clone(), before, net.dW[li].clone()))

    net._b = recording_b


def _train_and_check(dev, model, nets, groups, x, labels, R, stacked, tag):
    """Three steps of `model`.  Per step: loss (1e-5 relative); every filter's
    y, dW and dx on the GPU's own inputs (1e-5); every gradient against the
    float64 chain evaluated through the GPU's ReLU masks (1e-5; the unmasked
    error and the mask flips are printed); every parameter against the
    reference's Adam of the GPU's gradient (1e-5: Adam's first steps move a
    weight by ~lr sign(g) whatever |g|, so the update of a float64 chain's
    own gradient is ill-conditioned in the gradient's rounding)."""
    U = f64(model.U)
    xt, lt = t(x, dev), t(labels, dev)
    calls = [[] for _ in nets]
    for net, cl in zip(nets, calls):
        _record(net, cl)
    state = [(np.zeros(tuple(w.shape)), np.zeros(tuple(w.shape))) for w in model.W]
    for step in range(1, 4):
        Wprev = [f64(w) for w in model.W]
        nW = [[f64(w) for w in net.W] for net in nets]
        mW = [f64(w) for w in model.merge_W] if stacked else None
        for cl in calls:
            cl.clear()
        loss = model.train_step(xt, lt)
        torch.cuda.synchronize()
        lr = model.learning_rate(step - 1)
        masks, flips = [], 0
        for i, (net, (a, b)) in enumerate(zip(nets, groups)):
            ins, res = _filter_inputs(net, xt[..., a:b])
            xh, gm = [], []
            for li, (name, fi, fo, act) in enumerate(net.layers):
                ref, xhat = RR.filter_forward(f64(ins[li]), nW[i][li], U,
                                              None if res[li] is None else f64(res[li]), act)
                e = err_of(net.out[li], ref)
                assert e < TOL, (tag, step, name, "y", e)
                xh.append(xhat)
                gm.append(f64(net.out[li]) > 0 if act == "relu" else None)
            assert len(calls[i]) == len(net.layers)
            for li, dy, dx, before, dW in calls[i]:
                name, fi, fo, act = net.layers[li]
                rdx, rdW, _ = RR.filter_backward(f64(dy), None, act, nW[i][li], U, xh[li], gm[li])
                e = err_of(dW, rdW)
                assert e < TOL, (tag, step, name, "dW", e)
                if dx is not None:
                    e = err_of(dx, rdx + (f64(before) if before is not None else 0.0))
                    assert e < TOL, (tag, step, name, "dx", e)
            masks.append(gm)
        # the float64 chain from x alone
        if stacked:
            X, caches = RR.stacked_forward(x, nW, mW, groups, U, R)
            rl, dX = MO.loss_and_grad(X, labels)
            om = [f64(net.out[-1]) > 0 for net in nets]
            plain = RR.stacked_flat(*RR.stacked_backward(dX, caches, nW, mW, U, R))
            masked = RR.stacked_flat(*RR.stacked_backward(dX, caches, nW, mW, U, R, masks, om))
            flips += sum(int(np.count_nonzero((o > 0) != m)) for (o, _), m in zip(caches, om))
            cs = [c for _, cache in caches for c in cache]
        else:
            out, cache = RR.forward(x, nW[0], U, R)
            rl, dout = MO.loss_and_grad(out, labels)
            plain = RR.backward(dout, cache, nW[0], U, R)
            masked = RR.backward(dout, cache, nW[0], U, R, masks[0])
            cs = cache
        flips += sum(int(np.count_nonzero((c[2] > 0) != m))
                     for c, m in zip(cs, [m for gm in masks for m in gm]) if m is not None)
        assert abs(float(loss.item()) - rl) <= 1e-5 * rl, (tag, step, float(loss.item()), rl)
        e_plain = max(err_of(g, r) for g, r in zip(model.dW, plain))
        e_mask = {n: err_of(g, r) for n, g, r in zip(model.names, model.dW, masked)}
        print(f"{tag} step {step}: ReLU mask flips {flips}; end-to-end gradient error "
              f"{e_plain:.2e}, through the GPU's masks {max(e_mask.values()):.2e}")
        assert max(e_mask.values()) < TOL, (tag, step, e_mask, flips)
        new_state = []
        for name, w, w0, g, (m, v) in zip(model.names, model.W, Wprev, model.dW, state):
            rw, m2, v2 = O.adam_step(w0, f64(g), m, v, step, lr=lr)
            new_state.append((m2, v2))
            e = err_of(w, rw)
            assert e < TOL, (tag, step, name, "W", e)
        state = new_state


@pytest.mark.parametrize("graph,N,Fin,F,R", [("A", 5, 3, 16, 2), ("knn130", 3, 10, 24, 1)])
def test_resgnn_fourier_train_steps_vs_reference(dev, graph, N, Fin, F, R):
    from cnn_graph_amd.model import ResGNN
    L, M = laplacian(graph)
    model = ResGNN(L, N=N, Fin=Fin, nfilter=F, K=3, nres_layer_count=R, learning_rate=1e-2,
                   decay_rate=0.95, decay_steps=2, device=dev, seed=5, filter="fourier")
    assert model.plan is None and model.M == M
    assert [tuple(w.shape) for w in model.W] == [(M, F, Fin)] + [(M, F, F)] * (2 * R) + [(M, 2, F)]
    rng = np.random.default_rng(9)
    x = RR.r32(rng.random((N, M, Fin)))
    labels = RR.r32(rng.random((N, M, 2)))
    _train_and_check(dev, model, [model.net], [(0, Fin)], x, labels, R, False, f"ResGNN {graph}")


def test_stacked_resgnn_fourier_train_steps_vs_reference(dev):
    from cnn_graph_amd.model import StackedResGNN
    L, M = laplacian("A")
    N, C, F, R, groups = 3, 5, 8, 1, ((0, 3), (3, 5))
    model = StackedResGNN(L, N=N, C=C, nfilter=F, K=3, nres_layer_count=R, groups=groups,
                          learning_rate=1e-2, decay_rate=0.95, decay_steps=2, device=dev, seed=7,
                          filter="fourier")
    assert model.plan is None
    nl = len(model.nets[0].W)
    assert len(model.names) == 2 * (nl + 1) and model.names[nl] == "final_merge/W_0/weights"
    rng = np.random.default_rng(11)
    x = RR.r32(rng.random((N, M, C)))
    labels = RR.r32(rng.random((N, M, 2)))
    _train_and_check(dev, model, model.nets, list(groups), x, labels, R, True, "StackedResGNN A")


# -- 4. determinism ----------------------------------------------------------------------------
def test_fourier_train_steps_are_bitwise_reproducible(dev):
    from cnn_graph_amd.model import ResGNN
    L, M = laplacian("knn130")
    N, Fin = 3, 10
    rng = np.random.default_rng(21)
    x, labels = t(rng.random((N, M, Fin)), dev), t(rng.random((N, M, 2)), dev)
    runs = []
    for _ in range(2):
        model = ResGNN(L, N=N, Fin=Fin, nfilter=24, K=3, nres_layer_count=1, device=dev, seed=3,
                       filter="fourier")
        losses = [model.train_step(x, labels).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((model.flat.clone(), losses))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert bool(torch.isfinite(runs[0][0]).all())


# -- 5. other implementations ---------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["unfused_ops", "fourier_fused"])
def test_graphconv_fourier_autograd_matches_trainer(dev, fused):
    """GraphConv(filter="fourier").residual_network under autograd -- on
    ops.fourier_conv, and with fourier_fused on ops.fourier_conv_act -- gives the
    trainer's gradients for the trainer's weights."""
    from cnn_graph_amd.graph_conv import GraphConv
    from cnn_graph_amd.model import ResGNN
    L, M = laplacian("A")
    N, Fin, F, R = 4, 2, 8, 1
    model = ResGNN(L, N=N, Fin=Fin, nfilter=F, K=3, nres_layer_count=R, device=dev, seed=1,
                   filter="fourier")
    gc = GraphConv(filter="fourier", device=dev, fourier_fused=fused)
    assert gc.fourier_fused is fused
    rng = np.random.default_rng(2)
    x, labels = t(rng.random((N, M, Fin)), dev), t(rng.random((N, M, 2)), dev)
    gc.residual_network(x, L, F, 3, R, Fout_last=2)
    assert set(gc.weights) == set(model.names)
    for name, w in model.parameters().items():
        with torch.no_grad():
            gc.weights[name].copy_(w)
    out = gc.residual_network(x, L, F, 3, R, Fout_last=2)
    ((out - labels) ** 2).mean().backward()
    model.train_step(x, labels)
    torch.cuda.synchronize()
    for name, g in model.gradients().items():
        e = err_of(gc.weights[name].grad, f64(g))
        assert e < TOL, (name, e)


def test_chebyshev_keyword_is_the_default_model(dev):
    """ResGNN(filter="chebyshev5") is ResGNN(): the same parameters bit for bit
    after two steps."""
    from cnn_graph_amd.model import ResGNN
    L, M = laplacian("A")
    N, Fin = 3, 2
    rng = np.random.default_rng(4)
    x, labels = t(rng.random((N, M, Fin)), dev), t(rng.random((N, M, 2)), dev)
    flats = []
    for kw in ({}, {"filter": "chebyshev5"}):
        model = ResGNN(L, N=N, Fin=Fin, nfilter=8, K=4, nres_layer_count=1, device=dev, seed=6, **kw)
        assert model.plan is not None and model.filter == "chebyshev5"
        for _ in range(2):
            model.train_step(x, labels)
        torch.cuda.synchronize()
        flats.append(model.flat.clone())
    assert torch.equal(flats[0], flats[1])
