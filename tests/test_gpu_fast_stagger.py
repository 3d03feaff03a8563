"""CG_OPT_MFMA_STAGGER: the fast backward's fused-dW groups (cheb_bwd_fast<1, 3>)
run three recurrence steps earlier (steps 2, 8, ... instead of 5, 11, ...) in
two of a SIMD's four waves.  Only WHEN a wave runs a group changes: within a
wave the groups keep their order and operands, so every option value must
give the bits of value 0.

Graphs: those of test_gpu_fast_prologue.py (chord rings with rows of 0..16
nonzeros, and the bench graph at M = 976).  Shapes, for the edges of the
schedule: M = 33 / 257 / 976 / 1024 gives waves with 0, 1, odd and even octet
counts and a ragged last octet; K = 1 .. 25 gives no group in the loop, one,
and groups left for the epilogue, on both sides of each class's first group
step (2 and 5); Fin = 2 (cheb_bwd_fast<2, 3>, which is not staggered: every
value must still agree) up to the fused dW's bound Fin K <= 32.

Bars: basis, y, dx, dW and, after one cg_cheb_backward_adam, W, m, v
np.array_equal to option value 0 on the same inputs; two calls bitwise equal;
dW of every value within 1e-5 (normwise) of the float64 oracle, so a schedule
that is wrong the same way every time cannot pass by equality alone.

Sensitivity (checked on scratch builds of this kernel, not kept): running one
group twice, and starting the epilogue at group K / 6 whatever the wave ran in
the loop, each fail the equality cases below (dW, W, m, v differ)."""
import numpy as np
import pytest

from oracle import cheb_oracle as O
from test_gpu_fast_prologue import graph, inputs, t

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VALUES = (0, 1, 2)
KS = (1, 2, 3, 5, 6, 7, 8, 12, 13, 25)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def shapes(K):
    """(Fin, Fout, N) of one (M, K) case."""
    out = [(1, Fout, N) for Fout in (8, 32) for N in (1, 3)]
    if K <= 16:
        out += [(2, 32, N) for N in (1, 3)]
    return out


def run_once(plan, dev, N, Fin, K, Fout, xd, Wd, dyd):
    """basis, y, dx, dW of forward + backward in the orders layout, then W, m, v
    of one cg_cheb_backward_adam from zero moments (host arrays)."""
    from cnn_graph_amd import ops
    r = ops.ChebRunner(plan, N, Fin, K, Fout, dev, basis_layout="orders")
    assert r.basis_layout == "orders"
    r.basis.fill_(float("nan"))
    y = r.forward(xd, Wd).clone()
    basis = r.basis.clone()
    dx, dW = (a.clone() for a in r.backward(dyd, Wd))
    Wa = Wd.clone()
    m, v = torch.zeros_like(Wa), torch.zeros_like(Wa)
    dxa, dWa = r.backward_adam(dyd, Wa, m, v, 1)
    torch.cuda.synchronize()
    assert torch.equal(dxa, dx) and torch.equal(dWa, dW), "backward_adam's dx / dW differ from backward's"
    names = ("basis", "y", "dx", "dW", "W", "m", "v")
    return dict(zip(names, (a.cpu().numpy() for a in (basis, y, dx, dW, Wa, m, v))))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", [33, 257, 976, 1024])
def test_stagger_bitwise_equal_to_unstaggered(dev, cg_opts, M, K):
    rp, ci, v, fake, plan = graph(M)
    for Fin, Fout, N in shapes(K):
        tag = f"M={M} K={K} Fin={Fin} Fout={Fout} N={N}"
        assert plan.query_path(N, Fin, K, Fout) == "resident", tag
        x, W, dy = inputs(M, fake, N, Fin, K, Fout, 11 * M + K + 100 * Fin + N + Fout)
        xd, Wd, dyd = t(x, dev), t(W, dev), t(dy, dev)
        out = {}
        for val in VALUES:
            cg_opts("mfma_stagger", val)
            out[val] = run_once(plan, dev, N, Fin, K, Fout, xd, Wd, dyd)
        assert not np.array_equal(out[0]["W"], W), tag
        assert np.isfinite(out[0]["dW"]).all() and np.any(out[0]["dW"] != 0), tag
        for val in VALUES[1:]:
            for name, a in out[val].items():
                assert np.array_equal(a, out[0][name]), f"{name}: value {val} differs from 0: {tag}"


@pytest.mark.parametrize("val", VALUES)
def test_stagger_reproducible_and_vs_oracle(dev, cg_opts, val):
    """Config B's graph and filter (K = 25: four groups in the loop), N = 3:
    two calls bitwise equal, and dW against the float64 oracle."""
    M, K, Fin, Fout, N = 976, 25, 1, 32, 3
    rp, ci, v, fake, plan = graph(M)
    x, W, dy = inputs(M, fake, N, Fin, K, Fout, 4242)
    xd, Wd, dyd = t(x, dev), t(W, dev), t(dy, dev)
    cg_opts("mfma_stagger", val)
    a = run_once(plan, dev, N, Fin, K, Fout, xd, Wd, dyd)
    b = run_once(plan, dev, N, Fin, K, Fout, xd, Wd, dyd)
    for name in a:
        assert np.array_equal(a[name], b[name]), f"{name} not reproducible at value {val}"
    ob, _ = O.cheb_forward(x, rp, ci, v, W, K)
    _, odW = O.cheb_backward(dy, ob, W, rp, ci, v, N, M, Fin, K)
    err = O.normwise_err(a["dW"], odW)
    print(f"mfma_stagger={val}: dW normwise error {err:.2e}")
    assert err < 1e-5, f"dW normwise error {err:.3e} at value {val}"
