"""Geometry-class parity of the streaming path on small graphs: every dispatch
class of cheb_stream.hip's sample-major steps (k_cheb_step, k_cheb_last,
k_clenshaw_step) and of cheb_wide.hip, at the smallest shape that reaches it
(tests/stream_cases.py; the graphs' and the table's premises are checked
without a GPU in tests/test_stream_cases_cpu.py).

Every case first asserts that the plan takes the streaming path and that
ChebPlan.stream_dispatch reports exactly the class the case claims: a case that
lands in another class fails.  Then the project's bars: the basis, pre-filled
with NaN, BITWISE equal to the oracle's fp32 CSR-order recurrence; y, dx, dW
within 1e-5 (normwise) of the float64 oracle; two runs bitwise equal; dx
accumulation within 1e-5 of oracle dx + dx0; a dx-only call without the basis
bitwise equal to the full call's dx.  A wide-column case also runs under
variant 'narrow': basis and y bitwise equal between the layouts (the claim of
cheb_wide.hip's header), dx and dW each within 1e-5 (different dense passes)."""
import numpy as np
import pytest
import scipy.sparse

import stream_cases as S
from oracle import cheb_oracle as O

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


_PLANS = {}


def plan_for(gname, variant):
    if (gname, variant) not in _PLANS:
        from cnn_graph_amd.plan import ChebPlan
        rp, ci, v = S.graph(gname)
        M = len(rp) - 1
        Lt = scipy.sparse.csr_matrix((v, ci, rp), shape=(M, M))
        _PLANS[gname, variant] = ChebPlan(Lt, device=0, path="stream", variant=variant)
    return _PLANS[gname, variant]


def dispatch(c, variant=None):
    plan = plan_for(c["graph"], variant or c["variant"])
    shape = (c["N"], c["Fin"], c["K"], c["Fout"])
    assert plan.query_path(*shape) == "stream", c["name"]
    return plan.stream_dispatch(*shape, layout=c["layout"])


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rows_of(basis, c, M):
    """The basis as [N*M, Fin*K] whatever its layout."""
    if c["layout"] == "planes":   # [K][N*M][Fin] -> column fin*K + k
        return basis.permute(1, 2, 0).reshape(c["N"] * M, c["Fin"] * c["K"])
    return basis


def run(plan, c, dev, xd, Wd, dyd, dx0):
    """Forward and backward twice, the accumulating backward and the dx-only
    backward; returns the first run's (basis rows, y, dx, dW, dx0 + dx)."""
    from cnn_graph_amd import ops
    N, Fin, K, Fout, lay = c["N"], c["Fin"], c["K"], c["Fout"], c["layout"]
    M = plan.M
    runs = []
    for _ in range(2):
        shape = (K, N * M, Fin) if lay == "planes" else (N * M, Fin * K)
        basis = torch.full(shape, float("nan"), device=dev, dtype=torch.float32)
        _, y = ops.cheb_forward(plan, xd, Wd, K, out_basis=basis, layout=lay)
        dx, dW = ops.cheb_backward(plan, dyd, basis, Wd, K, layout=lay)
        torch.cuda.synchronize()
        runs.append([a.cpu().numpy() for a in (rows_of(basis, c, M), y, dx, dW)])
    for n, a, b in zip(("basis", "y", "dx", "dW"), runs[0], runs[1]):
        assert np.array_equal(a, b, equal_nan=True), f"{n} not reproducible: {c['name']}"
    dxa = t(dx0, dev)
    ops.cheb_backward_ex(plan, dyd, None, "none", basis, Wd, K, dx=dxa, dx_accumulate=True,
                         layout=lay)
    dx_only, no_dW = ops.cheb_backward(plan, dyd, None, Wd, K, need_dW=False, layout=lay)
    torch.cuda.synchronize()
    assert no_dW is None
    assert np.array_equal(dx_only.cpu().numpy(), runs[0][2]), \
        f"dx of the call without the basis differs: {c['name']}"
    return runs[0] + [dxa.cpu().numpy()]


def check(out, ref, c, what):
    basis, y, dx, dW, dxa = out
    ob, oy, odx, odW, dx0 = ref
    assert not np.isnan(basis).any(), f"basis not fully written: {c['name']} {what}"
    assert np.array_equal(basis, ob), f"basis not bit-exact: {c['name']} {what}"
    errs = {n: O.normwise_err(a, b) for n, a, b in
            (("y", y, oy), ("dx", dx, odx), ("dW", dW, odW), ("dx_acc", dxa, odx + dx0))}
    print(c["name"], what, {n: f"{e:.2e}" for n, e in errs.items()})
    for n, e in errs.items():
        assert e < TOL, f"{n} normwise error {e:.3e}: {c['name']} {what}"


def group_of(c):
    kind = "narrow" if c["name"].startswith("n_") else \
        "dy" if c["name"].startswith(("w_dy", "w_nody")) else "fwd"
    return f"{c['graph']}-{kind}"


GROUPS = sorted({group_of(c) for c in S.CASES})


@pytest.mark.parametrize("group", GROUPS)
def test_stream_classes_vs_oracle(dev, group):
    cases = [c for c in S.CASES if group_of(c) == group]
    assert cases
    for c in cases:
        d = dispatch(c)
        assert d == c["expect"], f"{c['name']} lands in another dispatch class: " \
            f"{ {k: (d[k], c['expect'][k]) for k in d if d[k] != c['expect'][k]} }"
        rp, ci, v = S.graph(c["graph"])
        M = len(rp) - 1
        N, Fin, K = c["N"], c["Fin"], c["K"]
        x, W, dy, dx0 = S.inputs(c)
        ob, oy = O.cheb_forward(x, rp, ci, v, W, K)
        odx, odW = O.cheb_backward(dy, ob, W, rp, ci, v, N, M, Fin, K)
        ref = (ob, oy, odx, odW, dx0)
        xd, Wd, dyd = t(x, dev), t(W, dev), t(dy, dev)
        out = run(plan_for(c["graph"], c["variant"]), c, dev, xd, Wd, dyd, dx0)
        check(out, ref, c, c["variant"])
        if d["wide"]:
            # the same shape on the sample-major steps
            dn = dispatch(c, "narrow")
            assert dn["wide"] == 0 and dn["vec"] >= 1, c["name"]
            outn = run(plan_for(c["graph"], "narrow"), c, dev, xd, Wd, dyd, dx0)
            check(outn, ref, c, "narrow")
            for n, a, b in zip(("basis", "y"), out[:2], outn[:2]):
                assert np.array_equal(a, b), f"{n} differs between wide and narrow: {c['name']}"


def test_every_dispatch_class_is_hit(dev):
    """What the library reports for the table covers the whole class list, and
    the table holds both sides of the fused last step's K bound as the hook
    gives it for CB = 32, pl = 4."""
    pairs = [(c, dispatch(c)) for c in S.CASES]
    hit = S.classes_hit(pairs)
    for name, names in hit.items():
        print(f"{name}: {', '.join(names) if names else 'NOT HIT'}")
    assert [name for name, names in hit.items() if not names] == []
    plan = plan_for("mixed101", "auto")
    fused = [K for K in range(2, 41) if plan.stream_dispatch(32, 1, K, 8)["fused_last"] == 1]
    assert fused and fused == list(range(2, fused[-1] + 1)) and fused[-1] < 40
    kb = fused[-1]
    at = {K: d for c, d in pairs for K in (c["K"],)
          if (c["N"], c["Fin"], c["graph"], c["variant"]) == (32, 1, "mixed101", "auto")}
    print(f"fused last step at CB=32 pl=4: K <= {kb}")
    assert at[kb]["fused_last"] == 1 and at[kb + 1]["fused_last"] == 0
    assert at[kb + 1]["assemble_tm"] > 0
