"""cg_cheb_workspace_bytes against what the kernels write: the sizes and the
offsets both come from one route (cheb_abi.cpp::cheb_route), and this pins that
they agree.  One case per workspace shape, the smallest of its class in
tests/stream_cases.py: sample-major steps with slots (K >= 3), wide columns
with the fused dy pass, wide columns with dBasis and D planes, the channel-group
kernels in the planes layout (tests/test_gpu_group.py's smaller graph), and a
resident shape (forward bytes 0).

The C ABI is called directly (ops rounds sizes up and reuses a larger buffer).
Exact size: a workspace of exactly the reported bytes with a patterned guard
behind it in the same allocation; CG_OK, the guard unchanged, y / dx / dW
bitwise equal to the same call through ops.  One byte short: forward and
backward refuse with CG_ERR_ARG before any launch, outputs untouched."""
import numpy as np
import pytest
import scipy.sparse

import stream_cases as S
from conftest import case, load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATTERN = 0xA5


def _smallest(pred):
    return min((c for c in S.CASES if pred(c)), key=S.largest_array_bytes)


STEPS = _smallest(lambda c: not c["expect"]["wide"] and c["layout"] == "rows" and c["K"] >= 3)
DYPASS = _smallest(lambda c: c["expect"]["wide"] and c["expect"]["dypass"] and c["K"] >= 2)
NODYPASS = _smallest(lambda c: c["expect"]["wide"] and not c["expect"]["dypass"])
GROUP = dict(name="group_planes", graph="golden_B.npz", N=2, Fin=16, K=5, Fout=32, variant="auto",
             layout="planes")
RESIDENT = dict(STEPS, name="resident", path="auto")
CASES = [STEPS, DYPASS, NODYPASS, GROUP, RESIDENT]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


_BUILT = {}


def _setup(c, dev):
    """(plan, x, W, dy) of a case, on the device; built once."""
    if c["name"] not in _BUILT:
        _BUILT[c["name"]] = _build(c, dev)
    return _BUILT[c["name"]]


def _build(c, dev):
    from cnn_graph_amd.plan import ChebPlan
    N, Fin, K, Fout = (c[k] for k in ("N", "Fin", "K", "Fout"))
    if c["graph"].endswith(".npz"):
        g = case(load_golden(c["graph"]))
        rp, ci, v = g["Lt_rowptr"], g["Lt_col"], g["Lt_val"]
        M = len(rp) - 1
        rng = np.random.default_rng(7)
        x = rng.standard_normal((N, M, Fin)).astype(np.float32)
        W = (rng.standard_normal((Fin * K, Fout)) * 0.1).astype(np.float32)
        dy = rng.standard_normal((N, M, Fout)).astype(np.float32)
    else:
        rp, ci, v = S.graph(c["graph"])
        M = len(rp) - 1
        x, W, dy, _ = S.inputs(c)
    Lt = scipy.sparse.csr_matrix((v, ci, rp), shape=(M, M))
    plan = ChebPlan(Lt, device=0, path=c.get("path", "stream"), variant=c["variant"])
    return (plan,) + tuple(torch.from_numpy(a).to(dev) for a in (x, W, dy))


def _check_class(c, plan):
    """The case reaches the workspace shape it stands for."""
    shape = (c["N"], c["Fin"], c["K"], c["Fout"])
    need_f, need_b = plan.workspace_bytes(*shape)
    if c is RESIDENT:
        assert plan.query_path(*shape) == "resident" and need_f == 0 and need_b > 0
        return
    d = plan.stream_dispatch(*shape, layout=c["layout"])
    if c is GROUP:
        assert d["group_fwd"] == 1 and d["group_bwd"] in (1, 2), d
    else:
        assert d == c["expect"], d
    assert need_f > 0 and need_b > 0


def _guarded(need, dev):
    guard = max(256, min(need, 1 << 20))
    return torch.full((need + guard,), PATTERN, dtype=torch.uint8, device=dev)


def _outputs(c, M, dev, fill):
    N, Fin, K, Fout = (c[k] for k in ("N", "Fin", "K", "Fout"))
    bshape = (K, N * M, Fin) if c["layout"] == "planes" else (N * M, Fin * K)
    shapes = dict(basis=bshape, y=(N, M, Fout), dx=(N, M, Fin), dW=(Fin * K, Fout))
    return {k: torch.full(s, fill, dtype=torch.float32, device=dev) for k, s in shapes.items()}


def _forward(c, plan, x, W, o, ws, ws_bytes):
    from cnn_graph_amd import _lib
    return _lib.lib().cg_cheb_forward_layout(
        plan.handle, c["N"], c["Fin"], c["K"], c["Fout"], x.data_ptr(), W.data_ptr(), None,
        _lib.CG_ACT_NONE, _lib.BASIS_LAYOUTS[c["layout"]], o["basis"].data_ptr(), o["y"].data_ptr(),
        ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)


def _backward(c, plan, dy, W, o, ws, ws_bytes):
    from cnn_graph_amd import _lib
    return _lib.lib().cg_cheb_backward_layout(
        plan.handle, c["N"], c["Fin"], c["K"], c["Fout"], dy.data_ptr(), None, _lib.CG_ACT_NONE,
        _lib.BASIS_LAYOUTS[c["layout"]], o["basis"].data_ptr(), W.data_ptr(), o["dx"].data_ptr(), 0,
        o["dW"].data_ptr(), None, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_exact_workspace_with_guard(dev, c):
    from cnn_graph_amd import _lib, ops
    plan, x, W, dy = _setup(c, dev)
    _check_class(c, plan)
    K, lay = c["K"], c["layout"]
    need_f, need_b = plan.workspace_bytes(c["N"], c["Fin"], K, c["Fout"])
    print(c["name"], "forward bytes", need_f, "backward bytes", need_b)
    rbasis, ry = ops.cheb_forward(plan, x, W, K, layout=lay)
    rdx, rdW = ops.cheb_backward(plan, dy, rbasis, W, K, layout=lay)
    o = _outputs(c, plan.M, dev, float("nan"))
    wf, wb = _guarded(need_f, dev), _guarded(need_b, dev)
    assert _forward(c, plan, x, W, o, wf, need_f) == _lib.CG_OK, _lib.lib().cg_last_error()
    assert _backward(c, plan, dy, W, o, wb, need_b) == _lib.CG_OK, _lib.lib().cg_last_error()
    torch.cuda.synchronize()
    assert bool((wf[need_f:] == PATTERN).all()), "the forward wrote past the reported size"
    assert bool((wb[need_b:] == PATTERN).all()), "the backward wrote past the reported size"
    for name, ref in (("basis", rbasis), ("y", ry), ("dx", rdx), ("dW", rdW)):
        assert torch.equal(o[name].reshape(ref.shape), ref), f"{name} differs from the ops call"


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_one_byte_short_is_refused(dev, c):
    from cnn_graph_amd import _lib, ops
    plan, x, W, dy = _setup(c, dev)
    _check_class(c, plan)
    need_f, need_b = plan.workspace_bytes(c["N"], c["Fin"], c["K"], c["Fout"])
    rbasis, _ = ops.cheb_forward(plan, x, W, c["K"], layout=c["layout"])
    o = _outputs(c, plan.M, dev, 3.0)
    ws = torch.full((max(need_f, need_b),), PATTERN, dtype=torch.uint8, device=dev)
    if need_f > 0:
        assert _forward(c, plan, x, W, o, ws, need_f - 1) == _lib.CG_ERR_ARG
        assert b"forward workspace too small" in _lib.lib().cg_last_error()
        assert bool((o["basis"] == 3.0).all()), "basis was written by a refused call"
    o["basis"].copy_(rbasis.reshape(o["basis"].shape))  # the backward's input, not an output
    assert _backward(c, plan, dy, W, o, ws, need_b - 1) == _lib.CG_ERR_ARG
    assert b"backward workspace too small" in _lib.lib().cg_last_error()
    torch.cuda.synchronize()
    assert bool((ws == PATTERN).all())
    for name in ("y", "dx", "dW"):
        assert bool((o[name] == 3.0).all()), f"{name} was written by a refused call"
