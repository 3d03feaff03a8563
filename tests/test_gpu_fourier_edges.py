"""The Fourier gconv-LSTM kernels (csrc/fourier_lstm.hip: k_gft<X3>, its prepare
kernels, the gate epilogue, k_fmix) where the tiles do not fit and where a
broken bf16 split would show: row tiles with tails beyond the first, fewer
than 16 rows, a second unit block in gate mode, column tiles that cut a
sample, k_fmix tiles with tails on every side.

Integer and one-hot operands make the transform and the contraction exact, so
they are compared BITWISE with float64; the recurrent step and the layers keep
the project's bar, normwise error < 1e-5 against the float64 restatement.
Every kernel output lies in a NaN-filled buffer between two NaN guard bands:
an unwritten element or a store next to the payload fails the test.  Inputs
and shapes: tests/fourier_edge_cases.py (their premises are checked without a
GPU in tests/test_fourier_lstm_cpu.py)."""
import numpy as np
import pytest

import fourier_edge_cases as FE
import test_gpu_fourier_lstm as TF
from test_gpu_fourier_lstm import check, t

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = FE.GUARD
STATES = pytest.mark.parametrize("given_state", [False, True], ids=["zero_state", "given_state"])


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


class Guarded:
    """A kernel output of n floats inside a NaN-filled buffer of n + 2 G."""

    def __init__(self, shape, dev, fill=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * G,), float("nan"), device=dev, dtype=torch.float32)
        self.flat = self.buf[G:G + self.n]  # what the op gets: contiguous, n elements
        self.out = self.flat.view(*shape)
        if fill is not None:
            self.out.copy_(fill)

    def verify(self, name):
        """Guards untouched, payload fully written (the inputs are NaN-free)."""
        assert bool(torch.isnan(self.buf[:G]).all()), f"{name}: store before the output"
        assert bool(torch.isnan(self.buf[G + self.n:]).all()), f"{name}: store past the output"
        assert not bool(torch.isnan(self.flat).any()), f"{name}: unwritten output element"
        return self.out


def t64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def gft_guarded(B, x, inverse, name):
    from cnn_graph_amd import ops
    o = Guarded(x.shape, x.device)
    ops.gft(B, x, inverse=inverse, out=o.flat)
    torch.cuda.synchronize()
    return o.verify(name)


def both_transforms(dev, U, x):
    """(analysis, synthesis) of x on the prepared U, each through a guarded buffer."""
    from cnn_graph_amd import ops
    B = ops.gft_prepare(t(U, dev))
    xt = t(x, dev)
    return gft_guarded(B, xt, False, "analysis"), gft_guarded(B, xt, True, "synthesis")


# -- 1. the transform, exact on integers ----------------------------------------------------
@pytest.mark.parametrize("M,N,C", FE.TRANSFORM_SHAPES)
def test_gft_is_exact_on_integers(dev, x3, M, N, C):
    U, x = FE.int_transform_case(M, N, C)
    ana, syn = both_transforms(dev, U, x)
    assert torch.equal(ana.double(), t64(FE.transform_ref(U, x, inverse=False), dev))
    assert torch.equal(syn.double(), t64(FE.transform_ref(U, x, inverse=True), dev))


# -- 2. the transform, the split is exact -----------------------------------------------------
def test_gft_permutation_returns_x_bitwise(dev, x3):
    """U a permutation matrix: every output is one product 1 * x plus zeros, so
    the moving operand's on-the-fly split must give x back to the last bit."""
    p, U, x = FE.permutation_case()
    ana, syn = both_transforms(dev, U, x)
    xt = t(x, dev)
    pt = torch.from_numpy(p).to(dev)
    assert torch.equal(ana, xt[:, pt, :])       # (U^T x)[m] = x[p[m]]
    assert torch.equal(syn[:, pt, :], xt)       # (U x)[p[m]] = x[m]


def test_gft_one_hot_returns_u_bitwise(dev, x3):
    """x one-hot per (n, c): every output column is a row (analysis) or a column
    (synthesis) of U, so the prepared three-term split and its fragment order
    must give U back to the last bit."""
    U, x, at = FE.one_hot_case()
    ana, syn = both_transforms(dev, U, x)
    Ut = t(U, dev)
    for n in range(at.shape[0]):
        for c in range(at.shape[1]):
            assert torch.equal(ana[n, :, c], Ut[at[n, c], :]), (n, c)
            assert torch.equal(syn[n, :, c], Ut[:, at[n, c]]), (n, c)


# -- 3. the per-frequency contraction, exact on integers -----------------------------------------
@pytest.mark.parametrize("R,M,Cin,Cout", FE.MIX_SHAPES)
def test_fourier_mix_is_exact_on_integers(dev, R, M, Cin, Cout):
    from cnn_graph_amd import ops
    c = FE.int_mix_case(R, M, Cin, Cout)
    ref = {k: t64(v, dev) for k, v in FE.mix_refs(c).items()}
    W, x, g, add = (t(c[k], dev) for k in ("W", "x", "g", "add"))
    runs = []

    def run(name, key, shape, fill=None, **kw):
        o = Guarded(shape, dev, fill)
        if fill is not None:
            kw["add"] = o.out  # in place: out is the same tensor as add
        ops.fourier_mix(out=o.out, **kw)
        runs.append((name, key, o))

    run("fwd", "fwd", (R, M, Cout), form="fwd", W=W, x=x)
    run("fwd + add", "fwd_add", (R, M, Cout), form="fwd", W=W, x=x, add=add)
    run("fwd in place", "fwd_add", (R, M, Cout), fill=add, form="fwd", W=W, x=x)
    run("t", "t", (R, M, Cin), form="t", W=W, g=g)
    run("dw", "dw", (M, Cout, Cin), form="dw", x=x, g=g)
    torch.cuda.synchronize()
    for name, key, o in runs:
        assert torch.equal(o.verify(name).double(), ref[key]), name


# -- 4. one recurrent step at tile edges ----------------------------------------------------------
@STATES
@pytest.mark.parametrize("gates", FE.GATE_SETS)
@pytest.mark.parametrize("M,N,H", FE.STEP_SHAPES)
def test_flstm_step_at_tile_edges(dev, x3, M, N, H, gates, given_state):
    from cnn_graph_amd import ops
    c = FE.step_case(M, N, H)
    ref = FE.step_ref(c, gates, given_state)
    if gates == "reference":
        assert np.abs(ref["az"]).max() < FE.AZ_MAX
    B = ops.gft_prepare(t(c["U"], dev))
    hp, cp = (t(c["h"], dev), t(c["c"], dev)) if given_state else (None, None)
    o = {k: Guarded((N, M, w * H), dev) for k, w in (("c", 1), ("h", 1), ("act", 4), ("hhat", 1))}
    ret = ops.flstm_step(B, hp, cp, t(c["ghat_x"], dev), t(c["Wh"], dev), t(c["b"], dev), gates,
                         out_c=o["c"].flat, out_h=o["h"].flat, out_act=o["act"].flat,
                         out_hhat=o["hhat"].flat)
    torch.cuda.synchronize()
    if not given_state:  # no analysis ran: hhat is not an output of this call
        assert ret[3] is None and bool(torch.isnan(o.pop("hhat").buf).all())
    got = {k: v.verify(k) for k, v in o.items()}
    check("c'", got["c"], ref["c"])
    check("h'", got["h"], ref["h"])
    for q, name in enumerate("zifo"):
        check(f"act {name}", got["act"][..., q * H:(q + 1) * H], ref["act"][..., q * H:(q + 1) * H])
    if given_state:
        check("hhat", got["hhat"], ref["hhat"])


# -- 5. layers through autograd at an edge shape ---------------------------------------------------
@STATES
@pytest.mark.parametrize("gates", FE.GATE_SETS)
def test_two_layers_on_the_knn_graph(dev, x3, gates, given_state):
    """M = 130, H = 40: row tails in a second row tile, a second unit block in
    the gate epilogue, C = 40 and 160 in the backward transforms, Cin = 40 in
    k_fmix's "t" and "dw" forms."""
    _, M = TF.laplacian(FE.LAYER_GRAPH)
    TF._run_layers(dev, FE.LAYER_GRAPH, given_state=given_state, gates=gates,
                   inputs=FE.layer_inputs(given_state, M=M, **FE.LAYER_CASE), **FE.LAYER_CASE)
