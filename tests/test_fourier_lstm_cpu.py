"""gconv-LSTM with the Fourier filter, the parts that need no GPU: the float64
restatement (tests/fourier_lstm_ref.py) pinned to itself by finite differences
and to a vertex-domain filter, the premises of the tile-edge GPU tests' inputs
(tests/fourier_edge_cases.py), and the new C-ABI entry points' argument checks."""
import ctypes

import numpy as np
import pytest

import fourier_edge_cases as FE
import fourier_lstm_ref as FR
from cnn_graph_amd import _lib

NEW_SYMBOLS = ("cg_gft_workspace_bytes", "cg_gft_prepare", "cg_gft", "cg_fourier_mix",
               "cg_flstm_supported", "cg_flstm_workspace_bytes", "cg_flstm_step")


def _setup(seed=0, M=12, N=2, H=3, T=3, Fin=2):
    rng = np.random.default_rng(seed)
    A = rng.random((M, M)) * (rng.random((M, M)) < 0.4)
    A = np.triu(A, 1)
    A = A + A.T
    L = np.diag(A.sum(1)) - A
    _, U = np.linalg.eigh(L)
    xs = rng.standard_normal((T, N, M, Fin))
    params = [rng.uniform(-0.1, 0.1, (M, 4 * H, Fin)), rng.uniform(-0.1, 0.1, (M, 4 * H, H)),
              rng.uniform(-0.5, 0.5, 4 * H)]
    c0, h0 = 0.5 * rng.standard_normal((N, M, H)), 0.5 * rng.standard_normal((N, M, H))
    gh, gc, ghT = (rng.standard_normal(s) for s in ((T, N, M, H), (N, M, H), (N, M, H)))
    return U, xs, params, c0, h0, gh, gc, ghT


def _loss(xs, params, U, c0, h0, gh, gc, ghT, gates):
    hs, cs, caches = FR.layer_forward(xs, params, U, c0, h0, gates)
    return float((hs * gh).sum() + (cs[-1] * gc).sum() + (hs[-1] * ghT).sum()), caches


def test_restatement_backward_matches_finite_differences():
    """Cell backward (T = 1 inside) and layer BPTT (T = 3) against central
    differences of the restatement's own forward, for x, c0, h0, Wx, Wh, b."""
    for gates in ("reference", "standard"):
        U, xs, params, c0, h0, gh, gc, ghT = _setup()
        _, caches = _loss(xs, params, U, c0, h0, gh, gc, ghT, gates)
        assert FR.max_az(caches) < 1.3
        grads = FR.layer_backward(gh, gc, caches, params, U, gates, dhT=ghT)
        dxs, dc0, dh0, dWx, dWh, db = grads
        rng = np.random.default_rng(1)
        eps = 1e-6
        for name, arr, g in (("xs", xs, dxs), ("c0", c0, dc0), ("h0", h0, dh0), ("Wx", params[0], dWx),
                             ("Wh", params[1], dWh), ("b", params[2], db)):
            assert g.shape == arr.shape
            for _ in range(6):
                idx = tuple(rng.integers(0, s) for s in arr.shape)
                old = arr[idx]
                arr[idx] = old + eps
                lp, _ = _loss(xs, params, U, c0, h0, gh, gc, ghT, gates)
                arr[idx] = old - eps
                lm, _ = _loss(xs, params, U, c0, h0, gh, gc, ghT, gates)
                arr[idx] = old
                fd = (lp - lm) / (2 * eps)
                assert abs(fd - g[idx]) <= 1e-6 * max(1.0, abs(fd)), (gates, name, idx, fd, g[idx])


def test_restatement_equals_a_vertex_domain_filter():
    """With every W[m] = g_m W0 the spectral cell is the vertex-domain filter
    U diag(g) U^T applied to x and h, then W0 on the features."""
    U, xs, params, c0, h0, *_ = _setup(seed=3)
    rng = np.random.default_rng(4)
    M, H = U.shape[0], c0.shape[-1]
    g = rng.standard_normal(M)
    Wx0, Wh0 = params[0][0].copy(), params[1][0].copy()
    Wx = g[:, None, None] * Wx0
    Wh = g[:, None, None] * Wh0
    b = params[2]
    cn, hn, cache = FR.cell_forward(xs[0], c0, h0, Wx, Wh, b, U)
    G = U @ np.diag(g) @ U.T
    a = np.einsum("vw,nwi,oi->nvo", G, xs[0], Wx0) + np.einsum("vw,nwi,oi->nvo", G, h0, Wh0) + b
    z, i, f, o = np.tan(a[..., :H]), 1 / (1 + np.exp(-a[..., H:2 * H])), \
        1 / (1 + np.exp(-a[..., 2 * H:3 * H])), np.tanh(a[..., 3 * H:])
    c_ref = f * c0 + i * z
    assert np.abs(cn - c_ref).max() < 1e-12 * max(1.0, np.abs(c_ref).max())
    assert np.abs(hn - o * np.tanh(c_ref)).max() < 1e-12


# -- what tests/test_gpu_fourier_edges.py rests on ---------------------------------------
@pytest.mark.parametrize("M,N,C", FE.TRANSFORM_SHAPES)
def test_edge_transform_operands_are_exact_in_float32(M, N, C):
    """Integers of at most 4 bits (no mid or lo term in the bf16 split), every
    partial sum below 2^24, and a U that tells U from U^T."""
    U, x = FE.int_transform_case(M, N, C)
    assert U.shape == (M, M) and x.shape == (N, M, C)
    assert FE.exact_bound(U, x, depth=M) < 2 ** 24
    assert 64 * M < 2 ** 24
    if M > 1:
        assert not np.array_equal(FE.transform_ref(U, x, False), FE.transform_ref(U, x, True))


@pytest.mark.parametrize("R,M,Cin,Cout", FE.MIX_SHAPES)
def test_edge_mix_operands_are_exact_in_float32(R, M, Cin, Cout):
    c = FE.int_mix_case(R, M, Cin, Cout)
    assert FE.exact_bound(*c.values(), depth=max(R, Cin, Cout)) < 2 ** 24
    assert 64 * max(M, R, Cin, Cout) < 2 ** 24
    for k, ref in FE.mix_refs(c).items():  # and the float64 einsums themselves are exact integers
        assert np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() < 2 ** 24, k


def test_edge_split_operands():
    """The permutation and one-hot cases: one non-zero product per output, and
    operands with full significands (a lo term to lose)."""
    p, U, x = FE.permutation_case()
    assert np.array_equal(U.sum(0), np.ones(len(p))) and np.array_equal(U.sum(1), np.ones(len(p)))
    assert not np.array_equal(p, np.argsort(p))  # p is not its own inverse: U and U^T differ
    assert np.array_equal(FE.transform_ref(U, x, False), x[:, p, :])
    U2, x2, at = FE.one_hot_case()
    assert np.array_equal(x2.sum(1), np.ones(at.shape)) and np.array_equal(np.unique(x2), [0.0, 1.0])
    for a in (x, U2):  # nearly every value needs the third bf16 term
        bits = np.asarray(a, np.float32).view(np.uint32)
        assert np.mean((bits & 0xff) != 0) > 0.9


@pytest.mark.parametrize("given_state", [False, True])
@pytest.mark.parametrize("M,N,H", FE.STEP_SHAPES)
def test_edge_step_inputs_clear_the_pole(M, N, H, given_state):
    c = FE.step_case(M, N, H)
    assert np.abs(c["U"].T @ c["U"] - np.eye(M)).max() < 1e-6  # orthogonal, as float32 values
    ref = FE.step_ref(c, "reference", given_state)
    assert np.abs(ref["az"]).max() < FE.AZ_MAX
    assert all(np.isfinite(v).all() for v in ref.values() if v is not None)


@pytest.mark.parametrize("given_state", [False, True])
def test_edge_layer_inputs_clear_the_pole(given_state):
    from cnn_graph_amd import graph
    L, M = FE.synthetic_laplacian(FE.LAYER_GRAPH)
    assert L.shape == (M, M) and M == 130 and abs(L - L.T).max() < 1e-6
    U = FR.r32(graph.fourier(L)[1])  # what filter.fourier_basis puts on the device
    inp = FE.layer_inputs(given_state, M=M, **FE.LAYER_CASE)
    for hs, cs, caches in FE.layers_forward(inp, U, "reference"):
        assert FR.max_az(caches) < FE.AZ_MAX


def test_header_declares_the_fourier_lstm_entry_points(built_lib):
    syms = _lib.header_symbols()
    h = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, s
        assert hasattr(h, s), s
    assert h.cg_version() == 301  # an additive extension


def test_fourier_lstm_entry_points_validate(built_lib):
    """Null pointers, bad shapes and short workspaces give CG_ERR_ARG with a
    message, before any device work (no GPU here)."""
    h = _lib.lib()
    E = _lib.CG_ERR_ARG
    sz = ctypes.c_size_t()
    ok = ctypes.c_int32()
    p, q, r, s = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3, 4))
    assert h.cg_gft_workspace_bytes(100, ctypes.byref(sz)) == _lib.CG_OK
    need = sz.value
    assert need >= 2 * 100 * 100 * (3 * 2 + 4)
    assert h.cg_gft_workspace_bytes(0, ctypes.byref(sz)) == E
    assert h.cg_gft_workspace_bytes(100, None) == E
    # prepare
    assert h.cg_gft_prepare(100, None, p, need, None) == E
    assert h.cg_gft_prepare(100, q, None, need, None) == E
    assert h.cg_gft_prepare(100, q, p, need - 1, None) == E
    assert "basis" in h.cg_last_error().decode()
    # transform
    assert h.cg_gft(0, 3, 100, 2, None, need, q, r, None) == E
    assert h.cg_gft(0, 3, 100, 2, p, need - 1, q, r, None) == E
    assert h.cg_gft(0, 3, 100, 2, p, need, None, r, None) == E
    assert h.cg_gft(0, 3, 100, 2, p, need, q, None, None) == E
    assert h.cg_gft(0, 3, 100, 2, p, need, q, q, None) == E
    assert h.cg_gft(0, 0, 100, 2, p, need, q, r, None) == E
    assert h.cg_gft(0, 3, 100, 0, p, need, q, r, None) == E
    assert h.cg_gft(0, 1 << 20, 100, 128, p, need, q, r, None) == E
    assert "2^31" in h.cg_last_error().decode()
    # per-frequency contraction
    assert h.cg_fourier_mix(3, 4, 100, 2, 32, p, q, r, None, s, None) == E
    assert "form" in h.cg_last_error().decode()
    assert h.cg_fourier_mix(0, 4, 100, 2, 32, None, q, None, None, s, None) == E
    assert h.cg_fourier_mix(0, 4, 100, 2, 32, p, None, None, None, s, None) == E
    assert h.cg_fourier_mix(0, 4, 100, 2, 32, p, q, None, None, None, None) == E
    assert h.cg_fourier_mix(1, 4, 100, 2, 32, p, None, None, None, s, None) == E
    assert h.cg_fourier_mix(2, 4, 100, 2, 32, None, q, None, None, s, None) == E
    assert h.cg_fourier_mix(2, 4, 100, 2, 32, None, q, r, r, s, None) == E
    assert h.cg_fourier_mix(0, 0, 100, 2, 32, p, q, None, None, s, None) == E
    assert h.cg_fourier_mix(0, 4, 100, 0, 32, p, q, None, None, s, None) == E
    # support query and the step
    assert h.cg_flstm_supported(100, 32, 2, ctypes.byref(ok)) == _lib.CG_OK and ok.value == 1
    assert h.cg_flstm_supported(100, 8, 1, ctypes.byref(ok)) == _lib.CG_OK and ok.value == 1
    assert h.cg_flstm_supported(100, 12, 2, ctypes.byref(ok)) == _lib.CG_OK and ok.value == 0
    assert h.cg_flstm_supported(100, 32, 2, None) == E
    assert h.cg_flstm_supported(0, 32, 2, ctypes.byref(ok)) == E
    assert h.cg_flstm_workspace_bytes(3, 100, 32, ctypes.byref(sz)) == _lib.CG_OK
    ws = sz.value
    assert ws >= 3 * 100 * 128 * 4
    assert h.cg_flstm_workspace_bytes(3, 100, 32, None) == E
    big = (ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20),
           ctypes.c_void_p(4 << 20), ctypes.c_void_p(5 << 20), ctypes.c_void_p(6 << 20),
           ctypes.c_void_p(7 << 20), ctypes.c_void_p(8 << 20), ctypes.c_void_p(9 << 20))
    hp, cp, gx, Wh, b, co, ho, act, hh = big
    w = ctypes.c_void_p(10 << 20)

    def step(N=3, M=100, H=32, gates=0, basis=p, nb=need, hp=hp, cp=cp, gx=gx, Wh=Wh, b=b, co=co,
             ho=ho, act=act, hh=hh, w=w, wsn=ws):
        return h.cg_flstm_step(N, M, H, gates, basis, nb, hp, cp, gx, Wh, b, co, ho, act, hh, w, wsn,
                               None)
    assert step(basis=None) == E
    assert step(nb=need - 1) == E
    assert step(gx=None) == E
    assert step(co=None) == E
    assert step(ho=None) == E
    assert step(Wh=None) == E
    assert step(hh=None) == E
    assert step(w=None) == E
    assert step(wsn=ws - 1) == E
    assert "workspace" in h.cg_last_error().decode()
    assert step(H=12) == E
    assert step(gates=7) == E
    assert "gate" in h.cg_last_error().decode()
    assert step(N=0) == E
