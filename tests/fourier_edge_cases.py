"""Shapes and seeded inputs of tests/test_gpu_fourier_edges.py, numpy only.

TEST HELPER ONLY.  The GPU tests build their operands here and the CPU
companion (tests/test_fourier_lstm_cpu.py) checks, without a GPU, what those
tests rest on: that the integer operands keep every partial sum exact in
float32, and that the float64 reference of every z = tan(a_z) case stays clear
of the pole.  A seed or shape edited here is therefore checked on both sides.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import scipy.sparse

import fourier_lstm_ref as FR

r32 = FR.r32

GUARD = 256      # floats of NaN on each side of every kernel output
INT_MAX = 8      # integer operands are uniform in [-INT_MAX, INT_MAX]
AZ_MAX = 1.3     # the pole guard of every z = tan(a_z) case: pi/2 = 1.57

# k_gft, (M, N, C): 128 x 128 block tiles, 16-deep k steps, column j = (n, c)
TRANSFORM_SHAPES = [
    (1, 1, 1),      # smallest case
    (7, 2, 3),      # M < 16: a single partly filled k step
    (17, 3, 5),     # the second k step holds one row
    (100, 3, 24),   # C does not divide 128
    (128, 2, 40),   # a full row tile
    (130, 7, 24),   # 168 columns: two column tiles, tile 0 cuts sample 5; row tile 1 holds 2 rows
    (200, 5, 160),  # 800 columns: 7 tiles, the last has 32
    (257, 2, 8),    # three row tiles, the last holds 1 row
]
SPLIT_SHAPE = (130, 3, 5)

# k_fmix, (R, M, Cin, Cout): one wave per (m, 32 x 32 tile), 8-deep k steps
MIX_SHAPES = [(1, 1, 1, 1), (5, 3, 40, 20), (33, 2, 33, 65), (70, 4, 64, 160)]

# cg_flstm_step, (M, N, H): gate mode has ceil(H / 32) column tiles per sample
STEP_SHAPES = [(1, 1, 8), (17, 2, 24), (100, 2, 64), (130, 3, 40), (257, 1, 16)]
GATE_SETS = ["reference", "standard"]

# the layers: a k-NN graph whose M = 130 leaves 2 rows in the second row tile, and
# H = 40: a second unit block with 8 units, C = 40 and 160 in the backward transforms
LAYER_GRAPH = "knn130"
SYNTHETIC_GRAPHS = {LAYER_GRAPH: dict(M=130, k=4, seed=130)}
LAYER_CASE = dict(T=3, N=2, Fin=3, H=40, layers=2, seed=51)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ints(rng, shape):
    return rng.integers(-INT_MAX, INT_MAX + 1, shape).astype(np.float64)


# -- 1. the transform on integers ---------------------------------------------------------
def int_transform_case(M, N, C):
    """(U [M, M], x [N, M, C]): integers of at most 4 significant bits, U not
    symmetric.  The bf16 split of either has no mid or lo term and every partial
    sum of U^T x or U x is an integer of magnitude <= 64 M: exact in float32 in
    any summation order (see exact_bound)."""
    rng = _rng("gft", M, N, C)
    U = _ints(rng, (M, M))
    if M > 1:
        assert not np.array_equal(U, U.T)
    return U, _ints(rng, (N, M, C))


def transform_ref(U, x, inverse):
    """float64 U^T x (analysis) or U x (synthesis) per sample; U[v, m]."""
    return np.einsum("vm,nmc->nvc" if inverse else "vm,nvc->nmc", U, x)


def exact_bound(*operands, depth):
    """The largest magnitude a partial sum of a `depth`-deep contraction of the
    operands can reach (plus one added operand), after checking that they are
    integers in [-INT_MAX, INT_MAX]: it must stay below 2^24."""
    for a in operands:
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= INT_MAX
    return INT_MAX * INT_MAX * depth + INT_MAX


# -- 2. the split ---------------------------------------------------------------------------
def permutation_case():
    """(p, U, x): U[p[m], m] = 1, x = 1e3 randn with full significands."""
    M, N, C = SPLIT_SHAPE
    rng = _rng("perm", M, N, C)
    p = rng.permutation(M)
    U = np.zeros((M, M))
    U[p, np.arange(M)] = 1.0
    return p, U, r32(1e3 * rng.standard_normal((N, M, C)))


def one_hot_case():
    """(U, x, at): U = randn with full significands, x[n, at[n, c], c] = 1."""
    M, N, C = SPLIT_SHAPE
    rng = _rng("onehot", M, N, C)
    U = r32(rng.standard_normal((M, M)))
    at = rng.integers(0, M, (N, C))
    x = np.zeros((N, M, C))
    n, c = np.meshgrid(np.arange(N), np.arange(C), indexing="ij")
    x[n, at, c] = 1.0
    return U, x, at


# -- 3. the per-frequency contraction on integers --------------------------------------------
def int_mix_case(R, M, Cin, Cout):
    """W [M, Cout, Cin], x [R, M, Cin], g and add [R, M, Cout], integers."""
    rng = _rng("fmix", R, M, Cin, Cout)
    return dict(W=_ints(rng, (M, Cout, Cin)), x=_ints(rng, (R, M, Cin)), g=_ints(rng, (R, M, Cout)),
                add=_ints(rng, (R, M, Cout)))


def mix_refs(c):
    fwd = np.einsum("moi,rmi->rmo", c["W"], c["x"])
    return dict(fwd=fwd, fwd_add=fwd + c["add"], t=np.einsum("moi,rmo->rmi", c["W"], c["g"]),
                dw=np.einsum("rmo,rmi->moi", c["g"], c["x"]))


# -- 4. one recurrent step --------------------------------------------------------------------
def step_state_scale(H):
    """Amplitude s of the given h and c.  With Wh uniform in +-0.1 and h uniform
    in +-s the recurrent part U Wh[m] U^T h of a_z has standard deviation
    s sqrt(H) / 30, on top of a_x (up to 0.9) and the bias (up to 0.1): at s = 1
    that is 0.27 for H = 64 and the reference itself crosses the pole guard for
    every H here but 8.  s = 2 / sqrt(H) holds the deviation at 1 / 15 for every
    H, so that 4.5 deviations fit into the 0.3 that the guard leaves."""
    return 2.0 / np.sqrt(H)


def step_case(M, N, H):
    """Inputs of cg_flstm_step, float32 values held as float64: U orthogonal and
    not symmetric (the Q of a Gaussian matrix), ghat_x = U^T a_x with a_x uniform
    in +-0.9, Wh and b uniform in +-0.1, h and c uniform in +-step_state_scale."""
    rng = _rng("step", M, N, H)
    U = r32(np.linalg.qr(rng.standard_normal((M, M)))[0])
    if M > 1:
        assert not np.allclose(U, U.T)
    a_x = rng.uniform(-0.9, 0.9, (N, M, 4 * H))
    s = step_state_scale(H)
    return dict(U=U, ghat_x=r32(transform_ref(U, a_x, inverse=False)),
                h=r32(rng.uniform(-s, s, (N, M, H))), c=r32(rng.uniform(-s, s, (N, M, H))),
                Wh=r32(rng.uniform(-0.1, 0.1, (M, 4 * H, H))), b=r32(rng.uniform(-0.1, 0.1, 4 * H)))


def step_ref(case, gates, given_state):
    """float64: hhat = U^T h, ghat = ghat_x + Wh[m] hhat, a = U ghat + b, the
    gates.  Returns dict(c, h, act [N, M, 4H] as z, i, f, o, hhat or None, az)."""
    U, ghat = case["U"], case["ghat_x"]
    hhat, c = None, 0.0
    if given_state:
        hhat = transform_ref(U, case["h"], inverse=False)
        ghat = ghat + np.einsum("moi,nmi->nmo", case["Wh"], hhat)
        c = case["c"]
    a = transform_ref(U, ghat, inverse=True) + case["b"]
    cn, hn, g = FR.gate_update(a, c, gates)
    return dict(c=cn, h=hn, act=np.concatenate([g[k] for k in "zifo"], axis=-1), hhat=hhat, az=g["az"])


# -- 5. the layers ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic_laplacian(name):
    """(L, M): the normalized Laplacian (float32 CSR, lmax = 2) of the k-NN graph
    of M seeded random points in the unit square."""
    from cnn_graph_amd import graph
    g = SYNTHETIC_GRAPHS[name]
    z = _rng("graph", name, g["seed"]).random((g["M"], 2)).astype(np.float32)
    dist, idx = graph.distance_scipy_spatial(z, k=g["k"])
    A = graph.adjacency(dist.astype(np.float32), idx)
    return scipy.sparse.csr_matrix(graph.laplacian(A, normalized=True), dtype=np.float32), g["M"]


def layer_inputs(given_state, T, N, Fin, H, layers, seed, M):
    """Everything _run_layers draws: per-layer parameters as the cell
    initialises them (Wx, Wh uniform in +-0.1, b glorot-uniform), the sequence,
    the output and c_T cotangents and, if given, the initial states."""
    rng = _rng("layers", given_state, T, N, Fin, H, layers, seed, M)
    lim = np.sqrt(6.0 / (2 * H))
    params = [(r32(rng.uniform(-0.1, 0.1, (M, 4 * H, Fin if li == 0 else H))),
               r32(rng.uniform(-0.1, 0.1, (M, 4 * H, H))), r32(rng.uniform(-lim, lim, 4 * H)))
              for li in range(layers)]
    xs = r32(rng.standard_normal((T, N, M, Fin)))
    G = r32(rng.standard_normal((T, N, M, H)))
    GC = r32(rng.standard_normal((layers, N, M, H)))
    st = [(r32(0.5 * rng.standard_normal((N, M, H))), r32(0.5 * rng.standard_normal((N, M, H))))
          for _ in range(layers)] if given_state else None
    return dict(params=params, xs=xs, G=G, GC=GC, st=st)


def layers_forward(inp, U, gates):
    """The float64 forward of every layer: [(hs, cs, caches)]."""
    x, fw = inp["xs"], []
    for li, P in enumerate(inp["params"]):
        c0, h0 = (None, None) if inp["st"] is None else inp["st"][li]
        fw.append(FR.layer_forward(x, P, U, c0, h0, gates))
        x = fw[-1][0]
    return fw
