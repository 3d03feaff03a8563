"""What tests/test_gpu_fourier_res.py rests on, checked without a GPU: the
float64 restatement's gradients (tests/fourier_resgnn_ref.py) against central
finite differences, the premises of the bitwise cases, and the argument
checks of the cg_fres_* entry points."""
import ctypes

import numpy as np
import pytest

import fourier_res_cases as FC
import fourier_resgnn_ref as RR
from cnn_graph_amd import _lib
from oracle import model_oracle as MO

NEW_SYMBOLS = ["cg_fres_workspace_bytes", "cg_fres_forward", "cg_fres_backward"]

# Central differences of the float64 loss along a unit-scale random direction D
# of one weight, step h = 1e-6: the truncation term is h^2 |f'''| / 6 ~ 1e-13,
# the rounding term eps |loss| / h ~ 2.2e-16 * 0.5 / 1e-6 ~ 1e-10, against
# directional derivatives of 1e-3 .. 1e-1 here: 1e-7 .. 1e-9 relative.  The loss
# is piecewise smooth; with some 300 pre-activations of magnitude ~0.1 a kink
# within +-h |D| of one of them has probability ~1e-3 and the seed is fixed.
# Bar: 1e-6 relative to the largest directional derivative of the case.
FD_STEP = 1e-6
FD_BAR = 1e-6
M, N, FIN, F, R = 12, 2, 3, 4, 1


def _case(seed, Fin):
    rng = np.random.default_rng(seed)
    U = RR.r32(np.linalg.qr(rng.standard_normal((M, M)))[0])
    assert not np.allclose(U, U.T)
    shapes = [(M, F, Fin)] + [(M, F, F)] * (2 * R) + [(M, 2, F)]
    Ws = [rng.uniform(-0.3, 0.3, s) for s in shapes]
    return rng, U, Ws


def _fd_check(f, weights, grads, rng):
    """d f / d (each weight along its own random direction) against grads."""
    got, ref = [], []
    for i, (W, g) in enumerate(zip(weights, grads)):
        D = rng.standard_normal(W.shape)
        plus = [w + FD_STEP * D if j == i else w for j, w in enumerate(weights)]
        minus = [w - FD_STEP * D if j == i else w for j, w in enumerate(weights)]
        got.append((f(plus) - f(minus)) / (2 * FD_STEP))
        ref.append(float(np.sum(g * D)))
    got, ref = np.array(got), np.array(ref)
    scale = np.abs(got).max()
    assert scale > 1e-4
    err = np.abs(got - ref).max() / scale
    print(f"finite differences: directional derivatives {got}, relative error {err:.2e}")
    assert err < FD_BAR, (got, ref)


def test_reference_gradients_match_finite_differences():
    rng, U, Ws = _case(1, FIN)
    x = rng.standard_normal((N, M, FIN))
    labels = rng.standard_normal((N, M, 2))
    out, cache = RR.forward(x, Ws, U, R)
    assert all(np.count_nonzero(c[2] == 0) > 0 for c in cache[:-1])  # the ReLUs clamp
    _, dout = MO.loss_and_grad(out, labels)
    dWs = RR.backward(dout, cache, Ws, U, R)
    _fd_check(lambda w: RR.loss(x, labels, w, U, R), Ws, dWs, rng)


def test_stacked_reference_gradients_match_finite_differences():
    groups = ((0, 2), (2, 3))
    rng, U, W0 = _case(2, 2)
    _, _, W1 = _case(3, 1)
    nets = [W0, W1]
    merge = [rng.uniform(-0.5, 0.5, (M, 2)) for _ in groups]
    x = rng.standard_normal((N, M, 3))
    labels = rng.standard_normal((N, M, 2))
    X, caches = RR.stacked_forward(x, nets, merge, groups, U, R)
    _, dX = MO.loss_and_grad(X, labels)
    dnets, dws = RR.stacked_backward(dX, caches, nets, merge, U, R)

    def f(flat):
        n2, m2 = RR.stacked_unflat(flat, nets)
        return RR.stacked_loss(x, labels, n2, m2, groups, U, R)

    _fd_check(f, RR.stacked_flat(nets, merge), RR.stacked_flat(dnets, dws), rng)


def test_train_step_composes_the_oracles():
    """train_step = forward, loss, backward, cheb_oracle.adam_step per weight."""
    from oracle import cheb_oracle as O
    rng, U, Ws = _case(4, FIN)
    x = rng.standard_normal((N, M, FIN))
    labels = rng.standard_normal((N, M, 2))
    state = [(np.zeros_like(w), np.zeros_like(w)) for w in Ws]
    l, dWs, W2, st2 = RR.train_step(x, labels, Ws, U, R, state, 1, 1e-2)
    assert l == RR.loss(x, labels, Ws, U, R)
    for w, g, w2, (m2, v2) in zip(Ws, dWs, W2, st2):
        rw, rm, rv = O.adam_step(w, g, np.zeros_like(w), np.zeros_like(w), 1, lr=1e-2)
        assert np.array_equal(w2, rw) and np.array_equal(m2, rm) and np.array_equal(v2, rv)


@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("M_,N_,Fin,Fout", FC.SHAPES)
def test_exact_cases_stay_exact_in_float32(M_, N_, Fin, Fout, kind):
    """Every partial sum of the bitwise cases is an integer below 2^24, the
    forward clamps some entries and passes others, dx's accumulation target is
    non-zero, and the perm cases need more than two bf16 terms."""
    c = FC.exact_case(M_, N_, Fin, Fout, kind)
    ref = FC.exact_ref(c)
    if kind == "perm":  # a two-term split keeps 16 significant bits
        for v in (c["x"], ref["yhat"]) if M_ > 1 else ():
            m, _ = np.frexp(np.abs(v))
            assert np.count_nonzero(m * 2.0 ** 16 != np.rint(m * 2.0 ** 16)) > 0
        assert np.abs(np.abs(c["U"]).sum(0) - 1).max() == 0 == np.abs(np.abs(c["U"]).sum(1) - 1).max()
    for k in ("xhat", "yhat", "pre", "y", "dz", "ghat", "dW", "dxhat", "dx", "dx_acc"):
        v = ref[k]
        assert np.array_equal(v, np.rint(v)), k
        assert np.abs(v).max() < 2 ** 24, (k, np.abs(v).max())
    assert ref["bound"] < 2 ** 24
    if M_ * N_ * Fout >= 8:
        assert np.count_nonzero(ref["pre"] <= 0) > 0 and np.count_nonzero(ref["pre"] > 0) > 0
        assert np.count_nonzero(ref["pre"] == 0) > 0
    assert np.all(ref["dz"][ref["y"] == 0] == 0)
    assert np.count_nonzero(c["dx0"]) > 0


def test_header_declares_the_fres_entry_points(built_lib):
    syms = _lib.header_symbols()
    h = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, s
        assert hasattr(h, s), s
    assert h.cg_version() == 301  # an additive extension


def test_fres_workspace_bytes(built_lib):
    h = _lib.lib()
    E = _lib.CG_ERR_ARG
    fb, bb = ctypes.c_size_t(), ctypes.c_size_t()
    assert h.cg_fres_workspace_bytes(3, 100, 10, 32, ctypes.byref(fb), ctypes.byref(bb)) == _lib.CG_OK
    assert fb.value >= 3 * 100 * 32 * 4                       # yhat
    assert bb.value >= 3 * 100 * 32 * 4 + 3 * 100 * 10 * 4    # ghat, dxhat
    assert fb.value % 256 == 0 and bb.value % 256 == 0
    assert h.cg_fres_workspace_bytes(1, 1, 1, 1, ctypes.byref(fb), ctypes.byref(bb)) == _lib.CG_OK
    assert fb.value >= 4 and bb.value >= 8
    for bad in ((0, 100, 10, 32), (3, 0, 10, 32), (3, 100, 0, 32), (3, 100, 10, 0)):
        assert h.cg_fres_workspace_bytes(*bad, ctypes.byref(fb), ctypes.byref(bb)) == E, bad
    assert h.cg_fres_workspace_bytes(3, 100, 10, 32, None, ctypes.byref(bb)) == E
    assert h.cg_fres_workspace_bytes(3, 100, 10, 32, ctypes.byref(fb), None) == E


def test_fres_entry_points_validate(built_lib):
    """Null required pointers, sizes < 1, a short workspace, act relu without
    y and dx_accumulate without dx give CG_ERR_ARG with a message before any
    device work (there is no GPU here, and the pointers are not memory)."""
    h = _lib.lib()
    E = _lib.CG_ERR_ARG
    NONE, RELU = _lib.CG_ACT_NONE, _lib.CG_ACT_RELU
    N_, M_, Fin, Fout = 3, 100, 10, 32
    sz, fb, bb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert h.cg_gft_workspace_bytes(M_, ctypes.byref(sz)) == _lib.CG_OK
    assert h.cg_fres_workspace_bytes(N_, M_, Fin, Fout, ctypes.byref(fb), ctypes.byref(bb)) == _lib.CG_OK
    nb, fw, bw = sz.value, fb.value, bb.value
    B, W, x, res, xhat, y, ws, dy, dz, dx, dW = (ctypes.c_void_p(4096 * k) for k in range(1, 12))

    def fwd(N=N_, M=M_, Fin=Fin, Fout=Fout, B=B, nb=nb, W=W, x=x, res=res, act=RELU, xhat=xhat, y=y,
            ws=ws, n=fw):
        return h.cg_fres_forward(N, M, Fin, Fout, B, nb, W, x, res, act, xhat, y, ws, n, None)

    def bwd(N=N_, M=M_, Fin=Fin, Fout=Fout, B=B, nb=nb, W=W, xhat=xhat, dy=dy, y=y, act=RELU, dz=dz,
            dx=dx, acc=0, dW=dW, ws=ws, n=bw):
        return h.cg_fres_backward(N, M, Fin, Fout, B, nb, W, xhat, dy, y, act, dz, dx, acc, dW, ws, n,
                                  None)

    for k in ("B", "W", "x", "xhat", "y", "ws"):
        assert fwd(**{k: None}) == E, k
    assert h.cg_last_error().decode() != ""
    for k in ("N", "M", "Fin", "Fout"):
        assert fwd(**{k: 0}) == E, k
        assert bwd(**{k: 0}) == E, k
    assert fwd(nb=nb - 1) == E and "basis" in h.cg_last_error().decode()
    assert fwd(n=fw - 1) == E and "workspace" in h.cg_last_error().decode()
    assert fwd(act=_lib.CG_ACT_TANH) == E
    assert fwd(N=1 << 20, Fout=128, n=1 << 40) == E and "2^31" in h.cg_last_error().decode()
    for k in ("B", "W", "xhat", "dy", "dW", "ws"):
        assert bwd(**{k: None}) == E, k
    assert bwd(nb=nb - 1) == E
    assert bwd(n=bw - 1) == E and "workspace" in h.cg_last_error().decode()
    assert bwd(y=None, act=RELU) == E and "needs y" in h.cg_last_error().decode()
    assert bwd(dx=None, acc=1) == E and "dx_accumulate" in h.cg_last_error().decode()
    assert bwd(act=_lib.CG_ACT_TANH) == E
