"""Shapes and seeded inputs of tests/test_gpu_fourier_res.py, numpy only.

TEST HELPER ONLY (the contract of fourier_edge_cases.py): the GPU tests build
their operands here and tests/test_fourier_resgnn_ref_cpu.py checks, without a
GPU, that the integer cases keep every partial sum exact in float32 and that
they clamp what they claim to clamp.
"""
from __future__ import annotations

import zlib

import numpy as np

import fourier_resgnn_ref as RR

# cg_fres_*, (M, N, Fin, Fout): one vertex; C = 10 and 32 on one row tile, 96
# columns; two row tiles with 2 rows in the second and Fout = 2 (4 columns);
# three row tiles, C = 5 and 40
SHAPES = [(1, 1, 1, 1), (100, 3, 10, 32), (130, 2, 32, 2), (257, 1, 5, 40)]
# the operand sets of the bitwise test
#   perm   U a signed permutation, x integers of up to 17 significant bits, W
#          in [-2, 2]: the synthesis' moving operand yhat has up to 23
#          significant bits, which only the full three-term bf16 split carries
#   small  U the sum of three signed permutations with coefficients +-1, +-2
#          (a small-integer matrix that mixes vertices), every operand in [-8, 8]
KINDS = ["perm", "small"]
X_WIDE = (1 << 17) - 1


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ints(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, shape).astype(np.float64)


def _signed_perm(rng, M, coef=(1,)):
    U = np.zeros((M, M))
    U[rng.permutation(M), np.arange(M)] = rng.choice(coef, M) * rng.choice([-1.0, 1.0], M)
    return U


def parity_case(M, N, Fin, Fout):
    """float32 values held as float64: U orthogonal and not symmetric, W as the
    model draws it (0.1 scale), unit-scale x / residual / dy / dx0."""
    rng = _rng("fres", M, N, Fin, Fout)
    U = RR.r32(np.linalg.qr(rng.standard_normal((M, M)))[0])
    if M > 1:
        assert not np.allclose(U, U.T)
    return dict(U=U, W=RR.r32(0.1 * rng.standard_normal((M, Fout, Fin))),
                x=RR.r32(rng.standard_normal((N, M, Fin))),
                res=RR.r32(rng.standard_normal((N, M, Fout))),
                dy=RR.r32(rng.standard_normal((N, M, Fout))),
                dx0=RR.r32(rng.standard_normal((N, M, Fin))))


def exact_case(M, N, Fin, Fout, kind):
    """Integer operands.  The residual is a small integer, except at every
    fifth entry, where it is -(U yhat): there the pre-activation is exactly 0,
    so y == 0 and the gradient must be dropped."""
    rng = _rng("fres-int", M, N, Fin, Fout, kind)
    if kind == "perm":
        U = _signed_perm(rng, M)
        x, W = _ints(rng, (N, M, Fin), X_WIDE), _ints(rng, (M, Fout, Fin), 2)
    else:
        U = sum(_signed_perm(rng, M, (1, 2)) for _ in range(3))
        x, W = _ints(rng, (N, M, Fin)), _ints(rng, (M, Fout, Fin))
    c = dict(U=U, W=W, x=x, res=_ints(rng, (N, M, Fout)), dy=_ints(rng, (N, M, Fout)),
             dx0=_ints(rng, (N, M, Fin)))
    c["dx0"][c["dx0"] == 0] = 3.0
    pre0 = RR.filter_forward(x, W, U)[0]
    flat = c["res"].reshape(-1)
    flat[::5] = -pre0.reshape(-1)[::5]
    return c


def exact_ref(c):
    """float64 values of every tensor the device path forms (spectra sample-
    major) and ``bound``: the largest magnitude any partial sum can reach."""
    U, W, x, res, dy = (c[k] for k in ("U", "W", "x", "res", "dy"))
    xhat = np.einsum("vm,nvi->nmi", U, x)
    yhat = np.einsum("moi,nmi->nmo", W, xhat)
    pre = np.einsum("vm,nmo->nvo", U, yhat) + res
    y = np.maximum(pre, 0.0)
    dz = dy * (y > 0)
    ghat = np.einsum("vm,nvo->nmo", U, dz)
    dW = np.einsum("nmo,nmi->moi", ghat, xhat)
    dxhat = np.einsum("moi,nmo->nmi", W, ghat)
    dx = np.einsum("vm,nmi->nvi", U, dxhat)
    aU, aW = np.abs(U), np.abs(W)
    b_xhat = np.einsum("vm,nvi->nmi", aU, np.abs(x))
    b_yhat = np.einsum("moi,nmi->nmo", aW, b_xhat)
    b_pre = np.einsum("vm,nmo->nvo", aU, b_yhat) + np.abs(res)
    b_ghat = np.einsum("vm,nvo->nmo", aU, np.abs(dy))
    b_dW = np.einsum("nmo,nmi->moi", b_ghat, b_xhat)
    b_dxhat = np.einsum("moi,nmo->nmi", aW, b_ghat)
    b_dx = np.einsum("vm,nmi->nvi", aU, b_dxhat) + np.abs(c["dx0"])
    bound = max(float(b.max()) for b in (b_xhat, b_yhat, b_pre, b_ghat, b_dW, b_dxhat, b_dx))
    return dict(xhat=xhat, yhat=yhat, pre=pre, y=y, dz=dz, ghat=ghat, dW=dW, dxhat=dxhat, dx=dx,
                dx_acc=dx + c["dx0"], bound=bound)


def parity_ref(c, act, residual):
    """float64 reference of one filter call pair on parity_case's operands."""
    res = c["res"] if residual else None
    y, xhat = RR.filter_forward(c["x"], c["W"], c["U"], res, act)
    return y, xhat
