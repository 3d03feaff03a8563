"""tests/glstm_period_ref.py (the float64 closeness / period / trend networks) pinned
without a GPU: the column rule of its input split on a hand-written x, and its
backward against central finite differences of its own forward on a tiny case --
both merges, both filters, unequal T, two layers with dropout multipliers.  The
finite-difference bound is tests/test_glstm_gconv_ref_cpu.py's, reasoned there."""
import zlib

import numpy as np
import pytest

import fourier_edge_cases as FE
import glstm_gconv_ref as GR
import glstm_period_ref as PR
from test_glstm_gconv_ref_cpu import EPS, FD_TOL, FD_ULPS, _filt

M, N, F, H, R, OUT, K = 12, 2, 2, 4, 1, 2, 2
T = (2, 1, 3)


def test_split_column_rule():
    """Column F S_b + f T_b + t is step t, feature f of branch b (lib/gconv_lstm.py
    :472-479: x_arr[0:2 Tc], x_arr[2 Tc:2 (Tc + Tp)], ...; :486-487: reshape to
    [N, M, F, T_b], unstack axis 3).  x holds its own column number."""
    C = F * sum(T)
    x = np.broadcast_to(np.arange(C, dtype=np.float64), (N, M, C)).copy()
    x += 100.0 * np.arange(N)[:, None, None] + 1000.0 * np.arange(M)[None, :, None]
    parts = PR.split(x, T, F)
    assert [p.shape for p in parts] == [(t, N, M, F) for t in T]
    s = 0
    for b, tb in enumerate(T):
        for t in range(tb):
            for f in range(F):
                assert np.array_equal(parts[b][t, :, :, f], x[:, :, F * s + f * tb + t]), (b, t, f)
        s += tb
    # by hand for T = (2, 1, 3), F = 2: closeness reads columns 0..3 as (f0t0, f0t1, f1t0, f1t1),
    # period 4..5 as (f0t0, f1t0), trend 6..11 as (f0t0, f0t1, f0t2, f1t0, f1t1, f1t2)
    assert parts[0][1, 0, 0].tolist() == [1.0, 3.0]
    assert parts[1][0, 0, 0].tolist() == [4.0, 5.0]
    assert parts[2][2, 0, 0].tolist() == [8.0, 11.0]
    # unsplit is its transpose, and columns no branch reads get no gradient
    wide = np.concatenate([x, x[:, :, :3]], axis=2)
    assert all(np.array_equal(a, b) for a, b in zip(PR.split(wide, T, F), parts))
    back = PR.unsplit(parts, T, F, C + 3)
    assert np.array_equal(back[:, :, :C], x) and not back[:, :, C:].any()


def _case(filter, mode, layers, keep):
    L = GR.ring_chords_laplacian(M)
    filt = _filt(filter, L)
    rng = np.random.default_rng(zlib.crc32(f"period-{filter}-{mode}-{layers}".encode()))
    B = len(T)
    branches, merge = PR.seeded_params(rng, filter, mode, M, F, H, K, R, OUT, B, layers)
    x = GR.r32(0.5 * rng.standard_normal((N, M, F * sum(T))))
    labels = GR.r32(rng.standard_normal((N, M, OUT)))
    mults = None
    if keep < 1.0:
        mults = []
        for b, tb in enumerate(T):
            m = [GR.drop_mult(100 + 10 * b + li, (tb, N, M, H), keep) for li in range(layers - 1)]
            m.append(GR.drop_mult(100 + 10 * b + layers, (N, M, H), keep, offset=(tb - 1) * N * M * H))
            mults.append(m)
    return filt, branches, merge, x, labels, mults


@pytest.mark.parametrize("layers,keep", [(1, 1.0), (2, 0.8)], ids=["one_layer", "two_layers_dropout"])
@pytest.mark.parametrize("mode", ["weights", "concat"])
@pytest.mark.parametrize("filter", ["cheby_conv", "fourier_conv"])
def test_backward_matches_finite_differences(filter, mode, layers, keep):
    filt, branches, merge, x, labels, mults = _case(filter, mode, layers, keep)
    args = (labels, T, F, branches, merge, filt, mode, R, "reference", mults)
    l0, _, dx, dbr, dm, fw = PR.loss_and_grads(x, *args)
    az = PR.max_az(fw, "reference")
    print(f"max|a_z| = {az:.3f}")
    assert az < FE.AZ_MAX
    if mults is not None:
        assert all((m == 0).any() and (m > 1).any() for ms in mults for m in ms)

    def loss():
        return PR.loss_and_grads(x, *args)[0]

    names = ["x"] + [f"param[{i}]" for i in range(len(PR.flat_params(branches, merge, mode)))]
    arrays = [x] + PR.flat_params(branches, merge, mode)
    grads = [dx] + PR.flat_params(dbr, dm, mode)
    assert len(arrays) == len(grads) == 1 + len(T) * (3 * layers + (2 if mode == "weights" else 0)) + \
        (2 * R + 2 if mode == "concat" else 0)
    # a one-step branch never runs its h-conv (zero state): its Wh has no gradient at all
    per = 3 * layers + (2 if mode == "weights" else 0)
    no_grad = {f"param[{b * per + 3 * li + 1}]" for b, tb in enumerate(T) if tb == 1 for li in range(layers)}
    rng = np.random.default_rng(3)
    worst = 0.0
    for name, a, g in zip(names, arrays, grads):
        assert g.shape == a.shape, name
        scale = np.abs(g).max()
        assert (scale == 0) == (name in no_grad), name
        for _ in range(4):
            idx = tuple(int(rng.integers(0, s)) for s in a.shape)
            keep_v = a[idx]
            a[idx] = keep_v + EPS
            lp = loss()
            a[idx] = keep_v - EPS
            lm = loss()
            a[idx] = keep_v
            fd = (lp - lm) / (2 * EPS)
            err = abs(fd - g[idx])
            bound = FD_TOL * scale + FD_ULPS * np.spacing(l0) / EPS
            worst = max(worst, err / bound)
            assert err < bound, (name, idx, fd, g[idx], bound)
    print(f"worst finite-difference error / its bound = {worst:.2e}")
    assert loss() == l0  # the inputs were restored


def test_train_step_keeps_the_variable_order():
    filt, branches, merge, x, labels, _ = _case("cheby_conv", "weights", 1, 1.0)
    flat0 = PR.flat_params(branches, merge, "weights")
    state = [(np.zeros_like(p), np.zeros_like(p)) for p in flat0]
    l, nb, nm, state2, ema = PR.train_step(x, labels, T, F, branches, merge, filt, "weights", R,
                                           "reference", None, state, 1, 1e-2, (0.0, 0.0, 0))
    flat1 = PR.flat_params(nb, nm, "weights")
    assert [p.shape for p in flat1] == [p.shape for p in flat0] and l > 0 and ema[1] > 0
    # Adam's first step moves every entry with a non-zero gradient by ~lr
    # (but the one-step branch's Wh, flat index 5 + 1: no h-conv ran, no gradient)
    for i, (p0, p1) in enumerate(zip(flat0, flat1)):
        d = np.abs(p1 - p0)
        assert d.max() <= 1e-2 * (1 + 1e-6) and (d.max() > 0.5e-2 or i == 6), i
