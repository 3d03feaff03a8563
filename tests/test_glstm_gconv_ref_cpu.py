"""tests/glstm_gconv_ref.py (the float64 inference_glstm_gconv) pinned without a GPU:
its backward against central finite differences of its own forward on a tiny
case, with dropout multipliers and two layers included, and its ``predict``
against a hand computation of the padding and the ``loss * batch_size / size``
weighting (lib/graph_model.py:64-94).  Also the host-side ABI checks of
cg_fres_forward_drop / cg_fres_backward_drop."""
import ctypes
import zlib

import numpy as np
import pytest

import fourier_edge_cases as FE
import glstm_gconv_ref as GR

M, N, T, F, H, C, R, OUT, K = 12, 2, 2, 2, 4, 3, 1, 2, 2
EPS = 1e-5
# A central difference of the float64 loss l: its truncation error is
# EPS^2 |l'''| / 6 (1e-10 relative to derivatives of the gradient's size; 1e-6
# of the largest gradient entry leaves four orders for |l'''| / |l'|), its
# rounding error (l's own few ulps) / EPS, taken as 8 ulps of l -- an ABSOLUTE
# term: the mean over N M out elements makes the gradients ~1e-5, so it is not
# negligible against them.
FD_TOL = 1e-6
FD_ULPS = 8


def _filt(filter, L):
    if filter == "fourier_conv":
        lam, U = np.linalg.eigh(L.toarray().astype(np.float64))
        return ("fourier_conv", U)
    return ("cheby_conv", GR.cheb_lap(L), K)


def _case(filter, gates, layers, keep):
    L = GR.ring_chords_laplacian(M)
    filt = _filt(filter, L)
    rng = np.random.default_rng(zlib.crc32(f"{filter}-{gates}-{layers}".encode()))
    ls, head = GR.seeded_params(rng, filter, M, F, H, C, K, R, OUT, layers)
    xs = GR.r32(0.5 * rng.standard_normal((T, N, M, F)))
    labels = GR.r32(rng.standard_normal((N, M, OUT)))
    mults = None
    if keep < 1.0:
        mults = [GR.drop_mult(100 + li, (T, N, M, H), keep) for li in range(layers - 1)]
        mults.append(GR.drop_mult(100 + layers, (N, M, H), keep, offset=(T - 1) * N * M * H))
    return filt, ls, head, xs, labels, mults


@pytest.mark.parametrize("layers,keep", [(1, 1.0), (2, 0.8)], ids=["one_layer", "two_layers_dropout"])
@pytest.mark.parametrize("gates", ["reference", "standard"])
@pytest.mark.parametrize("filter", ["cheby_conv", "fourier_conv"])
def test_backward_matches_finite_differences(filter, gates, layers, keep):
    filt, ls, head, xs, labels, mults = _case(filter, gates, layers, keep)
    l0, _, dxs, dl, dh, fw = GR.loss_and_grads(xs, labels, ls, head, filt, R, gates, mults)
    # the tan gate is the only place a finite difference can blow up
    az = GR.max_az(fw, gates)
    print(f"max|a_z| = {az:.3f}")
    assert az < FE.AZ_MAX
    if mults is not None:
        assert all((m == 0).any() and (m > 1).any() for m in mults)

    def loss():
        return GR.loss_and_grads(xs, labels, ls, head, filt, R, gates, mults)[0]

    rng = np.random.default_rng(3)
    arrays = [("xs", xs, dxs)]
    for li, (P, G) in enumerate(zip(ls, dl)):
        arrays += [(f"{n}[{li}]", p, g) for n, p, g in zip(("Wx", "Wh", "b"), P, G)]
    arrays += [(f"head[{i}]", w, g) for i, (w, g) in enumerate(zip(head, dh))]
    worst = 0.0
    for name, a, g in arrays:
        assert g.shape == a.shape, name
        scale = np.abs(g).max()
        assert scale > 0, name
        for _ in range(6):
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


def test_predict_padding_and_loss_weighting():
    """size 5, batch 2: batches (0,1), (2,3), (4, zero row).  A per-sample
    'model' keeps the hand computation short: out[n] = 2 * data[n] + 1."""
    rng = np.random.default_rng(0)
    data = rng.standard_normal((5, 3, 2))
    labels = rng.standard_normal((5, 3, 2))
    seen = []

    def fwd(batch):
        assert batch.shape == (2, 3, 2)
        seen.append(batch.copy())
        return 2 * batch + 1

    preds, loss = GR.predict(fwd, data, labels, 2)
    assert preds.shape == (5, 3, 2) and np.array_equal(preds, 2 * data + 1)
    assert len(seen) == 3 and np.array_equal(seen[2][0], data[4]) and not seen[2][1].any()
    sq = (labels - (2 * data + 1)) ** 2
    pad = np.ones((3, 2))  # the padded row: prediction 1 against label 0
    hand = (sq[0:2].mean() + sq[2:4].mean() + (sq[4].sum() + pad.sum()) / (2 * 3 * 2)) * 2 / 5
    assert abs(loss - hand) < 1e-15 * max(1.0, abs(hand))
    assert np.array_equal(GR.predict(fwd, data, None, 2), preds)
    assert GR.evaluate_mse(labels, preds) == np.sum(sq) / sq.size


def test_mask_restatement_matches_the_offset_rule():
    full = GR.keep_bits(77, (3, 40), 0.8)
    assert set(np.unique(full)) == {0.0, 1.0}
    assert np.array_equal(GR.keep_bits(77, (40,), 0.8, offset=80), full[2])
    assert np.array_equal(GR.drop_mult(77, (3, 40), 1.0), np.ones((3, 40)))


# -- the C ABI without a GPU ----------------------------------------------------------------
def test_drop_calls_exported_and_refuse_bad_arguments(built_lib):
    from cnn_graph_amd import _lib
    h = _lib.lib()
    assert h.cg_version() == 301
    E = _lib.CG_ERR_ARG
    one = ctypes.c_void_p(256)  # never dereferenced: every call fails its argument checks
    for keep in (0.0, 1.5, -0.1, float("nan")):
        assert h.cg_fres_forward_drop(1, 8, 4, 4, one, 0, one, one, ctypes.c_float(keep), 1, None, 0,
                                      one, one, one, 1 << 20, None) == E, keep
        assert h.cg_fres_backward_drop(1, 8, 4, 4, one, 0, one, one, one, None, 0,
                                       ctypes.c_float(keep), 1, None, one, one, one, 1 << 20,
                                       None) == E, keep
    # null dx, at keep < 1 and at keep == 1
    for keep in (0.8, 1.0):
        assert h.cg_fres_backward_drop(1, 8, 4, 4, one, 0, one, one, one, None, 0,
                                       ctypes.c_float(keep), 1, None, None, one, one, 1 << 20,
                                       None) == E
    # a null x and a short basis are refused as cg_fres_forward refuses them
    assert h.cg_fres_forward_drop(1, 8, 4, 4, one, 0, one, None, ctypes.c_float(0.8), 1, None, 0,
                                  one, one, one, 1 << 20, None) == E
