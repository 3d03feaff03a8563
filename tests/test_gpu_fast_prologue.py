"""The fast resident kernels' prologue, row images and pair contraction on
small graphs that exercise every shape of them: idle lanes and the zero
record, row images of 0, 1, 8, 9 and 16 slots, the forward's pair contraction
(for Fin = 1, Fout <= 32 with a compile-time ring slot, s mod 3 at each of the
three sites of the 6-unrolled loop, running offsets and a final pair
dispatched on ((K-1)>>1) % 3; otherwise multiplied out), and the backward over
L~^T with the same row images.

Graphs (all on the fast path: M <= 1024, rows <= 16 nonzeros, symmetric
pattern so L~^T has the same row lengths): a ring with seeded chords whose
vertices have exactly 16, 9 and 8 nonzeros (enough of each at M >= 976 to fill
a wave), ordinary vertices with 3..7, diagonal-only vertices (1) and empty
("fake") vertices (0); and the bench graph of tests/golden/golden_B.npz.

Bars: basis BITWISE equal to the oracle's fp32 CSR-order recurrence; y, dx, dW
within 1e-5 (normwise) of the float64 oracle; two runs bitwise equal;
cg_cheb_backward_adam bitwise equal to backward + cg_adam_update."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

from conftest import case, load_golden
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
LENGTHS = (0, 1, 8, 9, 16)
LDS_BYTES = 160 * 1024   # per CU on gfx950


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def chord_ring(M, seed):
    """Symmetric-pattern CSR (rowptr, col, val) on M vertices with rows of
    exactly 16, 9 and 8 nonzeros (nh of each), 3..7 (ring + diagonal + chord
    ends), 1 (diagonal only) and 0 (fake); |row sums| <= 1, so the recurrence
    stays bounded over K = 25 steps."""
    rng = np.random.default_rng(seed)
    nh = max(2, M // 16)              # M = 1024: 64 of each = one full wave
    nfake = max(2, M // 32)
    ndiag = max(2, M // 32)
    nbody = M - nfake - ndiag
    perm = rng.permutation(M)          # the classes are scattered over the vertex numbers
    body, diag = perm[:nbody], perm[nbody:nbody + ndiag]
    nbr = {int(v): {int(v)} for v in np.concatenate([body, diag])}
    for i in range(nbody):
        a, b = int(body[i]), int(body[(i + 1) % nbody])
        nbr[a].add(b)
        nbr[b].add(a)
    hubs = [(int(body[i]), t) for i, t in zip(range(3 * nh), [16] * nh + [9] * nh + [8] * nh)]
    plain = [int(v) for v in body[3 * nh:]]
    assert plain, "no ordinary vertices left"
    for hv, target in hubs:
        order = rng.permutation(len(plain))
        for j in order:
            if len(nbr[hv]) == target:
                break
            p = plain[j]
            if p not in nbr[hv] and len(nbr[p]) < 7:
                nbr[hv].add(p)
                nbr[p].add(hv)
        assert len(nbr[hv]) == target, "chord_ring: not enough ordinary vertices"
    rowptr, col = [0], []
    for v in range(M):
        col.extend(sorted(nbr.get(v, ())))
        rowptr.append(len(col))
    rowptr, col = np.asarray(rowptr, np.int32), np.asarray(col, np.int32)
    val = rng.standard_normal(len(col)).astype(np.float32)
    A = scipy.sparse.csr_matrix((np.abs(val), col, rowptr), shape=(M, M))
    norm = max(float(A.sum(axis=1).max()), float(A.sum(axis=0).max()))
    val = (val / np.float32(norm)).astype(np.float32)
    fake = np.nonzero(np.diff(rowptr) == 0)[0]
    return rowptr, col, val, fake


_GRAPHS = {}


def graph(M):
    """(rowptr, col, val, fake rows, plan) of the test graph with M vertices (cached)."""
    if M not in _GRAPHS:
        from cnn_graph_amd.plan import ChebPlan
        if M == 976:
            c = case(load_golden("golden_B.npz"))
            assert c["M"] == 976
            rp, ci, v = c["Lt_rowptr"], c["Lt_col"], c["Lt_val"]
            fake = np.nonzero(np.diff(rp) == 0)[0]
        else:
            rp, ci, v, fake = chord_ring(M, 1000 + M)
            lens = set(np.diff(rp).tolist())
            assert set(LENGTHS) <= lens, f"row lengths {sorted(lens)}"
            assert len(fake) >= 2
        assert M <= 1024 and np.diff(rp).max() <= 16           # fast path: L~ ...
        assert np.bincount(ci, minlength=M).max() <= 16         # ... and L~^T
        Lt = scipy.sparse.csr_matrix((v, ci, rp), shape=(M, M))
        _GRAPHS[M] = (rp, ci, v, fake, ChebPlan(Lt, device=0, path="resident"))
    return _GRAPHS[M]


def inputs(M, fake, N, Fin, K, Fout, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((N, M, Fin), dtype=np.float32)
    x[:, fake, :] = 0
    W = (rng.standard_normal((Fin * K, Fout)) * 0.1).astype(np.float32)
    dy = rng.standard_normal((N, M, Fout)).astype(np.float32)
    return x, W, dy


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("K", [1, 2, 3, 6, 7, 25])
@pytest.mark.parametrize("M", [33, 100, 976, 1024])
def test_fast_kernels_vs_oracle(dev, M, K):
    """Fin in {1, 2} x Fout in {8, 32} x N in {1, 3} x both basis layouts."""
    from cnn_graph_amd import _lib, ops
    rp, ci, v, fake, plan = graph(M)
    for Fin in (1, 2):
        for N in (1, 3):
            for Fout in (8, 32):
                tag = f"M={M} K={K} Fin={Fin} N={N} Fout={Fout}"
                if 4 * M * Fin * K > LDS_BYTES:
                    # M >= 976 with Fin * K = 50: one sample's basis alone is past the
                    # CU's LDS and past the orders layout's 32 columns, so there is no
                    # resident kernel for the shape: the plan must refuse it
                    with pytest.raises(_lib.CGError):
                        plan.query_path(N, Fin, K, Fout)
                    continue
                assert plan.query_path(N, Fin, K, Fout) == "resident", tag
                x, W, dy = inputs(M, fake, N, Fin, K, Fout, 7 * M + K + 100 * Fin + N + Fout)
                ob, oy = O.cheb_forward(x, rp, ci, v, W, K)        # fp32 basis, float64 y
                ob32, _ = O.cheb_forward(x, rp, ci, v, W, K, dtype=np.float32)
                assert ob.dtype == np.float32 and np.array_equal(ob, ob32)
                odx, odW = O.cheb_backward(dy, ob, W, rp, ci, v, N, M, Fin, K)
                xd, Wd, dyd = t(x, dev), t(W, dev), t(dy, dev)
                for layout in ("orders", "rows"):
                    if layout == "orders" and Fin * K > 32:
                        # no fused dW past 32 basis columns, so no orders layout: the
                        # library must say so, not run something else
                        assert plan.basis_elems(N, Fin, K, Fout, "orders") is None, tag
                        continue
                    r = ops.ChebRunner(plan, N, Fin, K, Fout, dev, basis_layout=layout)
                    runs = []
                    for _ in range(2):
                        r.basis.fill_(float("nan"))
                        y = r.forward(xd, Wd).clone()
                        basis = r.basis_rows().clone()
                        dx, dW = r.backward(dyd, Wd)
                        torch.cuda.synchronize()
                        runs.append([a.cpu().numpy() for a in (basis, y, dx, dW)])
                    where = f"{tag} {layout}"
                    basis, y, dx, dW = runs[0]
                    assert np.array_equal(basis, ob), f"basis not bit-exact: {where}"
                    errs = {n: O.normwise_err(a, b) for n, a, b in
                            (("y", y, oy), ("dx", dx, odx), ("dW", dW, odW))}
                    print(where, {n: f"{e:.2e}" for n, e in errs.items()})
                    for n, e in errs.items():
                        assert e < TOL, f"{n} normwise error {e:.3e}: {where}"
                    for n, a, b in zip(("basis", "y", "dx", "dW"), runs[0], runs[1]):
                        assert np.array_equal(a, b), f"{n} not reproducible: {where}"


def test_fused_adam_bitwise_on_bench_graph(dev):
    """cg_cheb_backward_adam at M = 976, K = 25 (the bench's kernels and layout):
    dx, dW, W, m, v bitwise equal to cg_cheb_backward + cg_adam_update."""
    from cnn_graph_amd import _lib, ops
    M, K, Fin, Fout, N = 976, 25, 1, 32, 3
    rp, ci, v, fake, plan = graph(M)
    x, W, dy = inputs(M, fake, N, Fin, K, Fout, 5)
    xd, dyd = t(x, dev), t(dy, dev)
    ra = ops.ChebRunner(plan, N, Fin, K, Fout, dev, basis_layout="orders")
    rb = ops.ChebRunner(plan, N, Fin, K, Fout, dev, basis_layout="orders")
    Wa, Wb = t(W, dev), t(W, dev)
    ma, va, mb, vb = (torch.zeros_like(Wa) for _ in range(4))
    ra.forward(xd, Wa)
    rb.forward(xd, Wb)
    dxa, dWa = ra.backward_adam(dyd, Wa, ma, va, 1)
    dxb, dWb = rb.backward(dyd, Wb)
    _lib.check("cg_adam_update", _lib.lib().cg_adam_update(
        Wb.data_ptr(), dWb.data_ptr(), mb.data_ptr(), vb.data_ptr(), Wb.numel(),
        ctypes.c_float(1e-3), ctypes.c_float(0.9), ctypes.c_float(0.999), ctypes.c_float(1e-8), 1,
        ctypes.c_float(1.0), None))
    torch.cuda.synchronize()
    for name, a, b in (("dx", dxa, dxb), ("dW", dWa, dWb), ("W", Wa, Wb), ("m", ma, mb), ("v", va, vb)):
        assert torch.equal(a, b), f"{name}: fused Adam differs from backward + cg_adam_update"
    assert not torch.equal(Wa, t(W, dev))
