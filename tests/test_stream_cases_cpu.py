"""The graph builders and the case table of tests/stream_cases.py keep their
promises (no GPU): row-length sets, the skew inequality both ways, empty rows,
row and column sums, a transpose that differs for the directed graph, a bounded
fp32 recurrence through K = 40, small shapes, and a table whose claimed
dispatch classes cover the whole list."""
import numpy as np
import pytest
import scipy.sparse

import stream_cases as S
from oracle import cheb_oracle as O


def _csr(name):
    rp, ci, v = S.graph(name)
    M = len(rp) - 1
    return rp, ci, v, M, scipy.sparse.csr_matrix((v, ci, rp), shape=(M, M))


@pytest.mark.parametrize("name", sorted(S.GRAPHS))
def test_builder_promises(name):
    rp, ci, v, M, A = _csr(name)
    assert M == S.GRAPHS[name][1] and rp.dtype == np.int32 and ci.dtype == np.int32
    assert v.dtype == np.float32 and np.isfinite(v).all() and (v != 0).all()
    for r in range(M):                                    # canonical CSR
        assert (np.diff(ci[rp[r]:rp[r + 1]]) > 0).all(), r
    lens = np.diff(rp)
    assert set(S.LENGTHS) <= set(lens.tolist()), sorted(set(lens.tolist()))
    assert len(S.empty_rows(rp)) >= 1
    assert float(abs(A).sum(axis=1).max()) <= 1.0 and float(abs(A).sum(axis=0).max()) <= 1.0
    AT = A.T.tocsr()
    AT.sort_indices()
    tlens = np.diff(AT.indptr)
    kind = S.GRAPHS[name][0]
    if kind is S.hub_rows:
        assert lens.max() >= S.HUB_MIN and lens.max() > S.skew_bound(rp)
        # the degree-sorted order (stable, longest first) differs from the
        # natural order at both ends
        order = sorted(range(M), key=lambda r: -int(lens[r]))
        assert order[0] != 0 and order[-1] != M - 1
        assert lens[order[0]] >= S.HUB_MIN and lens[order[-1]] == 0
    else:
        assert lens.max() <= S.skew_bound(rp)
    if kind is S.directed_rows:
        assert not np.array_equal(AT.indptr, rp), "L~^T has the row lengths of L~"
        assert sorted(tlens.tolist()) != sorted(lens.tolist())
        assert set(S.LENGTHS) <= set(tlens.tolist())
    else:
        assert np.array_equal(AT.indptr, rp) and np.array_equal(AT.indices, ci)


@pytest.mark.parametrize("name", sorted(S.GRAPHS))
def test_oracle_fp32_basis_at_k40(name):
    """cheb_forward(dtype=float32) returns the default call's fp32 basis, finite
    and of moderate size through K = 40."""
    rp, ci, v, M, _ = _csr(name)
    rng = np.random.default_rng(40)
    N, Fin, K, Fout = 2, 2, 40, 3
    x = rng.random((N, M, Fin), dtype=np.float32)
    x[:, S.empty_rows(rp), :] = 0
    W = (rng.standard_normal((Fin * K, Fout)) * 0.1).astype(np.float32)
    b64, y64 = O.cheb_forward(x, rp, ci, v, W, K)
    b32, y32 = O.cheb_forward(x, rp, ci, v, W, K, dtype=np.float32)
    assert b64.dtype == np.float32 and np.array_equal(b64, b32)
    assert np.isfinite(b64).all() and np.isfinite(y64).all() and y32.dtype == np.float32
    assert np.abs(b64).max() < 1e3, "the recurrence is not bounded on this graph"
    assert (b64.reshape(N, M, Fin * K)[:, S.empty_rows(rp), :] == 0).all()


def test_case_table_is_small_and_well_formed():
    assert len({c["name"] for c in S.CASES}) == len(S.CASES)
    for c in S.CASES:
        assert c["graph"] in S.GRAPHS and c["variant"] in ("auto", "narrow", "steps"), c["name"]
        assert c["layout"] in ("rows", "planes") and tuple(c["expect"]) == S.FIELDS, c["name"]
        assert S.largest_array_bytes(c) < S.MAX_ARRAY_BYTES, c["name"]
        x, W, dy, dx0 = S.inputs(c)
        M = S.GRAPHS[c["graph"]][1]
        assert x.shape == (c["N"], M, c["Fin"]) and W.shape == (c["Fin"] * c["K"], c["Fout"])
        assert dy.shape == (c["N"], M, c["Fout"]) and dx0.shape == x.shape
        assert (x[:, S.empty_rows(S.graph(c["graph"])[0]), :] == 0).all()
        if c["layout"] == "planes":
            assert c["Fin"] % 16 == 0 and c["K"] >= 2 and c["expect"]["wide"] == 0
        if c["variant"] == "narrow":
            assert c["expect"]["wide"] == 0


def test_claimed_classes_cover_the_list():
    """Every class of stream_cases.CLASSES is claimed by at least one case (the
    GPU test repeats this on what the library reports)."""
    hit = S.classes_hit((c, c["expect"]) for c in S.CASES)
    assert [name for name, cases in hit.items() if not cases] == []
    assert all(any(pred(c, c["expect"]) for pred in S.CLASSES.values()) for c in S.CASES)
