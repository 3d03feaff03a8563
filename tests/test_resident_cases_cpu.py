"""The case tables of tests/resident_cases.py cover what they claim (no GPU):
every row-length class under each kernel's own tiling, on L~ for the forwards
and on L~^T for the backwards; empty, idle and partly filled tiles; rows at
both parities of their CSR start; directed graphs whose L~^T is another matrix
in another order; the k_xbasis bound; the tan gate's distance from its pole;
small arrays."""
import numpy as np
import pytest

import fourier_edge_cases as FE
import resident_cases as RC
import stream_cases as SC
from cnn_graph_amd import graph as G
from oracle import lstm_oracle as LO


def _fwd(cases):
    return set().union(*(RC.tile_classes(RC.graph(c["graph"])[0]) for c in cases))


def _bwd(cases, fn):
    return set().union(*(fn(RC.tgraph(c["graph"])[0]) for c in cases))


def test_row_class_ladder():
    got = [RC.row_class(n) for n in range(0, 15)]
    assert got == [4] * 5 + [6] * 2 + [8] * 2 + [10] * 2 + [12] * 2 + [RC.DYN] * 2
    assert RC.row_class(67) == RC.DYN


@pytest.mark.parametrize("table", ["seq", "hstep", "layer"])
def test_forward_tilings_meet_every_class(table):
    """k_lstm_seq's 32-row tiles of lorder (k_lstm_hstep walks the natural
    order with a dynamic loop: the same graphs give it every row length)."""
    assert _fwd(RC.LSTM_TABLES[table]) == RC.ALL_CLASSES


def test_bstep_pairing_meets_every_class():
    assert _bwd(RC.BSTEP_CASES, RC.bstep_classes) == RC.ALL_CLASSES
    assert _bwd(RC.LAYER_CASES, RC.bstep_classes) == RC.ALL_CLASSES
    # the pairs of 16-row tiles are 32 consecutive entries of tlorder
    for name in RC.GRAPHS:
        trp = RC.tgraph(name)[0]
        assert RC.bstep_classes(trp) == RC.tile_classes(trp), name


def test_group_kernels_meet_every_class():
    by = lambda **kw: [c for c in RC.GROUP_CASES if all(c[k] == v for k, v in kw.items())]  # noqa: E731
    assert _fwd(by(fwd="grp16")) == RC.ALL_CLASSES   # k_grp16_fwd, and k_grp_fwd<1> with grp16 off
    assert _fwd(by(fwd="grp")) == RC.ALL_CLASSES                       # k_grp_fwd<2>
    assert _bwd(by(bwd=1), RC.tile_classes) == RC.ALL_CLASSES          # k_grp_clen, per tile
    assert _bwd(by(bwd=2), RC.clen_dy_classes) == RC.ALL_CLASSES       # k_grp_clen_dy, tiles w, w + 8
    for fout in (2, 32, 64):                                           # each instantiation of it
        assert _bwd(by(bwd=2, Fout=fout), RC.clen_dy_classes) == RC.ALL_CLASSES, fout
    # k_grp_clen's packed columns serve classes 4..12, lds_row_spmm_w the dynamic one
    assert RC.DYN in _bwd(by(bwd=1), RC.tile_classes)
    # the far pairing is not the neighbour pairing: it must be restated on its own
    trp = RC.tgraph("dir1001")[0]
    assert sorted(RC.clen_dy_classes(trp)) != sorted(RC.tile_classes(trp)[::2])


def test_group_table_shapes():
    assert {c["Fin"] for c in RC.GROUP_CASES} == {8, 16, 24}
    assert {c["K"] for c in RC.GROUP_CASES} == {2, 5, 7}
    assert {c["Fout"] for c in RC.GROUP_CASES if c["bwd"] == 2} == {2, 32, 64}
    assert {c["Fout"] for c in RC.GROUP_CASES if c["bwd"] == 1} == {20}
    assert {c["graph"] for c in RC.GROUP_CASES} == {"dir101", "hub301", "dir1001"}
    for c in RC.GROUP_CASES:
        # cheb_abi.cpp::check_layout: the planes layout (the group forward's) needs Fin % 16 == 0;
        # cheb_group.hip::launch_grp_fwd: g16 = ... Fin % kGQ16 == 0 && Fout <= 32
        assert c["fwd"] == (None if c["Fin"] % 16 else "grp16" if c["Fout"] <= 32 else "grp"), c["name"]
        assert c["layout"] == ("planes" if c["fwd"] else "rows"), c["name"]
        assert c["bwd"] == (2 if c["Fout"] in (2, 32, 64) else 1), c["name"]
        assert c["N"] in (1, 3) or (c["N"] == 8 and c["graph"] == "dir101"), c["name"]
    acc = [c for c in RC.GROUP_CASES if c["accumulate"]]
    assert len(acc) == 1 and acc[0]["graph"] == "dir101"


def test_lstm_table_shapes():
    for name, table in RC.LSTM_TABLES.items():
        for c in table:
            assert c["T"] == 3 and c["gates"] in ("reference", "standard"), c["name"]
            assert c["N"] in (1, 3) or (c["N"] == 8 and c["graph"] == "dir101"), c["name"]
            assert 1 <= c["K"] <= 4 and c["covers"], c["name"]
    assert {c["K"] for c in RC.SEQ_CASES} == {1, 2, 3, 4}
    assert {c["Fin"] for c in RC.SEQ_CASES} == {1, 2, 5, 8}
    assert {(c["gates"], c["state"]) for c in RC.SEQ_CASES} == \
        {(g, s) for g in ("reference", "standard") for s in (False, True)}
    assert any(c["N"] == 8 for c in RC.SEQ_CASES)
    assert {c["N"] for c in RC.HSTEP_CASES} == {3, 8}
    assert {(c["graph"], c["K"], c["gates"]) for c in RC.BSTEP_CASES} == \
        {(g, K, s) for g in ("dir101", "hub301", "dir1001") for K in (1, 2, 3, 4)
         for s in ("reference", "standard")}
    assert any(c["N"] == 8 for c in RC.BSTEP_CASES)
    assert {c["graph"] for c in RC.LAYER_CASES} == {"dir101", "hub301"}
    assert all(c["N"] == 3 and c["K"] == 3 for c in RC.LAYER_CASES)
    assert {(c["Fin"], c["K"]) for c in RC.XBASIS_CASES} >= {(1, 2), (1, 3), (2, 2), (2, 4), (1, 4), (2, 3)}


def test_tile_and_row_shapes():
    used = {c["graph"] for t in RC.LSTM_TABLES.values() for c in t} | {c["graph"] for c in RC.GROUP_CASES}
    assert used == set(RC.GRAPHS)
    fill = {g: RC.tile_fill(len(RC.graph(g)[0]) - 1) for g in used}
    assert fill["mixed37"] == (30, 6, 5)           # tiles rt >= 1 and waves 2..7 hold no row
    assert fill["dir101"] == (28, 4, 5) and fill["hub301"] == (22, 0, 13)
    assert fill["dir1001"] == (0, 0, 9)            # all 32 tiles, all 8 waves x 4, last one ragged
    assert any(f[0] > 0 for f in fill.values()) and any(f[1] > 0 for f in fill.values())
    assert all(f[2] > 0 for f in fill.values())    # every graph leaves a partly filled tile
    for g in used:
        rp = RC.graph(g)[0]
        M = len(rp) - 1
        empty = SC.empty_rows(rp)
        assert len(empty) >= 1 and (empty < M - 1).any(), g   # a zero-length row not in the last position
        starts = rp[:-1][np.diff(rp) > 0]
        assert (starts % 2 == 0).any() and (starts % 2 == 1).any(), g
    assert int((RC.graph("dir1001")[0][:-1] % 2 == 1).sum()) == 513
    assert len(SC.empty_rows(RC.graph("dir1001")[0])) == 25 and len(RC.graph("dir1001")[1]) == 7278
    # a dynamic-class tile with a long loop, forward and backward
    for rp in (RC.graph("hub301")[0], RC.tgraph("hub301")[0]):
        lens = RC.tile_lens(rp)
        assert RC.tile_classes(rp)[0] == RC.DYN and lens[0] >= 60 and lens[0] == 67


def test_directed_graphs_have_another_transpose():
    for g in ("dir101", "dir1001"):
        (rp, ci, v), (trp, tci, tv) = RC.graph(g), RC.tgraph(g)
        assert not np.array_equal(rp, trp), g
        assert sorted(np.diff(rp).tolist()) != sorted(np.diff(trp).tolist()), g
        assert not np.array_equal(RC.degree_order(rp), RC.degree_order(trp)), g
    rp, trp = RC.graph("dir1001")[0], RC.tgraph("dir1001")[0]
    fwd, bwd = RC.tile_classes(rp), RC.tile_classes(trp)
    assert fwd != bwd and fwd.count(4) == 6 and bwd.count(4) == 5
    assert set(fwd) == RC.ALL_CLASSES and set(bwd) == RC.ALL_CLASSES
    for g in ("chord100", "chord1000"):       # symmetric pattern, other values
        (rp, ci, v), (trp, tci, tv) = RC.graph(g), RC.tgraph(g)
        assert np.array_equal(rp, trp) and np.array_equal(ci, tci) and not np.array_equal(v, tv), g
    for g in ("mixed37", "hub301"):           # the symmetric controls
        for a, b in zip(RC.graph(g), RC.tgraph(g)):
            assert np.array_equal(a, b), g


def test_transpose_is_exact():
    rp, ci, v = RC.graph("dir101")
    trp, tci, tv = RC.tgraph("dir101")
    M = len(rp) - 1
    dense = np.zeros((M, M), np.float32)
    dense[np.repeat(np.arange(M), np.diff(rp)), ci] = v
    tdense = np.zeros((M, M), np.float32)
    tdense[np.repeat(np.arange(M), np.diff(trp)), tci] = tv
    assert np.array_equal(tdense, dense.T)
    assert all((np.diff(tci[trp[r]:trp[r + 1]]) > 0).all() for r in range(M))


@pytest.mark.parametrize("name", sorted(RC.GRAPHS))
def test_laplacian_round_trip_keeps_the_graph(name):
    """plan_for(laplacian_for(g)) holds L~ as given: rescale_L neither rounds a
    value, nor keeps an explicit zero, nor symmetrises."""
    rp, ci, v = G.canonical_csr(G.rescale_L(RC.laplacian_for(name), 2))
    for a, b in zip((rp, ci, v), RC.graph(name)):
        assert np.array_equal(a, b)


def test_xbasis_cases():
    for c in RC.XBASIS_CASES:
        rp = RC.graph(c["graph"])[0]
        lens = np.diff(rp)
        applies = RC.xbasis_applies(len(rp) - 1, c["Fin"], c["K"], int(lens.max()))
        assert applies == c["xbasis"], c["name"]
        if c["xbasis"]:
            assert lens.max() == RC.XL and {0, 1, 8, 9, 16} <= set(lens.tolist()), c["name"]
    assert sum(c["xbasis"] for c in RC.XBASIS_CASES) >= 4
    assert {c["graph"] for c in RC.XBASIS_CASES} == {"chord100", "chord1000", "dir101"}
    hub = RC.graph("hub301")[0]
    assert not RC.xbasis_applies(len(hub) - 1, 2, 3, int(np.diff(hub).max()))
    assert RC.xbasis_applies(1024, 2, 4, 16) and not RC.xbasis_applies(1024, 2, 4, 17)
    assert not RC.xbasis_applies(100, 3, 3, 16) and not RC.xbasis_applies(100, 2, 1, 16)
    assert not RC.xbasis_applies(100, 2, 5, 16) and not RC.xbasis_applies(1025, 1, 2, 16)


def test_tan_gate_stays_off_its_pole():
    """max|a_z| of the float64 oracle on every reference-gate case, with the
    halved bias range: the figures are printed (-s)."""
    worst = 0.0
    for tname in ("seq", "xbasis", "hstep", "layer"):
        for c in RC.LSTM_TABLES[tname]:
            if c["gates"] != "reference":
                continue
            rp, ci, v = RC.graph(c["graph"])
            d = RC.lstm_inputs(c)
            p = [d[k].astype(np.float64) for k in ("Wx", "Wh", "b")]
            _, _, caches = LO.layer_forward(d["xs"].astype(np.float64), p, (rp, ci, v.astype(np.float64)),
                                            c["K"], RC.H, d["c0"], d["h0"])
            # a_z itself from the cached bases (arctan(z) would fold a value
            # past the pole back under pi/2)
            az = max(float(np.abs((ca["Ax"] @ p[0] + ca["Ah"] @ p[1] + p[2])[:, :RC.H]).max())
                     for ca in caches)
            print(f"{c['name']}: max|a_z| = {az:.3f}")
            assert az < FE.AZ_MAX, c["name"]
            worst = max(worst, az)
    print(f"worst: {worst:.3f}")


def test_sizes():
    for table in list(RC.LSTM_TABLES.values()) + [RC.GROUP_CASES]:
        for c in table:
            assert RC.largest_array_bytes(c) < SC.MAX_ARRAY_BYTES, c["name"]
    c = RC.SEQ_CASES[0]
    d = RC.lstm_inputs(c)
    M = len(RC.graph(c["graph"])[0]) - 1
    assert d["xs"].shape == (3, c["N"], M, c["Fin"]) and d["Wh"].shape == (c["K"] * 32, 128)
    assert all(a is None or a.dtype == np.float32 for a in d.values())
    assert np.abs(d["b"]).max() <= RC.BIAS_RANGE and np.abs(d["Wx"]).max() <= 0.1
