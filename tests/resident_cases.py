"""Graphs, host restatements and the case tables of
tests/test_gpu_resident_geometry.py: the kernels that keep L~ (or L~^T) as CSR
in LDS and run the Chebyshev recurrence through csrc/lds_spmm.h -- k_lstm_seq,
k_xbasis and k_lstm_bstep (lstm_seq.hip), k_lstm_hstep (lstm_fused.hip) and the
channel-group kernels of cheb_group.hip.

Plain module, no GPU: tests/test_resident_cases_cpu.py checks that the tables
cover what they claim (row-length classes per tiling, ragged and empty tiles,
both parities of a row's CSR start, directed graphs whose L~^T differs, the
k_xbasis bound) and measures the tan gate's distance from its pole.

What a "class" is.  The kernels deal the rows to lanes in the plan's
degree-sorted order (lorder for L~, tlorder for L~^T: a stable sort by
decreasing row length), take the longest row of a group of lanes with wave_max
and unroll the gather to 4, 6, 8, 10 or 12 entries, or run the dynamic loop past
12 (lds_spmm.h::with_row_len).  Which rows share one switch differs per kernel;
the functions below restate each kernel's indexing.
"""
import numpy as np
import scipy.sparse

import stream_cases as SC
from test_gpu_fast_prologue import chord_ring

H = 32                     # hidden units of every LSTM kernel here
T = 3
DYN = 0                    # with_row_len's IntC<0>: the dynamic loop
ALL_CLASSES = {4, 6, 8, 10, 12, DYN}
WAVES = 8                  # every kernel here: 8 waves own the rows
TILE = 32
XL = 16                    # lstm_seq.hip::kXL
BIAS_RANGE = 0.153         # half of the cell's own +-0.306 (the tan gate, below)

GRAPHS = {
    # name: builder -> (rowptr, col, val)
    "mixed37": lambda: SC.graph("mixed37"),
    "dir101": lambda: SC.graph("dir101"),
    "hub301": lambda: SC.graph("hub301"),
    "dir1001": lambda: SC.directed_rows(1001, 22),
    "chord100": lambda: chord_ring(100, 1100)[:3],
    "chord1000": lambda: chord_ring(1000, 2000)[:3],
}
_BUILT = {}


def graph(name):
    """(rowptr, col, val) of GRAPHS[name], built once."""
    if name not in _BUILT:
        _BUILT[name] = GRAPHS[name]()
    return _BUILT[name]


def csr(name):
    rp, ci, v = graph(name)
    M = len(rp) - 1
    return scipy.sparse.csr_matrix((v, ci, rp), shape=(M, M))


def transpose(rowptr, col, val):
    """(trowptr, tcol, tval) of L~^T, sorted columns: what cg_plan_create builds
    (cheb_abi.cpp: trp / tci / tv, an exact transpose in CSR)."""
    M = len(rowptr) - 1
    AT = scipy.sparse.csr_matrix((val, col, rowptr), shape=(M, M)).T.tocsr()
    AT.sort_indices()
    return AT.indptr.astype(np.int32), AT.indices.astype(np.int32), AT.data.astype(np.float32)


def tgraph(name):
    return transpose(*graph(name))


def laplacian_for(name):
    """A float64 L with rescale_L(L, lmax=2) == L~ exactly (L = L~ + I in
    float64 loses no bit of a float32 entry above 2^-29), for cells built
    through plan_for: the plan then holds the directed L~ as given."""
    Lt = csr(name).astype(np.float64)
    return (Lt + scipy.sparse.identity(Lt.shape[0], dtype=np.float64, format="csr")).tocsr()


# ---- host restatements ---------------------------------------------------------
def row_class(length):
    """lds_spmm.h::with_row_len: ``if (len <= 4) f(IntC<4>{}); else if (len <= 6)
    ... else if (len <= 12) f(IntC<12>{}); else f(IntC<0>{});``"""
    for bound in (4, 6, 8, 10, 12):
        if length <= bound:
            return bound
    return DYN


def degree_order(rowptr):
    """cheb_abi.cpp::cg_plan_create: ``std::stable_sort(o.begin(), o.end(), [rp](a, b)
    { return rp[a + 1] - rp[a] > rp[b + 1] - rp[b]; })`` -- lorder / tlorder."""
    return np.argsort(-np.diff(rowptr), kind="stable")


def _sorted_lens(rowptr, slots):
    """Row length at every lane slot of the sorted order; slots past M are the
    padding rows (``idx < M ? order[idx] : M``, rb = re = 0: length 0), -1 marks them."""
    lens = np.diff(rowptr)[degree_order(rowptr)]
    out = np.full(slots, -1, np.int64)
    out[:len(lens)] = lens
    return out


def tile_lens(rowptr, rows_per_tile=TILE):
    """Longest row of each tile of ``rows_per_tile`` consecutive entries of the
    sorted order that holds a row (wave_max(re - rb))."""
    M = len(rowptr) - 1
    n = -(-M // rows_per_tile)
    lens = _sorted_lens(rowptr, n * rows_per_tile).reshape(n, rows_per_tile)
    return np.maximum(lens, 0).max(axis=1)


def tile_classes(rowptr, rows_per_tile=TILE):
    """The class of each tile under the stable degree sort.  This is the
    switch of k_lstm_seq (lstm_seq.hip: ``idx = (wave + 8 * rt) * 32 + j``,
    ``with_row_len(wl[rt], ...)``), k_grp_fwd and k_grp_clen (cheb_group.hip,
    the same idx) and of k_grp16_fwd, whose two 16-row halves of a tile share
    ``with_row_len(wl[rt][0] > wl[rt][1] ? wl[rt][0] : wl[rt][1], ...)``."""
    return [row_class(int(v)) for v in tile_lens(rowptr, rows_per_tile)]


def bstep_classes(trowptr):
    """k_lstm_bstep: lane (rt, jr) of wave w owns ``order[wave * 128 + rt * 16 + jr]``
    (kRB = 8 tiles of 16 rows) and tiles rp, rp + 1 share
    ``with_row_len(wl[rp] > wl[rp + 1] ? wl[rp] : wl[rp + 1], ...)``: 32
    consecutive entries of tlorder.  One class per pair that holds a row."""
    lens = _sorted_lens(trowptr, WAVES * 128)
    out = []
    for w in range(WAVES):
        for rp in range(0, 8, 2):
            idx = w * 128 + rp * 16 + np.arange(32)
            if (lens[idx] >= 0).any():
                out.append(row_class(int(max(lens[idx].max(), 0))))
    return out


def clen_dy_classes(trowptr):
    """k_grp_clen_dy: lane j of wave w owns ``order[(wave + 8 * rt) * 32 + j]``
    (kGRT = 4) and tiles rp, rp + 1 share ``with_row_len(wl[rp] > wl[rp + 1] ?
    ...)``: the 32-row tiles w + 8 rp and w + 8 rp + 8 of tlorder, which are NOT
    neighbours in the order.  One class per pair that holds a row."""
    lens = _sorted_lens(trowptr, WAVES * 4 * TILE).reshape(WAVES * 4, TILE)
    out = []
    for w in range(WAVES):
        for rp in (0, 2):
            pair = lens[[w + 8 * rp, w + 8 * rp + 8]]
            if (pair >= 0).any():
                out.append(row_class(int(max(pair.max(), 0))))
    return out


def tile_fill(M):
    """(tiles with no row, waves with no row, rows in the partly filled tile or
    0) of the forward tiling: tile (wave, rt) holds sorted entries
    [(wave + 8 rt) 32, + 32), 32 tiles in all."""
    full, part = divmod(M, TILE)
    used = full + (part > 0)
    return WAVES * 4 - used, max(0, WAVES - used), part


def xbasis_applies(M, Fin, K, max_row):
    """lstm_seq.hip::launch_lstm_seq: ``Fin <= 2 && K >= 2 && K <= 4 && M <= kXT &&
    max_row_nnz <= kXL`` (kXT = 1024, kXL = 16; the LDS bound K M Fin 4 B <= 160 KB
    follows from these) -- with CG_OPT_SEQ_XPRE = 1 the x basis comes from k_xbasis."""
    return Fin <= 2 and 2 <= K <= 4 and M <= 1024 and max_row <= XL


# ---- case tables ---------------------------------------------------------------
def _table():
    rows = []

    def add(name, graph, N, Fin, K, gates, covers, **kw):
        assert all(r["name"] != name for r in rows), name
        rows.append(dict(name=name, graph=graph, N=N, T=T, Fin=Fin, K=K, gates=gates,
                         covers=covers, **kw))
    return rows, add


# k_lstm_seq: fused x (in-kernel recurrence and pre-pass) and precomputed gx
SEQ_CASES, _seq = _table()
_seq("seq_mixed37_k1", "mixed37", 3, 2, 1, "reference", "K = 1: no plane; waves 2..7 idle", state=False,
     x="normal")
_seq("seq_mixed37_k2", "mixed37", 1, 8, 2, "standard", "padding tiles, one empty row; Fin = 8", state=True,
     x="uniform")
_seq("seq_dir101_n8", "dir101", 8, 1, 4, "reference", "pair_xcd on (N % 8 == 0); ragged fourth tile",
     state=True, x="uniform")
_seq("seq_dir101_k3", "dir101", 3, 5, 3, "standard", "directed pattern, Fin = 5", state=False, x="normal")
_seq("seq_hub301_k3", "hub301", 3, 2, 3, "reference", "all six classes, 67-entry dynamic rows",
     state=True, x="normal")
_seq("seq_hub301_k4", "hub301", 1, 5, 4, "reference", "all six classes at K = 4", state=False,
     x="uniform")
_seq("seq_dir1001_k3", "dir1001", 1, 2, 3, "reference", "all 32 tiles in use, last one ragged",
     state=True, x="uniform")
_seq("seq_dir1001_k2", "dir1001", 3, 8, 2, "standard", "all 32 tiles, Fin = 8", state=False, x="normal")
_seq("seq_dir1001_k4", "dir1001", 1, 1, 4, "standard", "all 32 tiles at K = 4, Fin = 1", state=True,
     x="normal")

# k_xbasis (CG_OPT_SEQ_XPRE = 1) against the streaming launches (= 2)
XBASIS_CASES, _xb = _table()
_xb("xb_chord100_f1k2", "chord100", 3, 1, 2, "reference", "rows of 0, 1, 8, 9, 16; M < 128", state=False,
    x="uniform", xbasis=True)
_xb("xb_chord100_f2k4", "chord100", 1, 2, 4, "standard", "K = 4, Fin = 2", state=True, x="normal",
    xbasis=True)
_xb("xb_chord1000_f1k3", "chord1000", 3, 1, 3, "reference", "M = 1000: 24 idle lanes", state=True,
    x="normal", xbasis=True)
_xb("xb_chord1000_f2k2", "chord1000", 1, 2, 2, "standard", "K = 2, Fin = 2", state=False, x="uniform",
    xbasis=True)
_xb("xb_chord1000_f2k4", "chord1000", 1, 2, 4, "reference", "K = 4, Fin = 2 at M = 1000", state=False,
    x="uniform", xbasis=True)
_xb("xb_dir101_f2k3", "dir101", 3, 2, 3, "reference", "a 17-entry row: the streaming launches instead",
    state=False, x="normal", xbasis=False)
_xb("xb_dir101_f1k4", "dir101", 1, 1, 4, "standard", "the same, Fin = 1, K = 4", state=True, x="uniform",
    xbasis=False)

# k_lstm_hstep
HSTEP_CASES, _hs = _table()
_hs("hs_dir101_n8", "dir101", 8, 2, 3, "reference", "pair_xcd on; directed pattern", state=True, x="normal")
_hs("hs_hub301_n3", "hub301", 3, 2, 4, "standard", "67-entry rows, empty rows", state=True, x="normal")
_hs("hs_dir1001_n3", "dir1001", 3, 2, 2, "reference", "M = 1001: 23 idle threads", state=True, x="normal")
_hs("hs_mixed37_k1", "mixed37", 3, 2, 1, "reference", "K = 1, one partly filled MFMA tile pair",
    state=True, x="normal")

# k_lstm_bstep: K x gates on the three graphs with a switch that matters
BSTEP_CASES, _bs = _table()
# N per K for the reference gates; the standard gates take the list two places on
for _g, _ns in (("dir101", (8, 3, 1, 8)), ("hub301", (3, 1, 3, 1)), ("dir1001", (1, 3, 1, 3))):
    for _K in (1, 2, 3, 4):
        for _gates in ("reference", "standard"):
            _n = _ns[_K - 1] if _gates == "reference" else _ns[(_K + 1) % 4]
            _bs(f"bs_{_g}_k{_K}_{_gates[:3]}", _g, _n, 0, _K, _gates,
                "tlorder pairs of 16-row tiles" + ("; pair_xcd on" if _n % 8 == 0 else ""))

# layer(): the kernels under the Python glue, N = 3, K = 3
LAYER_CASES, _ly = _table()
for _g in ("dir101", "hub301"):
    _ly(f"layer_{_g}", _g, 3, 2, 3, "reference", "autograd through seq / fused / unfused", state=True,
        x="normal")

# The channel-group kernels.  fwd: the forward group kernel, which serves the
# planes layout only (Fin % 16 == 0): "grp16" = k_grp16_fwd (Fout <= 32; with
# CG_OPT_GRP16 = 0 the same case runs k_grp_fwd<1>), "grp" = k_grp_fwd<2>
# (Fout = 64), None = rows layout, the streaming forward.  bwd: 2 =
# k_grp_clen_dy (Fout 2 / 32 / 64), 1 = k_grp_clen (from dBasis planes).
GROUP_CASES = []


def _grp(name, graph, N, Fin, K, Fout, covers, accumulate=False):
    assert all(r["name"] != name for r in GROUP_CASES), name
    fwd = None if Fin % 16 else "grp16" if Fout <= 32 else "grp"
    GROUP_CASES.append(dict(name=name, graph=graph, N=N, Fin=Fin, K=K, Fout=Fout, fwd=fwd,
                            bwd=2 if Fout in (2, 32, 64) else 1, covers=covers,
                            accumulate=accumulate, layout="planes" if fwd else "rows"))


_grp("g_dir101_f8k2o32", "dir101", 3, 8, 2, 32, "one order group of 2; dx accumulate", accumulate=True)
_grp("g_dir101_f16k5o2", "dir101", 8, 16, 5, 2, "Fout = 2, two channel groups, N = 8")
_grp("g_dir101_f24k7o20", "dir101", 1, 24, 7, 20, "dBasis planes, three channel groups")
_grp("g_dir101_f8k5o64", "dir101", 1, 8, 5, 64, "Fout = 64 with a class-4 pair (far pairing)")
_grp("g_hub301_f16k7o32", "hub301", 3, 16, 7, 32, "all six classes, two order groups")
_grp("g_hub301_f16k2o64", "hub301", 1, 16, 2, 64, "k_grp_fwd<2>: two output tiles, all six classes")
_grp("g_hub301_f8k5o64", "hub301", 1, 8, 5, 64, "Fout = 64, one channel group")
_grp("g_hub301_f24k2o20", "hub301", 3, 24, 2, 20, "dBasis planes: packed columns and the dynamic loop")
_grp("g_dir1001_f16k5o32", "dir1001", 1, 16, 5, 32, "all 32 tiles, L~^T tiles differ from L~")
_grp("g_dir1001_f16k7o64", "dir1001", 3, 16, 7, 64, "k_grp_fwd<2> on all 32 tiles")
_grp("g_dir1001_f8k2o20", "dir1001", 1, 8, 2, 20, "dBasis planes on all 32 tiles")
_grp("g_dir1001_f24k5o2", "dir1001", 1, 24, 5, 2, "Fout = 2 on all 32 tiles")

LSTM_TABLES = dict(seq=SEQ_CASES, xbasis=XBASIS_CASES, hstep=HSTEP_CASES, bstep=BSTEP_CASES,
                   layer=LAYER_CASES)


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def lstm_inputs(case):
    """The numbers of one forward LSTM case, float32, drawn in numpy from the
    case's name: Wx [K Fin, 4H] and Wh [K H, 4H] uniform(+-0.1), b uniform
    (+-BIAS_RANGE), xs [T, N, M, Fin] standard normal or uniform [0, 1), and
    (state=True) c0, h0 = 0.5 N(0, 1), else None."""
    M = len(graph(case["graph"])[0]) - 1
    N, Fin, K = case["N"], case["Fin"], case["K"]
    rng = np.random.default_rng(_seed(case["name"]))
    f32 = np.float32
    Wx = rng.uniform(-0.1, 0.1, (K * Fin, 4 * H)).astype(f32)
    Wh = rng.uniform(-0.1, 0.1, (K * H, 4 * H)).astype(f32)
    b = rng.uniform(-BIAS_RANGE, BIAS_RANGE, 4 * H).astype(f32)
    shape = (case["T"], N, M, Fin)
    xs = (rng.standard_normal(shape) if case["x"] == "normal" else rng.random(shape)).astype(f32)
    c0 = h0 = None
    if case["state"]:
        c0 = (0.5 * rng.standard_normal((N, M, H))).astype(f32)
        h0 = (0.5 * rng.standard_normal((N, M, H))).astype(f32)
    return dict(Wx=Wx, Wh=Wh, b=b, xs=xs, c0=c0, h0=h0)


def bstep_inputs(case):
    """One backward step's numbers: gate-major act [N, M, 4H] (z and o through
    tanh, i and f through a sigmoid of N(0, 1)), c_prev, c_out, dh, dh_rec, dc
    ~ N(0, 1), Wh = 0.1 N(0, 1)."""
    M = len(graph(case["graph"])[0]) - 1
    N, K = case["N"], case["K"]
    rng = np.random.default_rng(_seed(case["name"]))
    rn = lambda *sh: rng.standard_normal(sh)  # noqa: E731
    act = np.concatenate([np.tanh(rn(N, M, H)), 1 / (1 + np.exp(-rn(N, M, 2 * H))),
                          np.tanh(rn(N, M, H))], -1).astype(np.float32)
    out = dict(act=act)
    for k in ("c_prev", "c_out", "dh", "dh_rec", "dc"):
        out[k] = rn(N, M, H).astype(np.float32)
    out["Wh"] = (0.1 * rn(K * H, 4 * H)).astype(np.float32)
    return out


def group_inputs(case):
    """stream_cases.inputs' draw: x uniform [0, 1) with the empty rows zeroed,
    W = 0.1 N(0, 1), dy and dx0 ~ N(0, 1)."""
    rp = graph(case["graph"])[0]
    M = len(rp) - 1
    N, Fin, K, Fout = (case[k] for k in ("N", "Fin", "K", "Fout"))
    rng = np.random.default_rng(_seed(case["name"]))
    x = rng.random((N, M, Fin), dtype=np.float32)
    x[:, SC.empty_rows(rp), :] = 0
    W = (rng.standard_normal((Fin * K, Fout)) * 0.1).astype(np.float32)
    dy = rng.standard_normal((N, M, Fout)).astype(np.float32)
    dx0 = rng.standard_normal((N, M, Fin)).astype(np.float32)
    return x, W, dy, dx0


def largest_array_bytes(case):
    """The largest array a case allocates: the act / gx / dpre records of an LSTM
    case ([T, N, M, 4H]), the basis or partial y of a group case."""
    M = len(graph(case["graph"])[0]) - 1
    if "Fout" in case:
        N, Fin, K, Fout = (case[k] for k in ("N", "Fin", "K", "Fout"))
        return 4 * N * M * max(Fin * K, (Fin // 8) * Fout)
    return 4 * case["T"] * case["N"] * M * max(4 * H, case["K"] * case["Fin"])
