"""Graphs and the case table of tests/test_gpu_stream_geometry.py: small
synthetic graphs and the smallest shapes that reach every dispatch class of the
streaming path (cheb_stream.hip's sample-major steps and cheb_wide.hip).

Plain module, no GPU: tests/test_stream_cases_cpu.py checks the builders'
promises and the table's size; the GPU test asserts that every case lands in
the class it names (ChebPlan.stream_dispatch) before it compares numbers.

Graphs.  ``mixed_rows`` has pinned vertices of exactly 0, 1, 3, 4, 5, 7, 8, 9,
11, 12, 13, 16 and 17 entries -- every combination of the 8 / 4 / 1-entry loops
of wide_gather and of the 4 / 1-entry loops of row_spmm -- joined to a body of
"filler" vertices (a ring with a diagonal, 3..16 entries); the pattern is
symmetric and not skewed, so the plan keeps the natural row order.
``hub_rows`` adds hubs of >= 60 entries, which makes the plan build the
degree-sorted row orders.  ``directed_rows`` adds one-way edges, so L~ and L~^T
differ in pattern and in row lengths.  Values are N(0, 1), equal on the two
directions of a two-way edge, scaled so that the largest absolute row sum and
column sum are <= 1: the recurrence stays bounded through K = 40.
"""
import numpy as np
import scipy.sparse

LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16, 17)
FILLER_MAX = 16          # a filler row never grows past this many entries
HUB_MIN = 60
MAX_ARRAY_BYTES = 32 << 20   # no case's largest array may pass this


def skew_bound(rowptr):
    """The plan builds the degree-sorted row orders when max row > this."""
    M = len(rowptr) - 1
    return 2 * (int(rowptr[-1]) // M) + 8


def _build(M, seed, hubs=0, one_way=0):
    rng = np.random.default_rng(seed)
    reps = max(1, M // 40)
    npin = reps * len(LENGTHS)
    assert M - 2 - npin - hubs >= 20, "too few filler vertices"
    # vertices 0 and M-1 are fillers: neither end of the degree-sorted order
    # (hubs first, empty rows last) coincides with the natural order
    inner = 1 + rng.permutation(M - 2)
    pinned, hub_v = inner[:npin], inner[npin:npin + hubs]
    filler = np.concatenate([[0, M - 1], inner[npin + hubs:]])
    filler = filler[rng.permutation(len(filler))]
    nbr = {int(v): set() for v in range(M)}
    body = [int(v) for v in np.concatenate([filler, hub_v])]
    for i, a in enumerate(body):          # a ring with a diagonal: 3 entries each
        b = body[(i + 1) % len(body)]
        nbr[a] |= {a, b}
        nbr[b].add(a)
    fill = [int(v) for v in filler]

    def attach(v, count):
        got = 0
        for j in rng.permutation(len(fill)):
            if got == count:
                break
            f = fill[j]
            if f not in nbr[v] and len(nbr[f]) < FILLER_MAX:
                nbr[v].add(f)
                nbr[f].add(v)
                got += 1
        assert got == count, "not enough filler vertices with room"

    for i, v in enumerate(pinned):
        t = LENGTHS[i % len(LENGTHS)]
        if t >= 1:
            nbr[int(v)].add(int(v))
            attach(int(v), t - 1)
    for v in hub_v:
        attach(int(v), HUB_MIN + 4)
    out = {v: set(s) for v, s in nbr.items()}
    added = 0
    for j in rng.permutation(len(fill)):     # one-way edges u -> w between fillers
        if added == one_way:
            break
        u, w = fill[j], fill[(j + 7) % len(fill)]
        incoming = sum(1 for s in out.values() if w in s)
        if w not in out[u] and u not in out[w] and len(out[u]) < FILLER_MAX and incoming < FILLER_MAX:
            out[u].add(w)
            added += 1
    assert added == one_way
    rowptr, col = [0], []
    for v in range(M):
        col.extend(sorted(out[v]))
        rowptr.append(len(col))
    rowptr, col = np.asarray(rowptr, np.int32), np.asarray(col, np.int32)
    # symmetric values on the symmetric part (real spectrum in [-1, 1] after
    # the scaling, so T_k(L~) stays bounded), independent ones on one-way edges
    rows = np.repeat(np.arange(M), np.diff(rowptr))
    lo, hi = np.minimum(rows, col), np.maximum(rows, col)
    _, pair = np.unique(lo.astype(np.int64) * M + hi, return_inverse=True)
    val = rng.standard_normal(int(pair.max()) + 1).astype(np.float32)[pair]
    A = scipy.sparse.csr_matrix((np.abs(val), col, rowptr), shape=(M, M))
    norm = max(float(A.sum(axis=1).max()), float(A.sum(axis=0).max()))
    val = (val / np.float32(norm * 1.0001)).astype(np.float32)
    return rowptr, col, val


def mixed_rows(M, seed):
    """Symmetric pattern, every length of LENGTHS present, not skewed."""
    rp, ci, v = _build(M, seed)
    assert np.diff(rp).max() <= skew_bound(rp)
    return rp, ci, v


def hub_rows(M, seed, hubs=3):
    """mixed_rows' body plus ``hubs`` rows of >= HUB_MIN entries: skewed."""
    rp, ci, v = _build(M, seed, hubs=hubs)
    assert np.diff(rp).max() > skew_bound(rp)
    return rp, ci, v


def directed_rows(M, seed):
    """mixed_rows plus M // 4 one-way edges: L~ and L~^T differ in pattern."""
    rp, ci, v = _build(M, seed, one_way=M // 4)
    assert np.diff(rp).max() <= skew_bound(rp)
    return rp, ci, v


GRAPHS = {
    # name: (builder, M, seed); M leaves a ragged last row block for the
    # classes that use the graph (37 = 9*4 + 1, 101 = 3*32 + 5 = 64 + 37,
    # 259 = 256 + 3 = 2*128 + 3, 301 = 9*32 + 13, 2049 = 2048 + 1)
    "mixed37": (mixed_rows, 37, 11),
    "mixed101": (mixed_rows, 101, 12),
    "mixed259": (mixed_rows, 259, 13),
    "hub301": (hub_rows, 301, 14),
    "dir101": (directed_rows, 101, 15),
    "mixed2049": (mixed_rows, 2049, 16),
}
_BUILT = {}


def graph(name):
    """(rowptr, col, val) of GRAPHS[name], built once."""
    if name not in _BUILT:
        fn, M, seed = GRAPHS[name]
        _BUILT[name] = fn(M, seed)
    return _BUILT[name]


def empty_rows(rowptr):
    return np.nonzero(np.diff(rowptr) == 0)[0]


def inputs(case):
    """x uniform in [0, 1) with the empty rows zeroed, W ~ 0.1 N(0, 1), dy and
    the dx_accumulate start dx0 ~ N(0, 1); seeded by the case's name."""
    rp = graph(case["graph"])[0]
    M = len(rp) - 1
    N, Fin, K, Fout = (case[k] for k in ("N", "Fin", "K", "Fout"))
    rng = np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(case["name"])))
    x = rng.random((N, M, Fin), dtype=np.float32)
    x[:, empty_rows(rp), :] = 0
    W = (rng.standard_normal((Fin * K, Fout)) * 0.1).astype(np.float32)
    dy = rng.standard_normal((N, M, Fout)).astype(np.float32)
    dx0 = rng.standard_normal((N, M, Fin)).astype(np.float32)
    return x, W, dy, dx0


def largest_array_bytes(case):
    M = GRAPHS[case["graph"]][1]
    N, Fin, K, Fout = (case[k] for k in ("N", "Fin", "K", "Fout"))
    return 4 * N * M * max(Fin * K, Fout)


# ---- the dispatch classes (fields of ChebPlan.stream_dispatch) -----------------
FIELDS = ("wide", "G", "CB", "pl", "fused_last", "assemble_tm", "dypass", "sorted_rows_fwd",
          "sorted_rows_bwd", "group_fwd", "group_bwd", "vec", "lpr", "rpw", "xcd_map",
          "last_staged")


def wide(G, CB, pl, fused=0, tm=0, dyp=0, srt=0):
    """A wide-column class.  fused: k_wide_last; tm: k_wide_assemble's rows per
    tile (0 = not launched); dyp: 0 row-GEMM planes, 1 dypass_small, 2 MFMA
    dypass; srt: degree-sorted row order, forward and backward."""
    return dict(wide=1, G=G, CB=CB, pl=pl, fused_last=fused, assemble_tm=tm, dypass=dyp,
                sorted_rows_fwd=srt, sorted_rows_bwd=srt, group_fwd=0, group_bwd=0, vec=0, lpr=0,
                rpw=0, xcd_map=0, last_staged=-1)


def narrow(vec, lpr, rpw, xcd=1, staged=1, srt=0):
    """A sample-major class.  staged: 1 k_cheb_last, 0 k_cheb_step<., true>,
    -1 no assembling step (planes layout, K = 1)."""
    return dict(wide=0, G=0, CB=0, pl=0, fused_last=0, assemble_tm=0, dypass=0,
                sorted_rows_fwd=srt, sorted_rows_bwd=srt, group_fwd=0, group_bwd=0, vec=vec,
                lpr=lpr, rpw=rpw, xcd_map=xcd, last_staged=staged)


CASES = []


def _case(name, graph, N, Fin, K, Fout, expect, variant="auto", layout="rows"):
    assert set(expect) == set(FIELDS)
    assert all(c["name"] != name for c in CASES), name
    CASES.append(dict(name=name, graph=graph, N=N, Fin=Fin, K=K, Fout=Fout, expect=expect,
                      variant=variant, layout=layout))


# -- wide columns, forward geometry: B = N*Fin = G*CB, lpr = CB/pl lanes per row,
#    4*(64/lpr) rows per block.  dypass_small<FJ>: FJ = Fin*K.
_case("w_b1", "mixed259", 1, 1, 3, 8, wide(1, 1, 1, fused=1, dyp=1))                # FJ 3, N 1
_case("w_b2_fin1", "mixed259", 2, 1, 4, 8, wide(1, 2, 2, fused=1, dyp=1))           # FJ 4, N 2
_case("w_b2_fin2", "mixed259", 1, 2, 2, 8, wide(1, 2, 2, tm=32, dyp=1))             # FJ 4
_case("w_b4_fin1", "mixed259", 4, 1, 5, 8, wide(1, 4, 4, fused=1, dyp=1))           # FJ 5, N 4
_case("w_b4_fin2", "mixed259", 2, 2, 3, 8, wide(1, 4, 4, tm=32, dyp=1))             # FJ 6
_case("w_b8", "mixed259", 8, 1, 2, 8, wide(1, 8, 4, fused=1, dyp=1))                # FJ 2, N 8
_case("w_b16_fin1", "mixed101", 16, 1, 7, 8, wide(1, 16, 4, fused=1, dyp=1))        # FJ 7, N 16
_case("w_b16_fin2", "mixed101", 8, 2, 2, 8, wide(1, 16, 4, tm=32, dyp=1))
_case("w_b16_fin4", "mixed101", 4, 4, 2, 8, wide(1, 16, 4, tm=32, dyp=1))           # FJ 8
_case("w_b32_k1", "mixed101", 32, 1, 1, 8, wide(1, 32, 4, dyp=1))                   # FJ 1, K 1
_case("w_b32_k2", "mixed101", 32, 1, 2, 8, wide(1, 32, 4, fused=1, dyp=1))          # K 2
_case("w_b64", "mixed37", 64, 1, 3, 8, wide(2, 32, 4, fused=1, dyp=1))              # G 2, N 64
_case("w_b128", "mixed37", 32, 4, 2, 8, wide(4, 32, 4, tm=32, dyp=1))               # G 4
_case("w_b256", "mixed37", 64, 4, 2, 8, wide(8, 32, 4, tm=32, dyp=1))               # G 8
_case("w_b512", "mixed37", 512, 1, 3, 8, wide(8, 64, 4, fused=1, dyp=1))            # CB 64
_case("w_b1024", "mixed37", 512, 2, 3, 8, wide(8, 128, 4, tm=32, dyp=1))            # CB 128
_case("w_b2048_fin1", "mixed37", 2048, 1, 2, 8, wide(8, 256, 4, fused=1, dyp=1))    # CB 256, lpr 64
_case("w_b2048_fin4", "mixed37", 512, 4, 2, 8, wide(8, 256, 4, tm=32, dyp=1))
# -- the fused last step's LDS bound at CB = 32, pl = 4 (32 rows per block):
#    32 * (32 K + 1) * 4 B <= 64 KB  <=>  K <= 15
_case("w_last_k15", "mixed101", 32, 1, 15, 8, wide(1, 32, 4, fused=1, dyp=2))
_case("w_last_k16", "mixed101", 32, 1, 16, 8, wide(1, 32, 4, tm=16, dyp=2))         # FinK 16
# -- k_wide_assemble: TM = min(32, 256 // FinK), at least 1
_case("w_asm_fin2_tm6", "mixed101", 16, 2, 20, 8, wide(1, 32, 4, tm=6))             # FinK 40
_case("w_asm_fin4_tm1", "mixed101", 8, 4, 40, 8, wide(1, 32, 4, tm=1))              # FinK 160
# -- the same on the skewed graph: sorted rows, no fused last step
_case("w_hub_fin1", "hub301", 32, 1, 3, 8, wide(1, 32, 4, tm=32, dyp=1, srt=1))
_case("w_hub_fin1_k16", "hub301", 32, 1, 16, 8, wide(1, 32, 4, tm=16, dyp=2, srt=1))
_case("w_hub_fin2_tm6", "hub301", 16, 2, 20, 8, wide(1, 32, 4, tm=6, srt=1))
_case("w_hub_fin4_tm1", "hub301", 8, 4, 40, 8, wide(1, 32, 4, tm=1, srt=1))
_case("w_hub_b4", "hub301", 4, 1, 2, 16, wide(1, 4, 4, tm=32, dyp=1, srt=1))
# -- the backward's dense dy pass: MFMA kernel at FinK 9, 16 (above), 32;
#    Fout 8 / 16 / 24 / 32 on both kernels; partial and two sample tiles
_case("w_dy_mfma9", "mixed101", 32, 1, 9, 8, wide(1, 32, 4, fused=1, dyp=2))
_case("w_dy_mfma9_f16", "mixed101", 32, 1, 9, 16, wide(1, 32, 4, fused=1, dyp=2))
_case("w_dy_mfma9_f24", "mixed101", 32, 1, 9, 24, wide(1, 32, 4, fused=1, dyp=2))
_case("w_dy_mfma9_f32", "mixed101", 32, 1, 9, 32, wide(1, 32, 4, fused=1, dyp=2))
_case("w_dy_mfma32", "mixed101", 16, 2, 16, 8, wide(1, 32, 4, tm=8, dyp=2))         # FinK 32
_case("w_dy_mfma10_n2", "mixed101", 2, 2, 5, 24, wide(1, 4, 4, tm=25, dyp=2))       # N 2
_case("w_dy_mfma9_n64", "mixed37", 64, 1, 9, 8, wide(2, 32, 4, fused=1, dyp=2))     # N 64
_case("w_dy_small5_f16", "mixed101", 32, 1, 5, 16, wide(1, 32, 4, fused=1, dyp=1))
_case("w_dy_small5_f24", "mixed101", 32, 1, 5, 24, wide(1, 32, 4, fused=1, dyp=1))
_case("w_dy_small5_f32", "mixed101", 32, 1, 5, 32, wide(1, 32, 4, fused=1, dyp=1))
_case("w_dy_small6_n1_f24", "mixed101", 1, 2, 3, 24, wide(1, 2, 2, tm=32, dyp=1))   # N 1
# -- no dy pass: Fout past 32, Fout no multiple of 8, FinK past 32
_case("w_nody_f40", "mixed101", 32, 1, 4, 40, wide(1, 32, 4, fused=1))
_case("w_nody_f12", "mixed101", 16, 2, 3, 12, wide(1, 32, 4, tm=32))
_case("w_nody_fk36", "mixed101", 8, 4, 9, 8, wide(1, 32, 4, tm=7))
# -- L~^T with its own pattern and row lengths
_case("w_dir_fin1", "dir101", 32, 1, 5, 8, wide(1, 32, 4, fused=1, dyp=1))
_case("w_dir_fin2", "dir101", 16, 2, 6, 16, wide(1, 32, 4, tm=21, dyp=2))
_case("w_dir_nody", "dir101", 32, 1, 4, 12, wide(1, 32, 4, fused=1))

# -- sample-major steps: vec = 4 floats per lane where Fin % 4 == 0, lpr =
#    min(64, ceil(Fin / vec)) lanes per row, 64 // lpr rows per wave.  Shapes
#    wide_geometry refuses (B no power of two), or variant 'narrow'; Fin % 8 ==
#    0 at M <= 1024 under variant 'steps', which keeps the group kernels out.
_case("n_fin1", "mixed259", 3, 1, 3, 8, narrow(1, 1, 64))
_case("n_fin1_narrow", "mixed101", 32, 1, 5, 8, narrow(1, 1, 64), variant="narrow")
_case("n_fin3", "mixed101", 1, 3, 4, 8, narrow(1, 3, 21))
_case("n_fin5", "mixed101", 9, 5, 3, 8, narrow(1, 5, 12))
_case("n_fin8", "mixed101", 3, 8, 3, 8, narrow(4, 2, 32), variant="steps")
_case("n_fin12", "mixed101", 1, 12, 2, 8, narrow(4, 3, 21))
_case("n_fin20", "mixed101", 3, 20, 3, 8, narrow(4, 5, 12))
_case("n_fin64", "mixed37", 1, 64, 3, 8, narrow(4, 16, 4), variant="steps")
_case("n_fin64_planes", "mixed37", 1, 64, 3, 8, narrow(4, 16, 4, staged=-1), variant="steps",
      layout="planes")
_case("n_fin65", "mixed37", 3, 65, 2, 8, narrow(1, 64, 1))
_case("n_fin260", "mixed37", 1, 260, 3, 8, narrow(4, 64, 1))
_case("n_k1", "mixed101", 3, 5, 1, 8, narrow(1, 5, 12, staged=-1))
# -- the last step's LDS staging, 4 * rpw * (Fin*K + 1) * 4 B against 160 KB:
#    Fin = 8 (rpw 32): K = 39 -> 160 256 B staged, K = 40 -> 164 352 B not
_case("n_staged_k39", "mixed37", 1, 8, 39, 8, narrow(4, 2, 32), variant="steps")
_case("n_unstaged_k40", "mixed37", 1, 8, 40, 8, narrow(4, 2, 32, staged=0), variant="steps")
# -- a sample slab past 2 MB (2049 * 260 * 4 B): all blocks of a sample together
_case("n_noxcd", "mixed2049", 2, 260, 2, 8, narrow(4, 64, 1, xcd=0))
# -- the skewed graph: sorted rows from Fin = 16 on
_case("n_hub_fin16", "hub301", 3, 16, 4, 8, narrow(4, 4, 16, srt=1), variant="steps")
_case("n_hub_fin16_planes", "hub301", 3, 16, 4, 8, narrow(4, 4, 16, srt=1, staged=-1),
      variant="steps", layout="planes")
_case("n_hub_fin20", "hub301", 1, 20, 3, 8, narrow(4, 5, 12, srt=1))
_case("n_hub_fin8", "hub301", 3, 8, 3, 8, narrow(4, 2, 32), variant="steps")
_case("n_dir_fin3", "dir101", 3, 3, 4, 8, narrow(1, 3, 21))
_case("n_dir_fin16", "dir101", 1, 16, 3, 16, narrow(4, 4, 16), variant="steps")
_case("n_dir_fin16_planes", "dir101", 1, 16, 3, 16, narrow(4, 4, 16, staged=-1), variant="steps",
      layout="planes")


# ---- coverage: every class the table exists for ---------------------------------
def _w(d):
    return d["wide"] == 1


CLASSES = {}
for _pl in (1, 2, 4):
    CLASSES[f"wide pl={_pl}"] = lambda c, d, p=_pl: _w(d) and d["pl"] == p
for _cb in (1, 2, 4, 8, 16, 32, 64, 128, 256):
    CLASSES[f"wide CB={_cb}"] = lambda c, d, v=_cb: _w(d) and d["CB"] == v
for _g in (1, 2, 4, 8):
    CLASSES[f"wide G={_g}"] = lambda c, d, v=_g: _w(d) and d["G"] == v
for _fin in (1, 2, 4):
    CLASSES[f"wide Fin={_fin}"] = lambda c, d, v=_fin: _w(d) and c["Fin"] == v
CLASSES["wide Fin=4 N=4"] = lambda c, d: _w(d) and c["Fin"] == 4 and c["N"] == 4
CLASSES["wide K=1"] = lambda c, d: _w(d) and c["K"] == 1
CLASSES["wide K=2"] = lambda c, d: _w(d) and c["K"] == 2
CLASSES["wide fused last"] = lambda c, d: _w(d) and d["fused_last"] == 1
CLASSES["wide fused last K=2"] = lambda c, d: _w(d) and d["fused_last"] == 1 and c["K"] == 2
CLASSES["wide assemble TM=32"] = lambda c, d: _w(d) and d["assemble_tm"] == 32
CLASSES["wide assemble 1<TM<32"] = lambda c, d: _w(d) and 1 < d["assemble_tm"] < 32
CLASSES["wide assemble TM=1"] = lambda c, d: _w(d) and d["assemble_tm"] == 1
for _fin in (1, 2, 4):
    CLASSES[f"wide assemble Fin={_fin}"] = (
        lambda c, d, v=_fin: _w(d) and d["assemble_tm"] > 0 and c["Fin"] == v)
CLASSES["wide sorted rows off"] = lambda c, d: _w(d) and c["K"] > 1 and d["sorted_rows_fwd"] == 0
for _name, _lo, _hi in (("TM=32", 32, 32), ("1<TM<32", 2, 31), ("TM=1", 1, 1)):
    CLASSES[f"wide sorted rows, assemble {_name}"] = (
        lambda c, d, lo=_lo, hi=_hi: _w(d) and d["sorted_rows_fwd"] == 1 and
        d["sorted_rows_bwd"] == 1 and d["fused_last"] == 0 and lo <= d["assemble_tm"] <= hi)
CLASSES["wide sorted rows, Fin=1 (no fused last)"] = (
    lambda c, d: _w(d) and d["sorted_rows_fwd"] == 1 and c["Fin"] == 1 and c["K"] <= 15)
for _fj in range(1, 9):
    CLASSES[f"dypass_small FJ={_fj}"] = (
        lambda c, d, v=_fj: _w(d) and d["dypass"] == 1 and c["Fin"] * c["K"] == v)
for _fk in (9, 16, 32):
    CLASSES[f"dypass_mfma FinK={_fk}"] = (
        lambda c, d, v=_fk: _w(d) and d["dypass"] == 2 and c["Fin"] * c["K"] == v)
for _kind, _code in (("small", 1), ("mfma", 2)):
    for _fo in (8, 16, 24, 32):
        CLASSES[f"dypass_{_kind} Fout={_fo}"] = (
            lambda c, d, k=_code, v=_fo: _w(d) and d["dypass"] == k and c["Fout"] == v)
for _n in (1, 2, 4, 8, 16, 64):
    CLASSES[f"dypass N={_n}"] = lambda c, d, v=_n: _w(d) and d["dypass"] > 0 and c["N"] == v
CLASSES["dypass_mfma N<32"] = lambda c, d: _w(d) and d["dypass"] == 2 and c["N"] < 32
CLASSES["dypass_mfma N=64"] = lambda c, d: _w(d) and d["dypass"] == 2 and c["N"] == 64
CLASSES["no dypass Fout=40"] = lambda c, d: _w(d) and d["dypass"] == 0 and c["Fout"] == 40
CLASSES["no dypass Fout=12"] = lambda c, d: _w(d) and d["dypass"] == 0 and c["Fout"] == 12
CLASSES["no dypass FinK=36"] = (
    lambda c, d: _w(d) and d["dypass"] == 0 and c["Fin"] * c["K"] == 36 and c["Fout"] == 8)
for _dp in (0, 1, 2):
    CLASSES[f"wide directed graph dypass={_dp}"] = (
        lambda c, d, v=_dp: _w(d) and c["graph"].startswith("dir") and d["dypass"] == v)
    CLASSES[f"wide sorted rows bwd dypass={_dp}"] = (
        lambda c, d, v=_dp: _w(d) and d["sorted_rows_bwd"] == 1 and d["dypass"] == v)
for _fin in (1, 3, 5, 8, 12, 20, 64, 65, 260):
    CLASSES[f"narrow Fin={_fin}"] = lambda c, d, v=_fin: not _w(d) and c["Fin"] == v
for _n in (1, 3, 9):
    CLASSES[f"narrow N={_n}"] = lambda c, d, v=_n: not _w(d) and c["N"] == v
CLASSES["narrow vec=1 lpr=64 (second f0 trip)"] = (
    lambda c, d: not _w(d) and d["vec"] == 1 and d["lpr"] == 64 and c["Fin"] > 64)
CLASSES["narrow vec=4 lpr=64 (second f0 trip)"] = (
    lambda c, d: not _w(d) and d["vec"] == 4 and d["lpr"] == 64 and c["Fin"] > 256)
CLASSES["narrow variant of a wide shape"] = (
    lambda c, d: not _w(d) and c["variant"] == "narrow")
CLASSES["narrow rows layout"] = lambda c, d: not _w(d) and c["layout"] == "rows"
CLASSES["narrow planes layout"] = lambda c, d: not _w(d) and c["layout"] == "planes"
CLASSES["narrow K=1"] = lambda c, d: not _w(d) and c["K"] == 1
CLASSES["narrow last step staged"] = lambda c, d: not _w(d) and d["last_staged"] == 1
CLASSES["narrow last step unstaged"] = lambda c, d: not _w(d) and d["last_staged"] == 0
CLASSES["narrow xcd_map=1"] = lambda c, d: not _w(d) and d["xcd_map"] == 1
CLASSES["narrow xcd_map=0"] = lambda c, d: not _w(d) and d["xcd_map"] == 0
CLASSES["narrow sorted rows off"] = (
    lambda c, d: not _w(d) and d["sorted_rows_fwd"] == 0 and d["sorted_rows_bwd"] == 0)
for _lay in ("rows", "planes"):
    CLASSES[f"narrow sorted rows, {_lay} layout"] = (
        lambda c, d, v=_lay: not _w(d) and d["sorted_rows_fwd"] == 1 and
        d["sorted_rows_bwd"] == 1 and c["layout"] == v)
CLASSES["narrow sorted rows Fin=20"] = (
    lambda c, d: not _w(d) and d["sorted_rows_fwd"] == 1 and c["Fin"] == 20)
CLASSES["narrow skewed graph, Fin=8 (gate off)"] = (
    lambda c, d: not _w(d) and c["graph"].startswith("hub") and c["Fin"] == 8 and
    d["sorted_rows_fwd"] == 0 and d["sorted_rows_bwd"] == 0)
CLASSES["narrow directed graph"] = lambda c, d: not _w(d) and c["graph"].startswith("dir")
CLASSES["narrow Fin%8==0 without the group kernels"] = (
    lambda c, d: not _w(d) and c["Fin"] % 8 == 0 and d["group_fwd"] == 0 and d["group_bwd"] == 0)


def classes_hit(pairs):
    """{class name: [case names]} over (case, dispatch dict) pairs."""
    hit = {name: [] for name in CLASSES}
    for c, d in pairs:
        for name, pred in CLASSES.items():
            if pred(c, d):
                hit[name].append(c["name"])
    return hit
