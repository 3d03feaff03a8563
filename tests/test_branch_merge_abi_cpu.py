"""cg_branch_merge_* / cg_concat_drop_* without a GPU: the header's new symbols
are exported, and every refusal the header lists returns CG_ERR_ARG with a
cg_last_error text -- before any device work, so the pointers here are never
memory.  (The backward sums inside one workgroup: the calls take no workspace,
so there is no short-workspace refusal to test.)"""
import ctypes

import pytest

from cnn_graph_amd import _lib

NEW = ["cg_branch_merge_forward", "cg_branch_merge_backward", "cg_concat_drop_forward",
       "cg_concat_drop_backward"]


@pytest.fixture(scope="module")
def h(built_lib):
    return _lib.lib()


def arr(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def ints(*v):
    return (ctypes.c_int32 * len(v))(*v)


def seeds(n):
    return (ctypes.c_uint64 * n)(*range(1, n + 1))


def refused(h, status, text):
    assert status == _lib.CG_ERR_ARG, status
    msg = h.cg_last_error().decode()
    assert text in msg, msg


# distinct fake device addresses, 256 bytes apart
Y, W, DY, DW = ([256 * (10 * k + b + 1) for b in range(5)] for k in range(4))
OUT, DOUT = 256 * 100, 256 * 101


def test_symbols_exported_and_version(h):
    syms = _lib.header_symbols()
    for name in NEW:
        assert name in syms and name in _lib._SIGNATURES and hasattr(h, name)
    assert "cg_branch_merge_workspace_bytes" not in syms  # no workspace: the sum stays in one workgroup
    assert h.cg_version() == 301


def test_merge_forward_refusals(h):
    f = h.cg_branch_merge_forward
    for B in (0, 5, -1):
        refused(h, f(B, 2, 3, 2, arr(*Y[:4]), arr(*W[:4]), OUT, None), "bad sizes")
    for N, M, F in ((0, 3, 2), (2, 0, 2), (2, 3, 0), (-1, 3, 2)):
        refused(h, f(2, N, M, F, arr(*Y[:2]), arr(*W[:2]), OUT, None), "bad sizes")
    refused(h, f(2, 2, 3, 2, None, arr(*W[:2]), OUT, None), "null")
    refused(h, f(2, 2, 3, 2, arr(*Y[:2]), None, OUT, None), "null")
    refused(h, f(2, 2, 3, 2, arr(*Y[:2]), arr(*W[:2]), None, None), "null")
    refused(h, f(2, 2, 3, 2, arr(Y[0], None), arr(*W[:2]), OUT, None), "null")
    refused(h, f(2, 2, 3, 2, arr(*Y[:2]), arr(None, W[1]), OUT, None), "null")
    refused(h, f(2, 2, 3, 2, arr(Y[0], OUT), arr(*W[:2]), OUT, None), "alias")
    refused(h, f(2, 2, 3, 2, arr(*Y[:2]), arr(OUT, W[1]), OUT, None), "alias")


def test_merge_backward_refusals(h):
    f = h.cg_branch_merge_backward

    def call(B=2, N=2, M=3, F=2, dout=DOUT, y=Y, w=W, dy=DY, dw=DW):
        a = lambda v: None if v is None else arr(*v[:max(B, 1)][:4])  # noqa: E731
        return f(B, N, M, F, dout, a(y), a(w), a(dy), a(dw), 0, None)

    for B in (0, 5):
        refused(h, call(B=B), "bad sizes")
    for kw in (dict(N=0), dict(M=0), dict(F=-2)):
        refused(h, call(**kw), "bad sizes")
    refused(h, call(dout=None), "null")
    refused(h, call(y=None), "null")
    refused(h, call(w=None), "null")
    refused(h, call(y=[Y[0], None]), "null")
    refused(h, call(w=[None, W[1]]), "null")
    # nothing to compute: both output arrays absent, or every entry null
    refused(h, call(dy=None, dw=None), "every dy and dw entry is null")
    refused(h, call(dy=[None, None], dw=[None, None]), "every dy and dw entry is null")
    # an output that is an input, and two outputs in one buffer
    refused(h, call(dy=[DOUT, DY[1]]), "alias")
    refused(h, call(dy=[Y[1], DY[1]]), "alias")
    refused(h, call(dw=[DW[0], W[0]]), "alias")
    refused(h, call(dy=[DY[0], DY[0]]), "distinct")
    refused(h, call(dy=[DY[0], DY[1]], dw=[DY[1], DW[1]]), "distinct")


def test_concat_drop_refusals(h):
    fwd, bwd = h.cg_concat_drop_forward, h.cg_concat_drop_backward
    f32 = ctypes.c_float
    for name, f in (("forward", fwd), ("backward", bwd)):
        def call(B=3, N=2, M=3, H=(4, 8, 4), hs=Y, keep=0.8, sd=True, wide=OUT):
            Hc = None if H is None else ints(*H)
            branches = None if hs is None else arr(*hs[:4])
            sc = seeds(4) if sd else None
            if name == "forward":  # (B, N, M, H, h, keep, seed, out, stream)
                return f(B, N, M, Hc, branches, f32(keep), sc, wide, None)
            return f(B, N, M, Hc, wide, f32(keep), sc, branches, None)  # (..., dx, keep, seed, dh, stream)

        for B in (0, 5):
            refused(h, call(B=B, H=(4, 4, 4, 4)), "bad sizes")
        refused(h, call(N=0), "bad sizes")
        refused(h, call(M=-1), "bad sizes")
        refused(h, call(H=(4, 0, 4)), "H[1]")
        refused(h, call(H=None), "null")
        refused(h, call(hs=None), "null")
        refused(h, call(sd=False), "null")
        refused(h, call(wide=None), "null")
        refused(h, call(hs=[Y[0], None, Y[2]]), "null")
        for keep in (0.0, 1.5, -0.1, float("nan")):
            refused(h, call(keep=keep), "keep")
        refused(h, call(hs=[Y[0], OUT, Y[2]]), "alias")
        refused(h, call(hs=[Y[0], Y[1], Y[0]]), "distinct")
