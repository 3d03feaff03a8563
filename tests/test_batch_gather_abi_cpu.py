"""cg_batch_gather refuses bad arguments before any device work.  No GPU: every
call here fails its argument checks, and the pointers are never memory
(tests/test_gpu_batch_gather.py makes the calls that pass)."""
import ctypes

import pytest

from cnn_graph_amd import _lib

# fake, 16-byte aligned, distinct: never dereferenced
DATA, LABELS, IDX, X, Y = (ctypes.c_void_p(4096 * k) for k in range(1, 6))
GOOD = dict(data=DATA, labels=LABELS, idx=IDX, N=4, S=10, row=32, lrow=8, x=X, y=Y)


def call(**kw):
    a = dict(GOOD, **kw)
    h = _lib.lib()
    st = h.cg_batch_gather(a["data"], a["labels"], a["idx"], a["N"], a["S"], a["row"], a["lrow"],
                           a["x"], a["y"], None)
    return st, h.cg_last_error().decode()


# (row, overrides, message substring)
ROWS = [
    ("null data", dict(data=None), "null"),
    ("null idx", dict(idx=None), "null"),
    ("null x", dict(x=None), "null"),
    ("N < 1", dict(N=0), "N=0"),
    ("S < 1", dict(S=0), "S=0"),
    ("row < 1", dict(row=0), "row=0"),
    ("labels without y", dict(y=None), "both or neither"),
    ("y without labels", dict(labels=None), "both or neither"),
    ("lrow < 1", dict(lrow=0), "lrow"),
    ("N*row = 2^31", dict(N=1 << 11, row=1 << 20), "2^31"),
    ("N*lrow = 2^31", dict(N=1 << 11, lrow=1 << 20), "2^31"),
    ("row past int64 / N", dict(N=3, row=(1 << 62)), "2^31"),
    ("x is data", dict(x=DATA), "alias"),
    ("x is labels", dict(x=LABELS), "alias"),
    ("y is data", dict(y=DATA), "alias"),
    ("y is labels", dict(y=LABELS), "alias"),
    ("x is y", dict(y=X), "distinct"),
]


def test_symbol_is_declared_bound_and_exported(built_lib):
    assert "cg_batch_gather" in _lib.header_symbols()
    assert "cg_batch_gather" in _lib._SIGNATURES and hasattr(_lib.lib(), "cg_batch_gather")
    assert _lib.lib().cg_version() == 301  # additive: the version stays


@pytest.mark.parametrize("row,over,text", ROWS, ids=[r[0] for r in ROWS])
def test_refusals(built_lib, row, over, text):
    st, msg = call(**over)
    assert st == _lib.CG_ERR_ARG, (row, st, msg)
    assert text in msg, (row, msg)
    assert msg.startswith("batch_gather") and msg[len("batch_gather")] in ": ", msg  # the entry's own name


def test_data_only_refuses_the_same_way(built_lib):
    """labels and y both NULL is a valid form: lrow is then ignored, and the
    other checks still hold."""
    only = dict(labels=None, y=None, lrow=0)
    for over, text in ((dict(x=None), "null"), (dict(N=0), "N=0"), (dict(x=DATA), "alias"),
                       (dict(N=1 << 11, row=1 << 20), "2^31")):
        st, msg = call(**only, **over)
        assert st == _lib.CG_ERR_ARG and text in msg, (over, st, msg)


def test_largest_batch_passes_the_bound(built_lib):
    """N * row = 2^31 - 1 is inside the bound: the next refusal in line answers
    (x aliasing data), not the size check."""
    st, msg = call(N=1, row=(1 << 31) - 1, x=DATA)
    assert st == _lib.CG_ERR_ARG and "alias" in msg, msg
