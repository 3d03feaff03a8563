"""The four cg_fres_* entry points refuse the same bad arguments the same way,
and cg_fres_workspace_bytes is exactly the size each of them asks for.  No GPU:
every call here fails its argument checks before any device work, and the
pointers are never memory (tests/test_gpu_fres_bits.py makes the calls that
pass)."""
import ctypes

import pytest

from cnn_graph_amd import _lib

N_, M_, FIN, FOUT = 3, 100, 10, 32
# fake, 16-byte aligned, distinct: never dereferenced
B, W, X, RES, XHAT, Y, WS, DY, DZ, DX, DW = (ctypes.c_void_p(4096 * k) for k in range(1, 12))
# (C entry, keep_prob or None for the plain entries)
ENTRIES = [("cg_fres_forward", None), ("cg_fres_backward", None), ("cg_fres_forward_drop", 0.8),
           ("cg_fres_forward_drop", 1.0), ("cg_fres_backward_drop", 0.8), ("cg_fres_backward_drop", 1.0)]
IDS = [f"{e}{'' if k is None else f'@{k}'}" for e, k in ENTRIES]


@pytest.fixture(scope="module")
def sizes(built_lib):
    h = _lib.lib()
    nb, fb, bb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert h.cg_gft_workspace_bytes(M_, ctypes.byref(nb)) == _lib.CG_OK
    assert h.cg_fres_workspace_bytes(N_, M_, FIN, FOUT, ctypes.byref(fb), ctypes.byref(bb)) == _lib.CG_OK
    return nb.value, fb.value, bb.value


def call(entry, keep, sizes, **kw):
    """One call of ``entry`` with good arguments except the overrides in kw;
    returns (status, message)."""
    h = _lib.lib()
    nb, fw, bw = sizes
    forward = "forward" in entry
    a = dict(N=N_, M=M_, Fin=FIN, Fout=FOUT, B=B, nb=nb, W=W, x=X, res=RES, xhat=XHAT, y=Y, dy=DY, dz=DZ,
             dx=DX, dW=DW, ws=WS, n=fw if forward else bw, act=_lib.CG_ACT_RELU, keep=keep)
    a.update(kw)
    drop = () if keep is None else (ctypes.c_float(a["keep"]), 5)
    if forward:
        st = getattr(h, entry)(a["N"], a["M"], a["Fin"], a["Fout"], a["B"], a["nb"], a["W"], a["x"], *drop,
                               a["res"], a["act"], a["xhat"], a["y"], a["ws"], a["n"], None)
    else:
        acc = (0,) if keep is None else ()
        st = getattr(h, entry)(a["N"], a["M"], a["Fin"], a["Fout"], a["B"], a["nb"], a["W"], a["xhat"],
                               a["dy"], a["y"], a["act"], *drop, a["dz"], a["dx"], *acc, a["dW"], a["ws"],
                               a["n"], None)
    return st, h.cg_last_error().decode()


# (row, overrides from (basis bytes, workspace bytes), message substring)
ROWS = [
    ("short basis", lambda nb, need: dict(nb=nb - 1), "basis"),
    ("short workspace", lambda nb, need: dict(n=need - 1), "workspace"),
    ("N*M*C >= 2^31", lambda nb, need: dict(N=1 << 20, Fout=128, n=1 << 40), "2^31"),
    ("unknown act", lambda nb, need: dict(act=_lib.CG_ACT_TANH), "act must be"),
    # the backward reads y as the ReLU mask; the forward writes it
    ("relu without y", lambda nb, need: dict(y=None), {"backward": "needs y", "forward": "null W / x / xhat / y"}),
    ("null W", lambda nb, need: dict(W=None), "null W"),
]


@pytest.mark.parametrize("entry,keep", ENTRIES, ids=IDS)
@pytest.mark.parametrize("row,over,text", ROWS, ids=[r[0] for r in ROWS])
def test_same_refusals(sizes, entry, keep, row, over, text):
    nb, fw, bw = sizes
    direction = "forward" if "forward" in entry else "backward"
    st, msg = call(entry, keep, sizes, **over(nb, fw if direction == "forward" else bw))
    assert st == _lib.CG_ERR_ARG, (row, st, msg)
    assert (text if isinstance(text, str) else text[direction]) in msg, (row, msg)
    assert msg.startswith(entry[3:]) and msg[len(entry) - 3] in ": ", msg  # the entry's own name


@pytest.mark.parametrize("entry", ["cg_fres_forward_drop", "cg_fres_backward_drop"])
def test_drop_pre_checks(sizes, entry):
    for keep in (0.0, 1.5):
        st, msg = call(entry, keep, sizes)
        assert st == _lib.CG_ERR_ARG and "keep_prob" in msg, (keep, msg)
    if "backward" in entry:
        for keep in (0.8, 1.0):
            st, msg = call(entry, keep, sizes, dx=None)
            assert st == _lib.CG_ERR_ARG and "dx is required" in msg, (keep, msg)
        # keep_prob is judged first, then dx, then everything else
        assert "keep_prob" in call(entry, 0.0, sizes, dx=None, W=None)[1]
        assert "dx is required" in call(entry, 0.8, sizes, dx=None, W=None)[1]


@pytest.mark.parametrize("entry,keep", ENTRIES, ids=IDS)
def test_workspace_bytes_is_what_each_entry_asks_for(sizes, entry, keep):
    """One byte short is refused, and the size the refusal asks for is the
    reported one (dx given, so the backward counts dxhat)."""
    nb, fw, bw = sizes
    need = fw if "forward" in entry else bw
    for n in (need - 1, 0):
        st, msg = call(entry, keep, sizes, n=n)
        assert st == _lib.CG_ERR_ARG and msg.endswith(f"workspace too small: {n} < {need}"), msg


def test_backward_without_dx_needs_no_dxhat(sizes):
    nb, fw, bw = sizes
    st, msg = call("cg_fres_backward", None, sizes, dx=None, n=0)
    assert st == _lib.CG_ERR_ARG and msg.endswith(f"workspace too small: 0 < {fw}"), msg  # ghat alone
