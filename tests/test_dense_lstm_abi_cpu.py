"""cg_dlstm_* and cg_class_xent_sum without a GPU: the header's new symbols are
exported, and every refusal the header lists returns CG_ERR_ARG or
CG_ERR_UNSUPPORTED with a cg_last_error text -- before any device work, so the
pointers here are never memory.  (cg_dlstm_workspace_bytes reports 0 for both
directions, so the sequence entries have no short-workspace refusal to test;
cg_class_xent_sum has one.)"""
import ctypes

import pytest

from cnn_graph_amd import _lib

NEW = ["cg_dlstm_supported", "cg_dlstm_workspace_bytes", "cg_dlstm_seq_forward",
       "cg_dlstm_seq_backward", "cg_class_xent_sum"]
f32 = ctypes.c_float
# distinct fake device addresses, 256 bytes apart (16-byte aligned)
GX, WH, B, HS, CS, ACT, DHS, DPRE, WS = (256 * (k + 1) for k in range(9))
X, LAB, LOSS, DX = (256 * (k + 20) for k in range(4))


@pytest.fixture(scope="module")
def h(built_lib):
    return _lib.lib()


def refused(h, status, text, code=_lib.CG_ERR_ARG):
    assert status == code, status
    msg = h.cg_last_error().decode()
    assert text in msg, msg


def test_symbols_exported_and_version(h):
    syms = _lib.header_symbols()
    for name in NEW:
        assert name in syms and name in _lib._SIGNATURES and hasattr(h, name)
    assert h.cg_version() == 301


def test_library_reads_no_environment_variable(h):
    with open(_lib.LIB_PATH, "rb") as f:
        assert b"getenv" not in f.read()


def test_supported_range(h):
    ok = ctypes.c_int32(-1)
    for H in range(1, 161):
        assert h.cg_dlstm_supported(H, ctypes.byref(ok)) == _lib.CG_OK
        assert ok.value == int(H % 16 == 0 and 16 <= H <= 128), H
    for H in (0, -16):
        assert h.cg_dlstm_supported(H, ctypes.byref(ok)) == _lib.CG_OK and ok.value == 0
    refused(h, h.cg_dlstm_supported(32, None), "null")


def test_workspace_bytes(h):
    fb, bb = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert h.cg_dlstm_workspace_bytes(3, 5, 48, ctypes.byref(fb), ctypes.byref(bb)) == _lib.CG_OK
    assert fb.value == 0 and bb.value == 0  # nothing is handed between workgroups
    refused(h, h.cg_dlstm_workspace_bytes(3, 5, 48, None, ctypes.byref(bb)), "null")
    refused(h, h.cg_dlstm_workspace_bytes(3, 5, 48, ctypes.byref(fb), None), "null")
    for T, N, H in ((0, 5, 48), (3, 0, 48), (3, 5, 0), (-1, 5, 48)):
        refused(h, h.cg_dlstm_workspace_bytes(T, N, H, ctypes.byref(fb), ctypes.byref(bb)), "bad sizes")
    for H in (8, 24, 144, 129):
        refused(h, h.cg_dlstm_workspace_bytes(3, 5, H, ctypes.byref(fb), ctypes.byref(bb)), "H =",
                _lib.CG_ERR_UNSUPPORTED)


def test_forward_refusals(h):
    def call(T=3, N=5, H=48, gx=GX, Wh=WH, b=B, hs=HS, cs=CS, act=ACT, ws=None, nb=0):
        return h.cg_dlstm_seq_forward(T, N, H, gx, Wh, b, f32(1.0), hs, cs, act, ws, nb, None)

    for kw in (dict(gx=None), dict(Wh=None), dict(b=None), dict(hs=None), dict(cs=None)):
        refused(h, call(**kw), "null")
    for kw in (dict(T=0), dict(N=0), dict(H=0), dict(T=-2), dict(N=-1)):
        refused(h, call(**kw), "bad sizes")
    for H in (8, 24, 40, 144, 256):
        refused(h, call(H=H), "H =", _lib.CG_ERR_UNSUPPORTED)
    for kw in (dict(gx=GX + 4), dict(hs=HS + 8), dict(cs=CS + 4), dict(act=ACT + 12)):
        refused(h, call(**kw), "aligned")
    for kw in (dict(hs=GX), dict(cs=WH), dict(act=GX), dict(act=B)):
        refused(h, call(**kw), "alias")
    for kw in (dict(cs=HS), dict(act=HS), dict(act=CS)):
        refused(h, call(**kw), "distinct")


def test_backward_refusals(h):
    def call(T=3, N=5, H=48, dhs=DHS, act=ACT, cs=CS, Wh=WH, dpre=DPRE, ws=None, nb=0):
        return h.cg_dlstm_seq_backward(T, N, H, dhs, act, cs, Wh, f32(1.0), dpre, ws, nb, None)

    for kw in (dict(dhs=None), dict(act=None), dict(cs=None), dict(Wh=None), dict(dpre=None)):
        refused(h, call(**kw), "null")
    for kw in (dict(T=0), dict(N=0), dict(H=0), dict(H=-16)):
        refused(h, call(**kw), "bad sizes")
    for H in (8, 24, 144):
        refused(h, call(H=H), "H =", _lib.CG_ERR_UNSUPPORTED)
    for kw in (dict(dhs=DHS + 4), dict(act=ACT + 4), dict(cs=CS + 8), dict(dpre=DPRE + 4)):
        refused(h, call(**kw), "aligned")
    refused(h, call(dpre=ACT), "alias")  # dpre aliasing act
    for kw in (dict(dpre=DHS), dict(dpre=CS), dict(dpre=WH)):
        refused(h, call(**kw), "alias")


def test_class_xent_sum_refusals_mirror_the_ema_entry(h):
    need = ctypes.c_size_t()
    assert h.cg_class_xent_workspace_bytes(6, 7, 0, ctypes.byref(need)) == _lib.CG_OK

    def sum_(x=X, lab=LAB, N=6, C=7, loss=LOSS, dx=DX, ws=WS, nb=None):
        return h.cg_class_xent_sum(x, lab, N, C, f32(0.5), loss, dx, None, None, None, None, ws,
                                   need.value if nb is None else nb, None)

    def ema(x=X, lab=LAB, N=6, C=7, loss=LOSS, dx=DX, ws=WS, nb=None):
        return h.cg_class_xent_ema(x, lab, N, C, None, 0, 0, f32(0.0), loss, dx, None, f32(0.9), None,
                                   None, None, ws, need.value if nb is None else nb, None)

    cases = [(dict(x=None), "null"), (dict(lab=None), "null"), (dict(loss=None), "null"),
             (dict(N=0), "bad sizes"), (dict(C=0), "bad sizes"), (dict(N=-1), "bad sizes"),
             (dict(N=1 << 16, C=1 << 15), "2^31"), (dict(dx=X), "alias"),
             (dict(ws=None), "workspace too small"), (dict(nb=need.value - 1), "workspace too small")]
    for kw, text in cases:
        refused(h, sum_(**kw), text)
        refused(h, ema(**kw), text)
