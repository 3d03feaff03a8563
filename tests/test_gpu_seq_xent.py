"""cg_seq_xent_head (the gconvRNN per-step head + vertex softmax cross-entropy,
one pass over hs [T, N, M, H]) against the float64 reference of
tests/seq_model_ref.py.  Bars: 1e-5 normwise on logits, ce, dhs and dw, 1e-5
relative on the scalar loss; the dropout fold and repeated calls bitwise."""
import functools

import numpy as np
import pytest

import seq_model_ref as R
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
# (T, N, M, H): degenerate, scalar path, M not a tile multiple, H = 4 (one lane per row),
# the workload's tile, one past a 1024 tile at the widest common H, the widest supported H
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (3, 2, 100, 32), (2, 1, 976, 4), (2, 2, 1024, 32),
          (1, 2, 1030, 128), (1, 1, 7, 256)]
FOLD_SHAPES = [(3, 2, 100, 32), (1, 2, 1030, 128)]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def f64(x):
    return x.detach().cpu().numpy().astype(np.float64)


def labelings(T, N, M, rng):
    """Label sets [T, N] that between them hold vertex 0 and vertex M - 1."""
    lab = rng.integers(0, M, (T, N))
    if T * N == 1:
        return [np.zeros((1, 1), np.int64), np.full((1, 1), M - 1, np.int64)]
    lab.reshape(-1)[0], lab.reshape(-1)[-1] = 0, M - 1
    return [lab]


@functools.lru_cache(maxsize=None)
def problem(shape, wscale=1.0):
    """Inputs (float32 values) and the float64 results, computed once per shape."""
    T, N, M, H = shape
    rng = np.random.default_rng(1000 + M + H)
    hs = rng.standard_normal((T, N, M, H)).astype(np.float32)
    w = (wscale * rng.standard_normal(H)).astype(np.float32)
    b = rng.standard_normal(1).astype(np.float32)
    scale = 1.0 / T
    out = []
    for lab in labelings(T, N, M, rng):
        logits, ce, loss = R.head_forward(hs, w, b, lab, scale)
        dlogit, dhs, dw, db = R.head_backward(hs, w, logits, lab, scale)
        out.append(dict(lab=lab, logits=logits, ce=ce, loss=loss, dlogit=dlogit, dhs=dhs, dw=dw))
    return hs, w, b, scale, out


def call(dev, hs, w, b, lab, scale, **kw):
    from cnn_graph_amd import ops
    r = ops.seq_xent_call(hs if torch.is_tensor(hs) else t(hs, dev), t(w, dev), t(b, dev),
                          t(lab, dev, np.int32), loss_scale=scale, want_logits=True, want_ce=True, **kw)
    torch.cuda.synchronize()
    return r


def check(shape, r, ref, scale):
    T, N, M, H = shape
    errs = dict(logits=O.normwise_err(f64(r.logits), R.pred_out(ref["logits"])),
                ce=O.normwise_err(f64(r.ce), ref["ce"]), dhs=O.normwise_err(f64(r.dhs), ref["dhs"]),
                dw=O.normwise_err(f64(r.dw), ref["dw"]))
    loss = float(r.loss.item())
    rel = abs(loss - ref["loss"]) / abs(ref["loss"]) if ref["loss"] else abs(loss)
    db, bound = abs(float(r.db.item())), TOL * np.abs(ref["dlogit"]).sum()
    print(f"{shape}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          f" loss {rel:.2e} |db| {db:.2e} (bound {bound:.2e})")
    assert np.isfinite(loss) and all(bool(torch.isfinite(x).all()) for x in (r.logits, r.ce, r.dhs, r.dw))
    for k, v in errs.items():
        assert v < TOL, (shape, k, v)
    assert rel < TOL, (shape, loss, ref["loss"])
    assert db <= bound, (shape, db, bound)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_vs_float64(dev, shape):
    hs, w, b, scale, refs = problem(shape)
    for ref in refs:
        r = call(dev, hs, w, b, ref["lab"], scale)
        assert tuple(r.logits.shape) == (shape[1], shape[2], shape[0])
        check(shape, r, ref, scale)
        if shape == (1, 1, 1, 1):  # one vertex: softmax = 1, loss and every gradient exactly 0
            assert float(r.loss.item()) == 0.0 and float(r.ce.item()) == 0.0
            assert float(r.dhs.abs().max()) == 0.0 and float(r.dw.abs().max()) == 0.0
            assert float(r.db.item()) == 0.0


def test_wide_logits_are_stable(dev):
    """w scaled so the logits span about +-200: exp(logit) overflows float32
    unless the max is subtracted first."""
    shape = (2, 2, 1024, 32)
    span = np.abs(problem(shape)[4][0]["logits"]).max()
    hs, w, b, scale, refs = problem(shape, float(np.float32(200.0 / span)))
    ref = refs[0]
    # exp overflows float32 from 88.7 on
    assert ref["logits"].max() > 150 and ref["logits"].min() < -150
    check(shape, call(dev, hs, w, b, ref["lab"], scale), ref, scale)


def test_h_past_256_is_unsupported(dev):
    from cnn_graph_amd import _lib
    hs = torch.zeros((1, 1, 2, 257), device=dev)
    with pytest.raises(_lib.CGError) as e:
        call(dev, hs, np.zeros(257), np.zeros(1), np.zeros((1, 1)), 1.0)
    assert e.value.code == _lib.CG_ERR_UNSUPPORTED and "256" in str(e.value)


@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dropout_fold_is_bitwise(dev, shape):
    """head(hs, keep, seed) == head(ops.dropout(hs), keep = 1) bit for bit, and
    its dhs is the dropout backward of the unmasked call's dhs (keep 0.8, a
    non-zero offset into the mask stream)."""
    from cnn_graph_amd import _lib, ops
    hs, w, b, scale, refs = problem(shape)
    lab = refs[0]["lab"]
    keep, seed, offset = 0.8, 0x1234567890ABCDEF, 12345
    s = (seed + ops.DROP_WEYL * offset) & ((1 << 64) - 1)
    hs_d = t(hs, dev)
    hd = ops.dropout(hs_d, keep, seed, offset=offset)
    assert not torch.equal(hd, hs_d) and float((hd == 0).float().mean()) > 0.1
    fused = call(dev, hs_d, w, b, lab, scale, keep=keep, seed=s)
    plain = call(dev, hd, w, b, lab, scale)
    for k in ("logits", "ce", "loss", "dw", "db"):
        assert torch.equal(getattr(fused, k), getattr(plain, k)), k
    dhs = torch.empty_like(plain.dhs)
    _lib.call("cg_dropout_backward", plain.dhs.data_ptr(), dhs.numel(), keep, s, dhs.data_ptr(),
              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(fused.dhs, dhs)
    # and the masked call is itself right: against float64 on the dropped values
    logits, ce, loss = R.head_forward(f64(hd), w, b, lab, scale)
    assert O.normwise_err(f64(fused.ce), ce) < TOL and abs(float(fused.loss.item()) - loss) < TOL * loss


def test_repeatable_and_forward_only(dev):
    shape = (2, 2, 1024, 32)
    hs, w, b, scale, refs = problem(shape)
    lab = refs[0]["lab"]
    a, c = call(dev, hs, w, b, lab, scale), call(dev, hs, w, b, lab, scale)
    for k in ("logits", "ce", "loss", "dhs", "dw", "db"):
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    fwd = call(dev, hs, w, b, lab, scale, need_grad=False)
    assert fwd.dhs is None and fwd.dw is None
    assert torch.equal(fwd.loss, a.loss) and torch.equal(fwd.logits, a.logits)


def test_out_of_range_label_poisons_its_pair_only(dev):
    shape = (3, 2, 100, 32)
    hs, w, b, scale, refs = problem(shape)
    good = call(dev, hs, w, b, refs[0]["lab"], scale)
    for bad_value in (100, -1):
        lab = refs[0]["lab"].copy()
        lab[1, 1] = bad_value
        r = call(dev, hs, w, b, lab, scale)
        nan_ce = torch.isnan(r.ce)
        assert bool(nan_ce[1, 1]) and int(nan_ce.sum()) == 1
        assert torch.equal(r.ce[~nan_ce], good.ce[~nan_ce])
        assert bool(torch.isnan(r.dhs[1, 1]).all())
        rest = torch.ones_like(nan_ce)
        rest[1, 1] = False
        assert torch.equal(r.dhs[rest], good.dhs[rest])
        assert bool(torch.isnan(r.loss).all()) and bool(torch.isnan(r.dw).all())
        assert torch.equal(r.logits, good.logits)


def test_autograd_op_and_host_label_check(dev):
    """ops.seq_xent_head: the gradients of the launch handed out times the
    incoming scalar; no grad -> the forward-only launch; host labels validated."""
    from cnn_graph_amd import ops
    shape = (3, 2, 100, 32)
    hs, w, b, scale, refs = problem(shape)
    ref = refs[0]
    hs_d, w_d, b_d = (t(a, dev).requires_grad_() for a in (hs, w.reshape(-1, 1), b))
    loss, logits = ops.seq_xent_head(hs_d, w_d, b_d, ref["lab"], loss_scale=scale, want_logits=True)
    (2.0 * loss).sum().backward()
    torch.cuda.synchronize()
    assert not logits.requires_grad and tuple(w_d.grad.shape) == (32, 1)
    assert O.normwise_err(f64(hs_d.grad), 2 * ref["dhs"]) < TOL
    assert O.normwise_err(f64(w_d.grad).reshape(-1), 2 * ref["dw"]) < TOL
    with torch.no_grad():
        loss2 = ops.seq_xent_head(hs_d, w_d, b_d, ref["lab"], loss_scale=scale)
    assert torch.equal(loss2, loss.detach())
    bad = ref["lab"].copy()
    bad[0, 0] = 100
    with pytest.raises(ValueError):
        ops.seq_xent_head(hs_d, w_d, b_d, bad, loss_scale=scale)
