"""gconv_rnn.GConvRNNModel (lib/gconvRNN.py::Model, model_type='glstm') against
the float64 reference of tests/seq_model_ref.py: the loss as executed
((1/T) sum_t sum_n ce), every parameter gradient, sgd steps, per-variable
clipping with check_numerics, the two dropout seams, test_step / predict, and
two data-parallel ranks over gloo (grad_scale = 1).  Bar: 1e-5 normwise, the
scalar loss 1e-5 relative."""
import numpy as np
import pytest
import scipy.sparse

import dp_harness as DP
import gconv_rnn_dp_worker as Wk
import seq_model_ref as R
from conftest import case, load_golden
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
NAMES = ("Wx", "Wh", "b", "w", "bh")


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def graph(name):
    c = case(load_golden(f"golden_{name}.npz"))
    M = c["M"]
    Lt = scipy.sparse.csr_matrix((c["Lt_val"], c["Lt_col"], c["Lt_rowptr"]), shape=(M, M))
    return (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr(), M


def make(dev, gname="A", N=4, T=3, F=2, H=32, K=3, seed=11, **kw):
    from cnn_graph_amd.gconv_rnn import GConvRNNModel
    L, M = graph(gname)
    kw.setdefault("keep_prob", 1.0)
    kw.setdefault("learning_rate", 0.01)
    m = GConvRNNModel(L, N, T, F, num_hidden=H, K=K, device=dev, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, M, F, T)).astype(np.float32)
    labels = rng.integers(0, M, (N, T))
    labels[0, 0], labels[-1, -1] = 0, M - 1
    return m, x, labels


def params64(m):
    p = list(m.parameters().values())
    assert len(p) == 5
    return [a.detach().cpu().numpy().astype(np.float64) for a in p]


def grads64(m):
    return dict(zip(NAMES, (g.detach().cpu().numpy().astype(np.float64) for g in m.gradients().values())))


def lap_of(m):
    return (m.plan.rowptr, m.plan.col, m.plan.val.astype(np.float64))


def check_grads(got, ref, names=NAMES, what=""):
    for k in names:
        err = O.normwise_err(got[k].reshape(-1), ref[k].reshape(-1))
        print(f"{what} d{k}: {err:.2e}")
        assert err < TOL, (what, k, err)


@pytest.mark.parametrize("hconv", ["seq", "fused", "unfused"])
def test_loss_gradients_and_sgd_steps_vs_reference(dev, hconv):
    """Config A's graph (M 100), T 3, N 4, feat_in 2, H 32, K 3, keep 1, over
    the cell's one-launch layer and its two per-step paths."""
    m, x, labels = make(dev, hconv=hconv, optimizer="sgd")
    c = m.cells[0]
    assert c.seq == (hconv == "seq") and c.fused == (hconv != "unfused")
    p0, lap = params64(m), lap_of(m)
    xs = t(x, dev)
    loss, out = m.train_step(xs, labels, with_output=True)
    torch.cuda.synchronize()
    ref_loss, logits, _, st = R.model_forward(x, labels, p0, lap, m.K, m.H)
    ref_g = R.model_backward(st, p0, lap, m.K, m.H)
    rel = abs(float(loss.item()) - ref_loss) / ref_loss
    print(f"{hconv}: loss {float(loss.item()):.6f} ref {ref_loss:.6f} rel {rel:.2e}")
    assert rel < TOL
    assert tuple(out.shape) == (m.N, m.M, m.T)
    assert O.normwise_err(out.cpu().numpy(), R.pred_out(logits)) < TOL
    # the head bias: exact gradient 0, the plain sum is rounding noise
    got = grads64(m)
    check_grads(got, ref_g, NAMES[:4], hconv)
    assert abs(got["bh"][0]) <= TOL * np.abs(R.head_backward(st[0], p0[3], logits, st[2], 1 / m.T)[0]).sum()
    for _ in range(2):
        m.train_step(xs, labels)
    torch.cuda.synchronize()
    assert m.step_count == 3
    ref_p, _, _ = R.sgd_steps(x, labels, p0, lap, m.K, m.H, 0.01, 3)
    for k, a, b in zip(NAMES[:4], params64(m), ref_p):  # all but the head bias
        err = O.normwise_err(a.reshape(-1), b.reshape(-1))
        print(f"{hconv} after 3 sgd steps {k}: {err:.2e}")
        assert err < TOL, (k, err)
        assert not np.array_equal(a, p0[NAMES.index(k)])


def test_the_workload_tile(dev):
    """M 1024 (config E's graph), H 32, T 2, N 2."""
    m, x, labels = make(dev, "E", N=2, T=2, optimizer="sgd")
    assert m.cells[0].seq
    p0, lap = params64(m), lap_of(m)
    loss = m.train_step(t(x, dev), labels)
    torch.cuda.synchronize()
    ref_loss, _, _, st = R.model_forward(x, labels, p0, lap, m.K, m.H)
    assert abs(float(loss.item()) - ref_loss) < TOL * ref_loss
    check_grads(grads64(m), R.model_backward(st, p0, lap, m.K, m.H), NAMES[:4], "M 1024")


def test_clipping_and_check_numerics(dev):
    clip = 1e-3
    m, x, labels = make(dev, optimizer="sgd", max_grad_norm=clip)
    p0, lap = params64(m), lap_of(m)
    xs = t(x, dev)
    m.train_step(xs, labels)
    torch.cuda.synchronize()
    _, _, _, st = R.model_forward(x, labels, p0, lap, m.K, m.H)
    ref_g = R.model_backward(st, p0, lap, m.K, m.H)
    for k in NAMES[:4]:
        assert np.sqrt((ref_g[k] ** 2).sum()) > 10 * clip, k  # the clip binds
    got = grads64(m)
    check_grads(got, {k: R.clip_by_norm(ref_g[k], clip) for k in NAMES[:4]}, NAMES[:4], "clipped")
    for k in NAMES[:4]:
        assert abs(np.sqrt((got[k] ** 2).sum()) - clip) < 1e-5 * clip
    # a NaN in the exchanged gradient raises before the update
    flat, steps = m.flat.clone(), m.step_count
    clip_hook = m._after_exchange

    def poisoned(s):
        m.grad[3] = float("nan")
        clip_hook(s)
    m._after_exchange = poisoned
    with pytest.raises(FloatingPointError):
        m.train_step(xs, labels)
    assert torch.equal(m.flat, flat) and m.step_count == steps


def test_seams_are_bitwise_equal(dev):
    """keep 0.8, the same seed: the mask folded into the head (fused) against
    ops.dropout on the layer's output and its backward (unfused)."""
    res = {}
    for seam in ("fused", "unfused"):
        m, x, labels = make(dev, keep_prob=0.8, seam=seam, optimizer="adam")
        assert m.seam == seam
        xs, losses = t(x, dev), []
        for _ in range(2):
            losses.append(m.train_step(xs, labels).clone())
        torch.cuda.synchronize()
        res[seam] = (torch.stack(losses), m.grad.clone(), m.flat.clone())
    plain, x, labels = make(dev, keep_prob=1.0, optimizer="adam")
    assert not torch.equal(plain.train_step(t(x, dev), labels), res["fused"][0][0])  # the mask is on
    for a, b, what in zip(res["fused"], res["unfused"], ("loss", "gradients", "parameters")):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), what


def test_test_step_changes_nothing(dev):
    m, x, labels = make(dev, keep_prob=0.8, optimizer="rmsprop")
    xs = t(x, dev)
    m.train_step(xs, labels)  # non-trivial slots
    torch.cuda.synchronize()
    snap = [a.clone() for a in (m.flat, m.s1, m.s2)]
    steps = m.step_count
    loss, out = m.test_step(xs, labels, with_output=True)
    loss2 = m.test_step(xs, labels)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and tuple(out.shape) == (m.N, m.M, m.T)
    assert not torch.equal(loss, loss2)  # the reference drops at test time too: a new mask
    assert m.step_count == steps
    for a, b in zip(snap, (m.flat, m.s1, m.s2)):
        assert torch.equal(a, b)
    bad = labels.copy()
    bad[1, 1] = m.M
    with pytest.raises(ValueError):
        m.test_step(xs, bad)


def test_predict_pads_the_last_batch(dev):
    m, x, labels = make(dev, keep_prob=0.8)
    N, M = m.N, m.M
    size = 2 * N + 1
    data = np.random.default_rng(5).standard_normal((size, M, m.F, m.T)).astype(np.float32)
    flat = m.flat.clone()
    preds = m.predict(data)
    torch.cuda.synchronize()
    assert tuple(preds.shape) == (size, M, m.T)  # the padded rows are not returned
    assert torch.equal(m.predict(data), preds) and torch.equal(m.flat, flat)  # no dropout, no update
    for b0 in range(0, size, N):
        batch = np.zeros((N, M, m.F, m.T), np.float32)
        n = min(N, size - b0)
        batch[:n] = data[b0:b0 + n]
        out = m.forward(t(batch, dev), dropout=False)
        assert torch.equal(out[:n], preds[b0:b0 + n]), b0
    p0, lap = params64(m), lap_of(m)
    _, logits, _, _ = R.model_forward(data[:N], labels, p0, lap, m.K, m.H)
    assert O.normwise_err(preds[:N].cpu().numpy(), R.pred_out(logits)) < TOL
    assert not torch.equal(m.predict(data, reference_dropout=True), preds)


@pytest.mark.timeout(300)
def test_world2_matches_the_whole_batch(dev, tmp_path):
    """Two ranks over gloo, keep 1, sgd: the replicas are bitwise equal after
    every step and within 1e-5 of one process on the whole batch -- which holds
    only with grad_scale = 1 (the loss sums over the batch, so the shards'
    gradients add; 1/world would halve every step)."""
    d = DP.launch_world2("gconv_rnn_dp_worker", tmp_path / "gconv_rnn_dp.npz", 240)
    assert np.array_equal(d["P"], d["P_r1"]), "replicas diverged"
    L, x, labels = Wk.problem()
    P, losses = Wk.run(L, x, labels, dev, None)
    assert np.all(np.isfinite(losses))
    # the shards' losses add up to the whole batch's (a sum over the batch)
    assert np.all(np.abs(d["loss_sum"] - losses) < 1e-5 * np.abs(losses))
    DP.assert_tracks_full_batch(d["P"], P, Wk.STEPS, tol=TOL)
