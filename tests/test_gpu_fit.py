"""FlatTrainer.fit (GraphModel.fit, lib/graph_model.py:124-197) against the loop
it replaces: ``fit_schedule`` on the host, ``train_step(data[idx], labels[idx])``
with torch indexing, ``evaluate`` at the same steps.

Criterion.  The manual loop is run twice from one seed first.  Where those two
runs agree bit for bit (the model's step is repeatable), ``fit`` must equal
them bit for bit: the gather moves bits and the step is the same code.  Where
they do not, ``fit`` is held to the spread the two manual runs show: its
normwise distance from the first run may not exceed the distance between the
two runs, per compared quantity.  (On the MI355X both models' manual loops were
bitwise repeatable, so the bitwise branch is the one that ran.)  Compared: the flat parameter buffer, both
optimizer slots, ``step_count``, the loss average, ``accuracies`` and ``losses``.

Shapes: M = 16, S = 10 samples in batches of N = 4 (leftovers carry over: 2
epochs are 5 steps and one refill falls inside a batch), 6 validation samples
(a ragged last batch), ``eval_frequency = 2`` (evaluations at steps 2, 4, 5)."""
import functools

import numpy as np
import pytest

import glstm_gconv_ref as GR
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

M, S, SV, N, EPOCHS, EVERY, SEED = 16, 10, 6, 4, 2, 2, 21
KINDS = ["resgnn", "glstm_gconv_dropout"]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def laplacian():
    """One Laplacian object for the module: plan_for caches by the object and
    drops the plan with it."""
    return GR.ring_chords_laplacian(M)


def make(kind, dev, n=N):
    L = laplacian()
    if kind == "resgnn":
        from cnn_graph_amd.model import ResGNN
        return ResGNN(L, N=n, Fin=2, nfilter=4, K=2, nres_layer_count=1, learning_rate=1e-2,
                      device=dev, seed=7)
    from cnn_graph_amd.glstm_gconv import GLSTMGconvModel
    return GLSTMGconvModel(L, n, T=2, feat_in=2, num_hidden=8, num_hidden_conv=8, K=2, keep_prob=0.8,
                           filter="fourier_conv", learning_rate=1e-2, device=dev, seed=7)


def channels(kind):
    return 2 if kind == "resgnn" else 4  # F * T for the LSTM model


@pytest.fixture(scope="module")
def problem():
    """Per kind: (train data, train labels, val data, val labels), host float32; made once."""
    out = {}
    for kind in KINDS:
        rng = np.random.default_rng(3)
        C = channels(kind)
        out[kind] = tuple((0.4 * rng.standard_normal(s)).astype(np.float32)
                          for s in ((S, M, C), (S, M, 2), (SV, M, C), (SV, M, 2)))
    return out


def state(model, acc, losses):
    torch.cuda.synchronize()
    return {"flat": model.flat.cpu().numpy().copy(), "s1": model.s1.cpu().numpy().copy(),
            "s2": model.s2.cpu().numpy().copy(), "step_count": np.array([model.step_count]),
            "loss_average": model.loss_average.cpu().numpy().copy(),
            "accuracies": np.array(acc, np.float64), "losses": np.array(losses, np.float64)}


def manual(kind, dev, prob):
    """The loop a user writes without fit."""
    from cnn_graph_amd.trainer import fit_schedule
    model = make(kind, dev)
    data, labels, vd, vl = (torch.from_numpy(a).to(dev) for a in prob)
    num_steps = int(EPOCHS * S / N)
    sched = fit_schedule(S, N, num_steps, SEED)
    acc, losses = [], []
    for step in range(1, num_steps + 1):
        idx = torch.from_numpy(sched[step - 1].astype(np.int64)).to(dev)
        model.train_step(data[idx], labels[idx])
        if step % EVERY == 0 or step == num_steps:
            _, mse, _, loss, _ = model.evaluate(vd, vl)
            acc.append(mse)
            losses.append(loss)
    return state(model, acc, losses)


@pytest.fixture(scope="module")
def manual_runs(dev, problem):
    """Two manual runs per kind from one seed, shared by the tests below."""
    return {kind: (manual(kind, dev, problem[kind]), manual(kind, dev, problem[kind])) for kind in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_fit_equals_the_manual_loop(dev, problem, manual_runs, kind, capsys):
    a, b = manual_runs[kind]
    repeatable = all(np.array_equal(a[k], b[k]) for k in a)
    model = make(kind, dev)
    acc, losses, t_step = model.fit(*problem[kind], num_epochs=EPOCHS, eval_frequency=EVERY, rng=SEED,
                                    verbose=False)
    got = state(model, acc, losses)
    num_steps = int(EPOCHS * S / N)
    evals = sum(1 for s in range(1, num_steps + 1) if s % EVERY == 0 or s == num_steps)
    assert len(acc) == len(losses) == evals == 3
    assert got["step_count"][0] == num_steps == 5
    assert t_step > 0
    assert capsys.readouterr().out == ""  # verbose=False prints nothing
    assert np.isfinite(got["flat"]).all() and not np.array_equal(got["flat"], make(kind, dev).flat.cpu().numpy())
    with capsys.disabled():
        print(f"\n{kind}: manual loop bitwise repeatable = {repeatable}")
    for k in a:
        spread, err = O.normwise_err(b[k], a[k]), O.normwise_err(got[k], a[k])
        with capsys.disabled():
            print(f"  {k}: manual spread {spread:.3e}, fit vs manual {err:.3e}")
        if repeatable:
            assert np.array_equal(got[k], a[k]), (kind, k, err)
        else:
            assert err <= spread, (kind, k, err, spread)


def test_fit_prints_the_reference_lines(dev, problem, capsys):
    model = make("resgnn", dev)
    model.fit(*problem["resgnn"], num_epochs=EPOCHS, eval_frequency=EVERY, rng=SEED)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "step 2 / 5 (epoch 0.80 / 2):"
    assert out[1].startswith("  learning_rate = 1.00e-02, loss_average = ")
    assert out[2].startswith("  validation mse: ") and f"( {SV})" in out[2]
    assert out[3].startswith("  time: ")
    assert out[8] == "step 5 / 5 (epoch 2.00 / 2):"
    assert out[-1].startswith("validation accuracy: peak = ") and len(out) == 13


def test_fit_takes_device_tensors_and_flat_labels(dev, problem, manual_runs):
    """Device tensors go in without a copy, and labels may come as [S, M * Fout]."""
    data, labels, vd, vl = (torch.from_numpy(a).to(dev) for a in problem["resgnn"])
    model = make("resgnn", dev)
    acc, losses, _ = model.fit(data, labels.reshape(S, -1), vd, vl, num_epochs=EPOCHS,
                               eval_frequency=EVERY, rng=np.random.RandomState(SEED), verbose=False)
    a, b = manual_runs["resgnn"]
    if all(np.array_equal(a[k], b[k]) for k in a):
        got = state(model, acc, losses)
        assert all(np.array_equal(got[k], a[k]) for k in a)


def test_refusals(dev, problem):
    data, labels, vd, vl = problem["resgnn"]
    model = make("resgnn", dev)
    before = model.flat.clone()
    with pytest.raises(ValueError, match="IndexError"):  # S < N
        model.fit(data[:N - 1], labels[:N - 1], vd, vl, num_epochs=2, rng=0, verbose=False)
    with pytest.raises(ValueError, match="number of samples"):
        model.fit(data, labels[:-1], vd, vl, num_epochs=2, rng=0, verbose=False)
    with pytest.raises(ValueError, match="number of samples"):
        model.fit(data, labels, vd, vl[:-1], num_epochs=2, rng=0, verbose=False)
    with pytest.raises(ValueError):  # a wrong vertex count
        model.fit(data[:, :-1], labels[:, :-1], vd, vl, num_epochs=2, rng=0, verbose=False)
    with pytest.raises(ValueError):  # fewer samples than one step needs
        model.fit(data, labels, vd, vl, num_epochs=0.1, rng=0, verbose=False)

    class TwoRanks:
        world = 2

    model.comm = TwoRanks()
    try:
        with pytest.raises(ValueError, match="same permutations"):
            model.fit(data, labels, vd, vl, num_epochs=2, rng=None, rank=0, verbose=False)
        with pytest.raises(ValueError, match="rank"):
            model.fit(data, labels, vd, vl, num_epochs=2, rng=0, rank=2, verbose=False)
    finally:
        model.comm = None
    torch.cuda.synchronize()
    assert model.step_count == 0 and torch.equal(model.flat, before)
