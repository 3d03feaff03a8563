"""dense_rnn.LSTMRNNModel data parallel: two ranks over gloo, keep 1, sgd.  The
replicas are bitwise equal after every step and within 1e-5 of one process on
the whole batch -- which holds only with grad_scale = 1 (the loss sums over the
batch, so the shards' gradients add; 1/world would halve every step)."""
import numpy as np
import pytest

import dense_rnn_dp_worker as Wk
import dp_harness as DP

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.mark.timeout(300)
def test_world2_matches_the_whole_batch(dev, tmp_path):
    d = DP.launch_world2("dense_rnn_dp_worker", tmp_path / "dense_rnn_dp.npz", 240)
    assert np.array_equal(d["P"], d["P_r1"]), "replicas diverged"
    x, labels = Wk.problem()
    P, losses = Wk.run(x, labels, dev, None)
    assert np.all(np.isfinite(losses))
    # the shards' losses add up to the whole batch's (a sum over the batch)
    assert np.all(np.abs(d["loss_sum"] - losses) < 1e-5 * np.abs(losses))
    DP.assert_tracks_full_batch(d["P"], P, Wk.STEPS, tol=TOL)
