"""cgcnn.CGCNNModel data parallel: two ranks share this box's GPU over gloo (RCCL
refuses two ranks on one device), 4 samples each; one process trains on the
whole 8-sample batch.  ONE all-reduce of the flat gradient bucket per step,
grad_scale = 1/world, and the L2 term added once, in the update after the
exchange.  Bars: both replicas bitwise equal after every step; the parameters
within 1e-5 (normwise) of the full-batch run's after each of 2 Momentum steps
with regularization = 5e-2 -- a term added once per rank would double it."""
import numpy as np
import pytest

import cgcnn_dp_worker as Wk
import dp_harness as DP
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.mark.timeout(400)
def test_cgcnn_dp_world2_matches_full_batch(dev, tmp_path):
    d = DP.launch_world2("cgcnn_dp_worker", tmp_path / "cgcnn_dp.npz", 360)
    assert np.array_equal(d["P"], d["P_r1"]), "replicas diverged"
    L, x, labels = Wk.problem()
    P, losses, (rb, rn) = Wk.run(L, x, labels, dev, None)
    assert np.all(np.isfinite(losses)) and np.all(np.isfinite(d["losses"]))
    DP.assert_tracks_full_batch(d["P"], P, Wk.STEPS)
    # the bar sees the term: one step without it ends further away than the bar
    from cnn_graph_amd import CGCNNModel
    plain = CGCNNModel(L, Wk.N_GLOBAL, Wk.F, Wk.K, Wk.P, Wk.MFC, regularization=0.0, momentum=0.9,
                       learning_rate=0.05, decay_rate=0.95, decay_steps=1, device=dev, seed=2017)
    plain.train_step(torch.from_numpy(x).to(dev), labels)
    torch.cuda.synchronize()
    reg = slice(rb, rb + rn)
    assert O.normwise_err(plain.flat.cpu().numpy()[reg], P[0][reg].astype(np.float64)) > 1e-4
