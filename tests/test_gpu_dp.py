"""Data parallelism of the training step with the HIP kernels at world size 2
(the exchange sits between compute_gradients and
apply_gradients, lib/graph_model.py:296-298): two ranks, each running
ResGNN.train_step on its half of a fixed batch with ONE all-reduce of the flat
gradient buffer per step (dist.TorchComm over gloo: both ranks share this
box's one GPU, which RCCL does not allow), against one process training on the
whole batch.  Bars: the exchanged gradient / world and the loss within 1e-5
normwise of the full-batch ones, both replicas bitwise identical after three
steps, and their parameters within 1e-4 of the full-batch run's (Adam's
normalised step amplifies fp32 reduction-order differences)."""
import numpy as np
import pytest

import dp_harness as DP
import dp_resgnn_worker as Wk
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.mark.timeout(300)
def test_resgnn_dp_world2_matches_full_batch(dev, tmp_path):
    d = DP.launch_world2("dp_resgnn_worker", tmp_path / "dp.npz", 240)
    L, x, labels = Wk.problem()
    losses, g1, flat = Wk.run(Wk.N_GLOBAL, x, labels, L, None, dev)
    assert np.array_equal(d["flat"], d["flat_r1"]), "replicas diverged"
    assert O.normwise_err(d["loss"], losses) < 1e-5
    assert O.normwise_err(d["grad1"], g1) < 1e-5
    assert O.normwise_err(d["flat"], flat) < 1e-4
