"""Data-parallel ``fit`` at world size 2 (tests/fit_dp_worker.py): two ranks at
N = 2 each over dist.TorchComm (gloo: both ranks share this box's one GPU,
which RCCL does not allow), each reading its own columns of the one seeded
schedule of global batches, against one process fitting at N = 4 with the same
seed.  Bars, those of tests/test_gpu_dp.py: both replicas bitwise identical
after the run, and their parameters within 1e-4 normwise of the one-process
run's (Adam's normalised step amplifies fp32 reduction-order differences)."""
import numpy as np
import pytest

import dp_harness as DP
import fit_dp_worker as Wk
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.mark.timeout(300)
def test_fit_dp_world2_matches_one_process(dev, tmp_path):
    d = DP.launch_world2("fit_dp_worker", tmp_path / "fit_dp.npz", 240)
    L, sets = Wk.problem()
    flat, acc, losses, steps = Wk.run(Wk.N_GLOBAL, L, sets, None, dev)
    assert int(d["steps"]) == steps == int(Wk.EPOCHS * Wk.S / Wk.N_GLOBAL)
    assert np.array_equal(d["flat"], d["flat_r1"]), "replicas diverged"
    assert O.normwise_err(d["flat"], flat) < 1e-4
    assert len(d["acc"]) == len(acc) == 3
