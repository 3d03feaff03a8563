"""Data-parallel ``fit`` at world size 2 (tests/fit_dp_worker.py): two ranks at
N = 2 each over dist.TorchComm (gloo: both ranks share this box's one GPU,
which RCCL does not allow), each reading its own columns of the one seeded
schedule of global batches, against one process fitting at N = 4 with the same
seed.  Bars, those of tests/test_gpu_dp.py: both replicas bitwise identical
after the run, and their parameters within 1e-4 normwise of the one-process
run's (Adam's normalised step amplifies fp32 reduction-order differences)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
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
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fit_dp_worker as Wk
    out = tmp_path / "fit_dp.npz"
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "fit_dp_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    L, sets = Wk.problem()
    flat, acc, losses, steps = Wk.run(Wk.N_GLOBAL, L, sets, None, dev)
    assert int(d["world"]) == 2 and int(d["steps"]) == steps == int(Wk.EPOCHS * Wk.S / Wk.N_GLOBAL)
    assert np.array_equal(d["flat"], d["flat_r1"]), "replicas diverged"
    assert O.normwise_err(d["flat"], flat) < 1e-4
    assert len(d["acc"]) == len(acc) == 3
