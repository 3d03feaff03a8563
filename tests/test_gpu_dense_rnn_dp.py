"""dense_rnn.LSTMRNNModel data parallel: two ranks over gloo, keep 1, sgd.  The
replicas are bitwise equal after every step and within 1e-5 of one process on
the whole batch -- which holds only with grad_scale = 1 (the loss sums over the
batch, so the shards' gradients add; 1/world would halve every step)."""
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

TOL = 1e-5


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.mark.timeout(300)
def test_world2_matches_the_whole_batch(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dense_rnn_dp_worker as Wk
    out = tmp_path / "dense_rnn_dp.npz"
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "dense_rnn_dp_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    assert int(d["world"]) == 2
    assert np.array_equal(d["P"], d["P_r1"]), "replicas diverged"
    x, labels = Wk.problem()
    P, losses = Wk.run(x, labels, dev, None)
    assert np.all(np.isfinite(losses))
    # the shards' losses add up to the whole batch's (a sum over the batch)
    assert np.all(np.abs(d["loss_sum"] - losses) < 1e-5 * np.abs(losses))
    for n in range(Wk.STEPS):
        if n:
            assert not np.array_equal(d["P"][n], d["P"][n - 1])  # the update ran
        err = O.normwise_err(d["P"][n], P[n].astype(np.float64))
        print(f"step {n + 1}: {err:.2e}")
        assert err < TOL, (n + 1, err)
