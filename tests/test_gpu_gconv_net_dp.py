"""GConvNetModel data parallel: two ranks share the GPU over gloo
(tests/gconv_net_dp_worker.py, the pattern of tests/test_gpu_glstm_dp.py), two
samples each of a 4-sample batch, for each of the three networks -- the
three-branch flat buffer with merge_layer carved last included.  Bars: both
replicas bitwise equal after every step; the first step's exchanged gradient
(sum / 2) within 1e-5 (normwise) of the one-process full batch's, and the
parameters within 1e-5 of the full-batch run's after each of 3 Adam steps."""
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
def test_gconv_net_world2_matches_full_batch(dev, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gconv_net_dp_worker as Wk
    out = tmp_path / "gconv_net_dp.npz"
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "gconv_net_dp_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    assert int(d["world"]) == 2
    L, x, labels = Wk.problem()
    for fn in Wk.INFER_FUNCS:
        assert np.array_equal(d[f"{fn}_P"], d[f"{fn}_P_r1"]), f"{fn}: replicas diverged"
        P, g1, names = Wk.run(fn, L, x, labels, dev, None)
        if fn == "inference_gconv_period_expand":
            assert names[-1] == "merge_layer/weights" and len(names) == 3 * (2 * Wk.R + 2) + 1
        assert np.all(np.isfinite(P))
        e_g = O.normwise_err(d[f"{fn}_g1"], g1.astype(np.float64))
        print(f"{fn}: first exchanged gradient, normwise err {e_g:.3e}")
        assert e_g < 1e-5, (fn, e_g)
        for n in range(Wk.STEPS):
            if n:
                assert not np.array_equal(d[f"{fn}_P"][n], d[f"{fn}_P"][n - 1])  # the update ran
            err = O.normwise_err(d[f"{fn}_P"][n], P[n].astype(np.float64))
            print(f"{fn} step {n + 1}: normwise err {err:.3e}")
            assert err < 1e-5, (fn, n + 1, err)
