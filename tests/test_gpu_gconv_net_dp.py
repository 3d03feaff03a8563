"""GConvNetModel data parallel: two ranks share the GPU over gloo
(tests/gconv_net_dp_worker.py, the pattern of tests/test_gpu_glstm_dp.py), two
samples each of a 4-sample batch, for each of the three networks -- the
three-branch flat buffer with merge_layer carved last included.  Bars: both
replicas bitwise equal after every step; the first step's exchanged gradient
(sum / 2) within 1e-5 (normwise) of the one-process full batch's, and the
parameters within 1e-5 of the full-batch run's after each of 3 Adam steps."""
import numpy as np
import pytest

import dp_harness as DP
import gconv_net_dp_worker as Wk
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
    d = DP.launch_world2("gconv_net_dp_worker", tmp_path / "gconv_net_dp.npz", 280)
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
        DP.assert_tracks_full_batch(d[f"{fn}_P"], P, Wk.STEPS)
