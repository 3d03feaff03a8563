"""The opt-in for more than 64 KB of dynamic LDS is made per (device, kernel)
(csrc/launch.h): one process launches the row GEMM with 120 KB (k_rowgemm_x3<1>)
and with 80 KB (k_rowgemm<1, .>) of dynamic LDS on device 1 first, then on
device 0.  It guards that the row GEMM's opt-in and its resident count stay
keyed on the device: both devices succeed and compute the same bits.  (The row
GEMM was keyed on the device before the shared helper too, inside its occupancy
query, so this test pins that behaviour; it does not tell the helper from what
it replaced.)

Shape: the sample-major steps (variant 'steps') at M = 64, Fin = 32, K = 20,
Fout = 32, N = 2, so the y GEMM has Kc = 640 and one column tile.  Bars, as in
tests/test_gpu_stream_geometry.py: the basis bitwise equal to the oracle's fp32
CSR-order recurrence, y within 1e-5 (normwise) of the float64 oracle; and basis
and y bitwise equal between the two devices."""
import numpy as np
import pytest
import scipy.sparse

import stream_cases as S
from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_gpu_stream_geometry.py's
M, FIN, K, FOUT, N = 64, 32, 20, 32, 2


@pytest.fixture(scope="module")
def case(built_lib):
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs in one process")
    rp, ci, v = S.mixed_rows(M, 17)
    rng = np.random.default_rng(1317)
    x = rng.random((N, M, FIN), dtype=np.float32)
    x[:, S.empty_rows(rp), :] = 0
    W = (rng.standard_normal((FIN * K, FOUT)) * 0.1).astype(np.float32)
    ob, oy = O.cheb_forward(x, rp, ci, v, W, K)
    return (rp, ci, v), x, W, ob, oy


@pytest.mark.parametrize("gemm_x3", [1, 0])
def test_big_lds_row_gemm_on_second_device_first(case, gemm_x3):
    from cnn_graph_amd import _lib, ops
    from cnn_graph_amd.plan import ChebPlan
    (rp, ci, v), x, W, ob, oy = case
    Lt = scipy.sparse.csr_matrix((v, ci, rp), shape=(M, M))
    got = {}
    with _lib.options(gemm_x3=gemm_x3):
        for d in (1, 0):
            with torch.cuda.device(d):
                dev = torch.device("cuda", d)
                plan = ChebPlan(Lt, device=d, path="stream", variant="steps")
                assert plan.query_path(N, FIN, K, FOUT) == "stream"
                basis = torch.full((N * M, FIN * K), float("nan"), device=dev, dtype=torch.float32)
                _, y = ops.cheb_forward(plan, torch.from_numpy(x).to(dev), torch.from_numpy(W).to(dev),
                                        K, out_basis=basis)
                torch.cuda.synchronize(dev)
                got[d] = (basis.cpu().numpy(), y.cpu().numpy())
    for d, (basis, y) in got.items():
        assert np.array_equal(basis, ob), f"basis not bit-exact on device {d}"
        err = O.normwise_err(y, oy)
        print(f"device {d} gemm_x3={gemm_x3}: y normwise error {err:.2e}")
        assert err < TOL, f"y normwise error {err:.3e} on device {d}"
    assert np.array_equal(got[0][0], got[1][0]), "basis differs between the devices"
    assert np.array_equal(got[0][1], got[1][1]), "y differs between the devices"
