"""The one harness of the world-2 data-parallel tests (not a test module, not a
conftest).  A test calls ``launch_world2(case, out, timeout)``; that starts two
ranks under torchrun on this file, each of which runs the case module's
``rank_result(rank, world, dev, comm)``, and rank 0 saves what it returned.
The ranks share cuda:0 and exchange over gloo (dist.TorchComm; RCCL refuses two
ranks on one GPU), the same train_step code path the RCCL comm drives at N > 1.

The rules, stated here and followed by every launch:
  * the child is always a fresh process (subprocess.run), never a replaced one;
  * two ranks plus the parent open the GPU: three processes in all;
  * every launch carries a time limit, the caller's, below its pytest timeout;
  * a non-zero status ends the test there, with the tails of the child's output.

One case by hand:
  python -m torch.distributed.run --nproc-per-node 2 tests/dp_harness.py CASE OUT.npz
"""
import importlib
import os
import socket
import subprocess
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CASES = ("dp_resgnn_worker", "dp_bench_worker", "fit_dp_worker", "glstm_dp_worker",
         "glstm_period_dp_worker", "gconv_rnn_dp_worker", "gconv_net_dp_worker", "cgcnn_dp_worker",
         "dense_rnn_dp_worker", "dp_selfcheck_case", "dp_selfcheck_raises_case")
LAUNCHER_VARS = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")


def known_case(case):
    if case not in CASES:
        raise ValueError(f"unknown data-parallel case {case!r}; the cases are {', '.join(CASES)}")
    return case


# -- parent side: the tests ---------------------------------------------------------
def child_env(strip_launcher_vars=False):
    """The environment of a child that opens the GPU next to this process;
    without a launcher's rank variables for a child that starts its own ranks."""
    env = {k: v for k, v in os.environ.items() if not (strip_launcher_vars and k in LAUNCHER_VARS)}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def launch_world2(case, out, timeout):
    """Run ``case`` on two ranks and return what rank 0 saved to ``out``."""
    known_case(case)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(TESTS, "dp_harness.py"), case, str(out)]
    r = subprocess.run(cmd, env=child_env(), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    assert int(d["world"]) == 2
    return d


def assert_tracks_full_batch(dp, full, steps, tol=1e-5, start=None):
    """Every step moved the data-parallel parameters ``dp[n]`` (step 0: away from
    ``start``, where given) and left them within ``tol`` normwise of ``full[n]``."""
    from oracle import cheb_oracle as O
    for n in range(steps):
        prev = dp[n - 1] if n else start
        if prev is not None:
            assert not np.array_equal(dp[n], prev), f"step {n + 1}: the update did not run"
        err = O.normwise_err(dp[n], full[n].astype(np.float64))
        print(f"step {n + 1}: normwise err {err:.3e}")
        assert err < tol, (n + 1, err)


# -- worker side: one rank under torchrun -------------------------------------------
def golden_laplacian(name):
    """The Laplacian stored in golden file ``name`` as a scipy CSR matrix."""
    import scipy.sparse
    from conftest import load_golden
    g = load_golden(name)
    return scipy.sparse.csr_matrix((g["L_data"], g["L_indices"], g["L_indptr"]), shape=tuple(g["L_shape"]))


def shard_of(n_global, rank, world):
    from cnn_graph_amd import dist as cdist
    return cdist.shard(n_global, rank, world)


def gather_ranks(array):
    """Every rank's copy of ``array`` (any dtype; one shape on all ranks), by rank."""
    import torch
    import torch.distributed as dist
    mine = torch.from_numpy(np.ascontiguousarray(array))
    every = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(every, mine)
    return [t.numpy() for t in every]


def train_steps(model, xs, labels, steps, first_grad=False):
    """``steps`` train steps: (parameters after each step [steps, P], losses
    [steps]), and with ``first_grad`` the gradient bucket after step 1 as a third."""
    import torch
    params, losses, g1 = [], [], None
    for n in range(steps):
        loss = model.train_step(xs, labels)
        if first_grad and n == 0:
            g1 = model.grad.detach().cpu().numpy().copy()
        params.append(model.flat.detach().cpu().numpy().copy())
        losses.append(float(loss))
    torch.cuda.synchronize()
    P, losses = np.stack(params), np.array(losses)
    return (P, losses, g1) if first_grad else (P, losses)


def main(case, out):
    sys.path[:0] = [ROOT, TESTS]
    mod = importlib.import_module(known_case(case))
    import torch
    import torch.distributed as dist
    from cnn_graph_amd import dist as cdist
    rank, world, _ = cdist.init(backend="gloo")
    dev = None
    if getattr(mod, "DEVICE", "cuda") != "cpu":
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
    res = mod.rank_result(rank, world, dev, cdist.TorchComm())
    if rank == 0:
        np.savez(out, world=world, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    # recorded, a failing rank's traceback closes torchrun's report: the tail the parent shows
    from torch.distributed.elastic.multiprocessing.errors import record
    record(main)(*sys.argv[1:])
