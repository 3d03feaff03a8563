"""Case of tests/test_gpu_dp.py (not a test module): a data-parallel ResGNN
training step on the HIP kernels.  Rank r trains on its contiguous shard of a
fixed global batch and rank 0 writes what the parent compares with a
one-process full-batch run.  Run through tests/dp_harness.py (case
``dp_resgnn_worker``)."""
import numpy as np

import dp_harness as DP

STEPS = 3
N_GLOBAL, FIN, NFILTER, K, NRES = 8, 2, 8, 4, 1


def problem():
    """Graph (golden A's Laplacian), inputs and labels shared by every rank."""
    L = DP.golden_laplacian("golden_A.npz")
    M = L.shape[0]
    rng = np.random.default_rng(7)
    x = rng.standard_normal((N_GLOBAL, M, FIN)).astype(np.float32)
    labels = rng.standard_normal((N_GLOBAL, M, 2)).astype(np.float32)
    return L, x, labels


def run(N, x, labels, L, comm, dev):
    """STEPS train steps; returns (losses, grad after step 1, flat params)."""
    import torch
    from cnn_graph_amd.model import ResGNN
    net = ResGNN(L, N, FIN, NFILTER, K, NRES, device=dev, comm=comm, seed=2017)
    P, losses, g1 = DP.train_steps(net, torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev),
                                  STEPS, first_grad=True)
    return losses, g1, P[-1]


def rank_result(rank, world, dev, comm):
    L, x, labels = problem()
    lo, hi = DP.shard_of(N_GLOBAL, rank, world)
    losses, g1, flat = run(hi - lo, x[lo:hi], labels[lo:hi], L, comm, dev)
    # mean of the shard means = full-batch mean
    return dict(loss=sum(DP.gather_ranks(losses)) / world, grad1=g1 / world, flat=flat,
                flat_r1=DP.gather_ranks(flat)[1])
