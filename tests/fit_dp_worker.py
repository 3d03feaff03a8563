"""Case of tests/test_gpu_fit_dp.py (not a test module): a data-parallel
``ResGNN.fit``.  Every rank builds the same seeded schedule of global batches
and trains on its own columns of it; rank 0 writes what the parent compares
with a one-process fit at the global batch.  Run through tests/dp_harness.py
(case ``fit_dp_worker``)."""
import numpy as np

import dp_harness as DP

N_GLOBAL, FIN, NFILTER, K, NRES = 4, 2, 8, 4, 1
S, SV, EPOCHS, EVERY, SEED = 10, 6, 2, 2, 33


def problem():
    """Graph (golden A's Laplacian) and the datasets shared by every rank."""
    L = DP.golden_laplacian("golden_A.npz")
    M = L.shape[0]
    rng = np.random.default_rng(9)
    sets = tuple(rng.standard_normal(s).astype(np.float32)
                 for s in ((S, M, FIN), (S, M, 2), (SV, M, FIN), (SV, M, 2)))
    return L, sets


def run(N, L, sets, comm, dev):
    """fit at per-rank batch N; returns (flat params, accuracies, losses, step count)."""
    import torch
    from cnn_graph_amd.model import ResGNN
    net = ResGNN(L, N, FIN, NFILTER, K, NRES, device=dev, comm=comm, seed=2017)
    acc, losses, _ = net.fit(*sets, num_epochs=EPOCHS, eval_frequency=EVERY, rng=SEED, verbose=False)
    torch.cuda.synchronize()
    return net.flat.detach().cpu().numpy(), np.array(acc), np.array(losses), net.step_count


def rank_result(rank, world, dev, comm):
    L, sets = problem()
    flat, acc, losses, steps = run(N_GLOBAL // world, L, sets, comm, dev)  # rank: the launcher's
    return dict(flat=flat, flat_r1=DP.gather_ranks(flat)[1], acc=acc, losses=losses, steps=steps)
