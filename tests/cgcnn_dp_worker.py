"""Case of tests/test_gpu_cgcnn_dp.py (not a test module): the data-parallel
training step of cgcnn.CGCNNModel.  Rank r trains on its contiguous shard of a
fixed global batch; rank 0 writes both replicas' parameters after every step.
Run through tests/dp_harness.py (case ``cgcnn_dp_worker``)."""
import numpy as np

import dp_harness as DP

STEPS = 2
N_GLOBAL, M, F, K, P, MFC = 8, [16, 8], [3, 4], [3, 2], [2, 2], [6, 5]
REG = 5e-2  # large, so a term added once per rank would miss the bar by far


def problem():
    """Two ring levels (16 and 8 vertices; pooling by 2 connects them), a batch of
    8 and its class ids."""
    import scipy.sparse

    def ring(m):
        i = np.arange(m)
        A = scipy.sparse.coo_matrix((np.ones(2 * m, np.float32),
                                     (np.concatenate([i, i]), np.concatenate([(i - 1) % m, (i + 1) % m]))),
                                    shape=(m, m)).tocsr()
        d = np.asarray(A.sum(axis=1)).ravel()
        D = scipy.sparse.diags(1 / np.sqrt(d)).astype(np.float32)
        return (scipy.sparse.identity(m, dtype=np.float32, format="csr") - D @ A @ D).tocsr()

    L = [ring(m) for m in M] + [ring(M[-1] // 2)]
    rng = np.random.default_rng(12)
    x = rng.standard_normal((N_GLOBAL, M[0], 1)).astype(np.float32)
    labels = rng.integers(0, MFC[-1], N_GLOBAL)
    return L, x, labels


def run(L, x, labels, dev, comm):
    """STEPS training steps: (parameters after each step [STEPS, P], the losses)."""
    import torch
    from cnn_graph_amd import CGCNNModel
    model = CGCNNModel(L, x.shape[0], F, K, P, MFC, regularization=REG, momentum=0.9, dropout=1.0,
                       learning_rate=0.05, decay_rate=0.95, decay_steps=1, device=dev, seed=2017,
                       comm=comm)
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return (*DP.train_steps(model, xs, labels, STEPS), (model.reg_begin, model.reg_n))


def rank_result(rank, world, dev, comm):
    L, x, labels = problem()
    lo, hi = DP.shard_of(N_GLOBAL, rank, world)
    Pm, losses, _ = run(L, x[lo:hi], labels[lo:hi], dev, comm)
    return dict(P=Pm, P_r1=DP.gather_ranks(Pm)[1], losses=losses)
