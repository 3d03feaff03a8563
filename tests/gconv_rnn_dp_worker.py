"""Case of tests/test_gpu_gconv_rnn.py (not a test module): the data-parallel
gconvRNN sequence model (gconv_rnn.GConvRNNModel: gconv-LSTM, per-step head,
vertex softmax cross-entropy summed over the batch, sgd; ONE all-reduce(sum) of
the flat gradient bucket per step and grad_scale = 1) on config A's graph.  Rank
r trains on its contiguous shard of a fixed global batch; rank 0 writes both
replicas' parameters after every step for the parent to compare.  Run through
tests/dp_harness.py (case ``gconv_rnn_dp_worker``)."""
import numpy as np

import dp_harness as DP

STEPS = 3
N_GLOBAL, T, FIN, H, K, LR = 4, 3, 2, 32, 3, 0.01


def problem():
    """Config A's graph (golden_A.npz: L~ of the 100-vertex 4-NN graph; the
    model is built from L = L~ + I so that rescale_L(L, 2) = L~), the input
    [N, M, Fin, T] and the target vertices [N, T]."""
    import scipy.sparse
    from conftest import case, load_golden
    c = case(load_golden("golden_A.npz"))
    M = c["M"]
    Lt = scipy.sparse.csr_matrix((c["Lt_val"], c["Lt_col"], c["Lt_rowptr"]), shape=(M, M))
    L = (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr()
    rng = np.random.default_rng(77)
    x = rng.standard_normal((N_GLOBAL, M, FIN, T)).astype(np.float32)
    labels = rng.integers(0, M, (N_GLOBAL, T))
    return L, x, labels


def run(L, x, labels, dev, comm):
    """STEPS sgd steps; returns (params after each step [STEPS, P], losses)."""
    import torch
    from cnn_graph_amd.gconv_rnn import GConvRNNModel
    model = GConvRNNModel(L, x.shape[0], T, FIN, num_hidden=H, K=K, keep_prob=1.0, optimizer="sgd",
                          learning_rate=LR, device=dev, seed=2017, comm=comm)
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return DP.train_steps(model, xs, labels, STEPS)


def rank_result(rank, world, dev, comm):
    L, x, labels = problem()
    lo, hi = DP.shard_of(N_GLOBAL, rank, world)
    P, losses = run(L, x[lo:hi], labels[lo:hi], dev, comm)
    return dict(P=P, P_r1=DP.gather_ranks(P)[1], loss_sum=sum(DP.gather_ranks(losses)))
