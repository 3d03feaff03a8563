"""Case of tests/test_gpu_dense_rnn_dp.py (not a test module): the
data-parallel dense LSTM baseline (dense_rnn.LSTMRNNModel: class softmax
cross-entropy summed over the batch, sgd; ONE all-reduce(sum) of the flat
gradient bucket per step and grad_scale = 1).  Rank r trains on its contiguous
shard of a fixed global batch; rank 0 writes both replicas' parameters after
every step for the parent to compare.  Run through tests/dp_harness.py (case
``dense_rnn_dp_worker``)."""
import numpy as np

import dp_harness as DP

STEPS = 3
N_GLOBAL, T, C, H, LR = 4, 3, 40, 32, 0.01


def problem():
    rng = np.random.default_rng(77)
    x = rng.standard_normal((N_GLOBAL, C, T)).astype(np.float32)
    labels = rng.integers(0, C, (N_GLOBAL, T))
    return x, labels


def run(x, labels, dev, comm):
    """STEPS sgd steps; returns (params after each step [STEPS, P], losses)."""
    import torch
    from cnn_graph_amd.dense_rnn import LSTMRNNModel
    model = LSTMRNNModel(x.shape[0], T, C, num_hidden=H, keep_prob=1.0, optimizer="sgd", learning_rate=LR,
                         device=dev, seed=2017, comm=comm)
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return DP.train_steps(model, xs, labels, STEPS)


def rank_result(rank, world, dev, comm):
    x, labels = problem()
    lo, hi = DP.shard_of(N_GLOBAL, rank, world)
    P, losses = run(x[lo:hi], labels[lo:hi], dev, comm)
    return dict(P=P, P_r1=DP.gather_ranks(P)[1], loss_sum=sum(DP.gather_ranks(losses)))
