"""Case of tests/test_gpu_glstm_dp.py (not a test module): the data-parallel
gconv-LSTM training step (gconv_lstm.GLSTMModel: glstm_layer + fc_layer + MSE +
Adam, ONE all-reduce of the flat gradient bucket per step, grad_scale = 1/world)
at config E's graph and shape (T = 12, K = 3, H = 32, Fin = 2).  Rank r trains
on its contiguous shard of a fixed global batch; rank 0 writes both replicas'
parameters after every step and the first step's exchanged gradient bucket for
the parent to compare.  Run through tests/dp_harness.py (case
``glstm_dp_worker``)."""
import numpy as np

import dp_harness as DP

STEPS = 3
N_GLOBAL, T, FIN, H, K, FOUT = 8, 12, 2, 32, 3, 2


def problem():
    """Config E's graph (golden_E.npz: L~ of the 1024-vertex grid; the model is
    built from L = L~ + I so that rescale_L(L, 2) = L~), the input sequence as
    the reference feeds it ([N, M, Fin*T]) and the labels."""
    import scipy.sparse
    from conftest import case, load_golden
    c = case(load_golden("golden_E.npz"))
    M = c["M"]
    Lt = scipy.sparse.csr_matrix((c["Lt_val"], c["Lt_col"], c["Lt_rowptr"]), shape=(M, M))
    L = (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr()
    rng = np.random.default_rng(512)
    x = rng.random((N_GLOBAL, M, FIN * T), dtype=np.float32)
    labels = rng.random((N_GLOBAL, M, FOUT), dtype=np.float32)
    return L, x, labels


def run(L, x, labels, dev, comm, optimizer="adam"):
    """STEPS training steps; returns (params after each step [STEPS, P], the
    gradient bucket of step 1 divided by the world size [P], losses)."""
    import torch
    from cnn_graph_amd.gconv_lstm import GLSTMModel
    N = x.shape[0]
    model = GLSTMModel(L, N, T, FIN, num_hidden=H, K=K, out_features=FOUT, keep_prob=1.0,
                       optimizer=optimizer, device=dev, seed=2017, comm=comm)
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ys = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    P, losses, g1 = DP.train_steps(model, xs, ys, STEPS, first_grad=True)
    return P, g1 / model.world, losses


def rank_result(rank, world, dev, comm):
    L, x, labels = problem()
    lo, hi = DP.shard_of(N_GLOBAL, rank, world)
    P, g1, _ = run(L, x[lo:hi], labels[lo:hi], dev, comm)
    return dict(P=P, P_r1=DP.gather_ranks(P)[1], g1=g1)
