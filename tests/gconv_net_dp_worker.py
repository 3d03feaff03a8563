"""Case of tests/test_gpu_gconv_net_dp.py (not a test module): the data-parallel
training step of gconv_net.GConvNetModel for each of its three networks.  Rank
r trains on its contiguous shard of a fixed global batch; rank 0 writes both
replicas' parameters after every step and its first exchanged gradient.  Run
through tests/dp_harness.py (case ``gconv_net_dp_worker``)."""
import numpy as np

import dp_harness as DP

STEPS = 3
N_GLOBAL, M, T, H, K, R, FOUT = 4, 40, (2, 1, 3), 8, 3, 2, 2
INFER_FUNCS = ("inference_gconv", "inference_gconv_period_no_expand", "inference_gconv_period_expand")


def problem():
    import glstm_gconv_ref as GG
    L = GG.ring_chords_laplacian(M)
    rng = np.random.default_rng(78)
    x = rng.standard_normal((N_GLOBAL, M, 2 * sum(T))).astype(np.float32)
    labels = (100 * rng.standard_normal((N_GLOBAL, M, FOUT))).astype(np.float32)
    return L, x, labels


def run(infer_func, L, x, labels, dev, comm):
    """STEPS training steps: (parameters after each step [STEPS, P], the first
    step's gradient bucket as the optimizer saw it, divided by world)."""
    import torch
    from cnn_graph_amd import GConvNetModel
    model = GConvNetModel(L, x.shape[0], T=T, num_hidden=H, K=K, conv_layer_num=R, out_features=FOUT,
                          infer_func=infer_func, learning_rate=1e-3, device=dev, seed=2017, comm=comm)
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ys = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    P, _, g1 = DP.train_steps(model, xs, ys, STEPS, first_grad=True)
    return P, g1 / model.world, list(model.names)


def rank_result(rank, world, dev, comm):
    L, x, labels = problem()
    lo, hi = DP.shard_of(N_GLOBAL, rank, world)
    res = {}
    for fn in INFER_FUNCS:
        P, g1, _ = run(fn, L, x[lo:hi], labels[lo:hi], dev, comm)
        res[f"{fn}_P"] = P
        res[f"{fn}_P_r1"] = DP.gather_ranks(P)[1]
        res[f"{fn}_g1"] = g1
    return res
