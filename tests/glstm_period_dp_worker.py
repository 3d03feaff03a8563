"""Case of tests/test_gpu_glstm_period.py::test_world2_over_gloo (not a test
module): the data-parallel training step of glstm_period.GLSTMPeriodModel in
both merge modes.  Rank r trains on its contiguous shard of a fixed global
batch; rank 0 writes both replicas' parameters after every step, and every
rank's wrapper seeds of a model built with dropout on.  Run through
tests/dp_harness.py (case ``glstm_period_dp_worker``)."""
import numpy as np

import dp_harness as DP

STEPS = 2
N_GLOBAL, M, T, FIN, H, K, FOUT, LAYERS = 4, 40, (3, 2, 4), 2, 8, 2, 2, 2
MODES = {"weights": "inference_glstm_period_expand", "concat": "inference_glstm_period_expand_gconv3"}


def problem():
    import glstm_gconv_ref as GR
    L = GR.ring_chords_laplacian(M)
    rng = np.random.default_rng(77)
    x = (0.5 * rng.standard_normal((N_GLOBAL, M, FIN * sum(T)))).astype(np.float32)
    labels = rng.standard_normal((N_GLOBAL, M, FOUT)).astype(np.float32)
    return L, x, labels


def build(mode, L, n, dev, comm, keep=1.0):
    from cnn_graph_amd import GLSTMPeriodModel
    return GLSTMPeriodModel(L, n, T, FIN, num_hidden=H, K=K, layer_count=LAYERS, conv_layer_num=1,
                            out_features=FOUT, keep_prob=keep, infer_func=MODES[mode],
                            learning_rate=1e-2, device=dev, seed=2017, comm=comm)


def run(mode, L, x, labels, dev, comm):
    """STEPS training steps; returns the parameters after each step [STEPS, P]."""
    import torch
    model = build(mode, L, x.shape[0], dev, comm)
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ys = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    return DP.train_steps(model, xs, ys, STEPS)[0]


def rank_result(rank, world, dev, comm):
    L, x, labels = problem()
    lo, hi = DP.shard_of(N_GLOBAL, rank, world)
    res = {}
    for mode in MODES:
        P = run(mode, L, x[lo:hi], labels[lo:hi], dev, comm)
        # the mask-stream seeds of this rank's wrappers (dropout on), as int64 bit patterns
        dropped = build(mode, L, hi - lo, dev, comm, keep=0.8)
        seeds = np.array([w._seed - (1 << 64) if w._seed >= 1 << 63 else w._seed
                          for ws in dropped.wrapped for w in ws], dtype=np.int64)
        res[f"{mode}_P"] = P
        res[f"{mode}_P_r1"] = DP.gather_ranks(P)[1]
        res[f"{mode}_seeds"] = np.stack(DP.gather_ranks(seeds))
    return res
