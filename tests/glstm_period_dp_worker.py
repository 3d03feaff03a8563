"""Worker of tests/test_gpu_glstm_period.py::test_world2_over_gloo (not a test
module): one rank of the data-parallel training step of
glstm_period.GLSTMPeriodModel in both merge modes, launched by
``torch.distributed.run --nproc-per-node 2``.  Both ranks share cuda:0 and
exchange over gloo (dist.TorchComm), as tests/glstm_dp_worker.py does.  Rank r
trains on its contiguous shard of a fixed global batch; rank 0 writes both
replicas' parameters after every step, and every rank's wrapper seeds of a
model built with dropout on.

  python -m torch.distributed.run --nproc-per-node 2 tests/glstm_period_dp_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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
    params = []
    for _ in range(STEPS):
        model.train_step(xs, ys)
        params.append(model.flat.cpu().numpy().copy())
    torch.cuda.synchronize()
    return np.stack(params)


def main():
    import torch
    import torch.distributed as dist
    from cnn_graph_amd import dist as cdist
    out = sys.argv[1]
    rank, world, _ = cdist.init(backend="gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L, x, labels = problem()
    lo, hi = cdist.shard(N_GLOBAL, rank, world)
    comm = cdist.TorchComm()
    res = {"world": world}
    for mode in MODES:
        P = run(mode, L, x[lo:hi], labels[lo:hi], dev, comm)
        gathered = [torch.zeros(P.size, dtype=torch.float32) for _ in range(world)]
        dist.all_gather(gathered, torch.from_numpy(P.reshape(-1)))
        # the mask-stream seeds of this rank's wrappers (dropout on), as int64 bit patterns
        dropped = build(mode, L, hi - lo, dev, comm, keep=0.8)
        seeds = torch.tensor([w._seed - (1 << 64) if w._seed >= 1 << 63 else w._seed
                              for ws in dropped.wrapped for w in ws], dtype=torch.int64)
        all_seeds = [torch.zeros_like(seeds) for _ in range(world)]
        dist.all_gather(all_seeds, seeds)
        res[f"{mode}_P"] = P
        res[f"{mode}_P_r1"] = gathered[1].numpy().reshape(P.shape)
        res[f"{mode}_seeds"] = torch.stack(all_seeds).numpy()
    if rank == 0:
        np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
