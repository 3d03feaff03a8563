"""Worker of tests/test_gpu_gconv_net_dp.py (not a test module): one rank of the
data-parallel training step of gconv_net.GConvNetModel for each of its three
networks, launched by ``torch.distributed.run --nproc-per-node 2``.  Both ranks
share cuda:0 and exchange over gloo (dist.TorchComm), as tests/glstm_dp_worker.py
does.  Rank r trains on its contiguous shard of a fixed global batch; rank 0
writes both replicas' parameters after every step and its first exchanged
gradient.

  python -m torch.distributed.run --nproc-per-node 2 tests/gconv_net_dp_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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
    params, g1 = [], None
    for _ in range(STEPS):
        model.train_step(xs, ys)
        if g1 is None:
            g1 = model.grad.cpu().numpy() / model.world
        params.append(model.flat.cpu().numpy().copy())
    torch.cuda.synchronize()
    return np.stack(params), g1, list(model.names)


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
    for fn in INFER_FUNCS:
        P, g1, _ = run(fn, L, x[lo:hi], labels[lo:hi], dev, comm)
        gathered = [torch.zeros(P.size, dtype=torch.float32) for _ in range(world)]
        dist.all_gather(gathered, torch.from_numpy(P.reshape(-1)))
        res[f"{fn}_P"] = P
        res[f"{fn}_P_r1"] = gathered[1].numpy().reshape(P.shape)
        res[f"{fn}_g1"] = g1
    if rank == 0:
        np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
