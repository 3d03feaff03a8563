"""Worker of tests/test_gpu_cgcnn_dp.py (not a test module): one rank of the
data-parallel training step of cgcnn.CGCNNModel, launched by
``torch.distributed.run --nproc-per-node 2``.  Both ranks share cuda:0 and
exchange over gloo (dist.TorchComm), as tests/glstm_dp_worker.py does.  Rank r
trains on its contiguous shard of a fixed global batch; rank 0 writes both
replicas' parameters after every step.

  python -m torch.distributed.run --nproc-per-node 2 tests/cgcnn_dp_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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
    params, losses = [], []
    for _ in range(STEPS):
        losses.append(float(model.train_step(xs, labels)))
        params.append(model.flat.cpu().numpy().copy())
    torch.cuda.synchronize()
    return np.stack(params), np.array(losses), (model.reg_begin, model.reg_n)


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
    Pm, losses, _ = run(L, x[lo:hi], labels[lo:hi], dev, cdist.TorchComm())
    gathered = [torch.zeros(Pm.size, dtype=torch.float32) for _ in range(world)]
    dist.all_gather(gathered, torch.from_numpy(Pm.reshape(-1)))
    if rank == 0:
        np.savez(out, world=world, P=Pm, P_r1=gathered[1].numpy().reshape(Pm.shape), losses=losses)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
