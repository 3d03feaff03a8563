"""Worker of tests/test_gpu_fit_dp.py (not a test module): one rank of a
data-parallel ``ResGNN.fit``, launched by ``torch.distributed.run
--nproc-per-node 2``.  Both ranks share cuda:0 and exchange through a gloo group
(dist.TorchComm; RCCL refuses two ranks on one GPU).  Every rank builds the
same seeded schedule of global batches and trains on its own columns of it;
rank 0 writes what the parent compares with a one-process fit at the global
batch.

  python -m torch.distributed.run --nproc-per-node 2 tests/fit_dp_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_GLOBAL, FIN, NFILTER, K, NRES = 4, 2, 8, 4, 1
S, SV, EPOCHS, EVERY, SEED = 10, 6, 2, 2, 33


def problem():
    """Graph (golden A's Laplacian) and the datasets shared by every rank."""
    import scipy.sparse
    from conftest import load_golden
    g = load_golden("golden_A.npz")
    L = scipy.sparse.csr_matrix((g["L_data"], g["L_indices"], g["L_indptr"]), shape=tuple(g["L_shape"]))
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


def main():
    import torch
    import torch.distributed as dist
    from cnn_graph_amd import dist as cdist
    out = sys.argv[1]
    rank, world, _ = cdist.init(backend="gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L, sets = problem()
    comm = cdist.TorchComm()
    flat, acc, losses, steps = run(N_GLOBAL // world, L, sets, comm, dev)  # rank: the launcher's
    flats = [torch.zeros(flat.size, dtype=torch.float32) for _ in range(world)]
    dist.all_gather(flats, torch.from_numpy(flat))
    if rank == 0:
        np.savez(out, flat=flat, flat_r1=flats[1].numpy(), acc=acc, losses=losses, steps=steps, world=world)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
