"""Worker of tests/test_gpu_dense_rnn_dp.py (not a test module): one rank of the
data-parallel dense LSTM baseline (dense_rnn.LSTMRNNModel: class softmax
cross-entropy summed over the batch, sgd; ONE all-reduce(sum) of the flat
gradient bucket per step and grad_scale = 1), launched by
``torch.distributed.run --nproc-per-node 2``.  Both ranks share cuda:0 and
exchange over gloo (dist.TorchComm).  Rank r trains on its contiguous shard of a
fixed global batch; rank 0 writes both replicas' parameters after every step for
the parent to compare.

  python -m torch.distributed.run --nproc-per-node 2 tests/dense_rnn_dp_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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
    params, losses = [], []
    for _ in range(STEPS):
        loss = model.train_step(xs, labels)
        params.append(model.flat.cpu().numpy().copy())
        losses.append(float(loss.item()))
    torch.cuda.synchronize()
    return np.stack(params), np.array(losses)


def main():
    import torch
    import torch.distributed as dist
    from cnn_graph_amd import dist as cdist
    out = sys.argv[1]
    rank, world, _ = cdist.init(backend="gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    x, labels = problem()
    lo, hi = cdist.shard(N_GLOBAL, rank, world)
    P, losses = run(x[lo:hi], labels[lo:hi], dev, cdist.TorchComm())
    gathered = [torch.zeros(P.size, dtype=torch.float32) for _ in range(world)]
    dist.all_gather(gathered, torch.from_numpy(P.reshape(-1)))
    all_losses = [torch.zeros(STEPS, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(all_losses, torch.from_numpy(losses))
    if rank == 0:
        np.savez(out, P=P, P_r1=gathered[1].numpy().reshape(P.shape), world=world,
                 loss_sum=sum(l.numpy() for l in all_losses))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
