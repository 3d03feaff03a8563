"""Writes resgnn_steps.npz: the flat parameters and the loss of ``ResGNN`` (both
filters) after two ``train_step``s on a 40-vertex graph, as the commit BEFORE
``_ResNet`` gained its ``input_grad`` switch computed them on an MI355X.
tests/test_gpu_glstm_gconv.py::test_resgnn_unchanged replays the same steps and
compares bitwise.

How it was generated: with the parent commit's package (its Python files and
its built libcheb_mi355.so) first on PYTHONPATH,

    PYTHONPATH=<parent checkout> python tests/golden/make_resgnn_steps.py OUT.npz

The inputs come from ``resgnn_case`` below, which the test imports, so both
sides draw the same numbers.  Needs a GPU; not run by the suite.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# after PYTHONPATH, so that a parent checkout named there provides cnn_graph_amd
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.append(p)

CASE = dict(M=40, N=3, Fin=3, F=8, K=3, R=1, Fout=2, seed=11, steps=2)


def resgnn_case():
    """(L, x [N, M, Fin], labels [N, M, Fout]) of the golden steps."""
    import glstm_gconv_ref as GR
    c = CASE
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((c["N"], c["M"], c["Fin"])).astype(np.float32)
    labels = rng.standard_normal((c["N"], c["M"], c["Fout"])).astype(np.float32)
    return GR.ring_chords_laplacian(c["M"]), x, labels


def run_steps(filter):
    """(flat parameters, loss) after CASE['steps'] steps of a fresh ResGNN."""
    import torch
    from cnn_graph_amd.model import ResGNN
    c = CASE
    L, x, labels = resgnn_case()
    dev = torch.device("cuda", 0)
    m = ResGNN(L, c["N"], c["Fin"], c["F"], c["K"], c["R"], c["Fout"], device=dev, seed=c["seed"],
               filter=filter)
    xt, lt = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    for _ in range(c["steps"]):
        loss = m.train_step(xt, lt)
    torch.cuda.synchronize()
    return m.flat.cpu().numpy(), loss.cpu().numpy()


if __name__ == "__main__":
    out = {}
    for f in ("chebyshev5", "fourier"):
        out[f"{f}_flat"], out[f"{f}_loss"] = run_steps(f)
    np.savez(sys.argv[1], **out)
    print({k: v.shape for k, v in out.items()})
