"""Writes the train-step goldens that later refactors are held to, bitwise.

resgnn_steps.npz: the flat parameters and the loss of ``ResGNN`` (both filters)
after two ``train_step``s on a 40-vertex graph, as the commit BEFORE ``_ResNet``
gained its ``input_grad`` switch computed them on an MI355X.
tests/test_gpu_glstm_gconv.py::test_resgnn_unchanged replays the same steps and
compares bitwise.

model_steps.npz (``--models``): flat, loss and the loss moving average of the
other three model classes (``MODEL_CASES``) after two ``train_step``s with
``decay_steps=1, decay_rate=0.95`` (the second step runs at the decayed rate), as
the commit BEFORE the four models moved onto ``trainer.FlatTrainer`` computed
them.  ``test_models_unchanged`` replays them.  It was recorded twice, in two
processes, and the two files were identical.

How they were generated: with the parent commit's package (its Python files and
its built libcheb_mi355.so) first on PYTHONPATH,

    PYTHONPATH=<parent checkout> python tests/golden/make_resgnn_steps.py OUT.npz
    PYTHONPATH=<parent checkout> python tests/golden/make_resgnn_steps.py --models OUT.npz

The inputs come from ``resgnn_case`` / ``model_case`` below, which the tests
import, so both sides draw the same numbers.  Needs a GPU; not run by the suite.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# after PYTHONPATH, so that a parent checkout named there provides cnn_graph_amd
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.append(p)

CASE = dict(M=40, N=3, Fin=3, F=8, K=3, R=1, Fout=2, seed=11, steps=2)

# the suite's small shapes: 40-vertex ring with chords, N 3, T 3, F 2, C 8
MODEL = dict(M=40, N=3, T=3, F=2, C=8, Fout=2, seed=11, steps=2, decay_steps=1, decay_rate=0.95)
_LSTM = dict(layer_count=2, keep_prob=0.8)
_HEAD = dict(num_hidden=8, num_hidden_conv=8, K=2, conv_layer_num=1, **_LSTM)
# name -> (class, constructor keywords beyond the shapes of MODEL)
MODEL_CASES = {
    "stacked_chebyshev5": ("StackedResGNN", dict(filter="chebyshev5")),
    "stacked_fourier": ("StackedResGNN", dict(filter="fourier")),
    "glstm_cheby_step_adam": ("GLSTMModel", dict(num_hidden=8, K=3, optimizer="adam", **_LSTM)),
    "glstm_cheby_step_sgd": ("GLSTMModel", dict(num_hidden=8, K=3, optimizer="sgd", **_LSTM)),
    "glstm_cheby_step_rmsprop": ("GLSTMModel", dict(num_hidden=8, K=3, optimizer="rmsprop", **_LSTM)),
    "glstm_cheby_seq": ("GLSTMModel", dict(num_hidden=32, K=2, **_LSTM)),
    "glstm_fourier": ("GLSTMModel", dict(num_hidden=8, filter="fourier_conv", **_LSTM)),
    "glstm_gconv_fourier_fused": ("GLSTMGconvModel", dict(filter="fourier_conv", seam="fused", **_HEAD)),
    "glstm_gconv_cheby": ("GLSTMGconvModel", dict(filter="cheby_conv", **_HEAD)),
}


def resgnn_case():
    """(L, x [N, M, Fin], labels [N, M, Fout]) of the golden steps."""
    import glstm_gconv_ref as GR
    c = CASE
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((c["N"], c["M"], c["Fin"])).astype(np.float32)
    labels = rng.standard_normal((c["N"], c["M"], c["Fout"])).astype(np.float32)
    return GR.ring_chords_laplacian(c["M"]), x, labels


@functools.lru_cache(maxsize=None)
def model_case():
    """(L, x [N, M, F*T], labels [N, M, Fout]) of the model goldens; every case
    reads the same six input channels.  Cached: a model's Chebyshev plan lives
    as long as the Laplacian object it was built from."""
    import glstm_gconv_ref as GR
    c = MODEL
    rng = np.random.default_rng(2025)
    x = (0.5 * rng.standard_normal((c["N"], c["M"], c["F"] * c["T"]))).astype(np.float32)
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


def build_model(name, dev):
    """A fresh model of MODEL_CASES[name] on ``dev``."""
    from cnn_graph_amd.gconv_lstm import GLSTMModel
    from cnn_graph_amd.glstm_gconv import GLSTMGconvModel
    from cnn_graph_amd.model import StackedResGNN
    c = MODEL
    cls, kw = MODEL_CASES[name]
    common = dict(decay_steps=c["decay_steps"], decay_rate=c["decay_rate"], device=dev, seed=c["seed"])
    L = model_case()[0]
    if cls == "StackedResGNN":
        return StackedResGNN(L, c["N"], c["F"] * c["T"], c["C"], 3, 1, groups=((0, 4), (4, 6)),
                             Fout_last=c["Fout"], **common, **kw)
    ctor = GLSTMModel if cls == "GLSTMModel" else GLSTMGconvModel
    return ctor(L, c["N"], c["T"], c["F"], out_features=c["Fout"], **common, **kw)


def run_model_steps(name):
    """(flat, loss, ema) after MODEL['steps'] steps of a fresh MODEL_CASES[name]."""
    import torch
    dev = torch.device("cuda", 0)
    m = build_model(name, dev)
    _, x, labels = model_case()
    xt, lt = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    for _ in range(MODEL["steps"]):
        loss = m.train_step(xt, lt)
    torch.cuda.synchronize()
    assert m.step_count == MODEL["steps"]
    return m.flat.detach().cpu().numpy(), loss.cpu().numpy(), m.ema.cpu().numpy()


if __name__ == "__main__":
    out = {}
    if sys.argv[1] == "--models":
        for name in MODEL_CASES:
            out[f"{name}_flat"], out[f"{name}_loss"], out[f"{name}_ema"] = run_model_steps(name)
    else:
        for f in ("chebyshev5", "fourier"):
            out[f"{f}_flat"], out[f"{f}_loss"] = run_steps(f)
    np.savez(sys.argv[-1], **out)
    print({k: v.shape for k, v in out.items()})
