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

branch_model_steps.npz (``--branch-models``): the same for ``BRANCH_CASES`` --
``GLSTMPeriodModel``, ``GConvNetModel`` (both on the eight channels of
``branch_case``, T = (2, 1, 1)) and ``GConvRNNModel`` (x [N, M, F, T], integer
labels [N, T]; flat and loss, it has no loss average) -- as the commit BEFORE the
models' shared pieces moved into ``trainer.py`` computed them.  Recorded twice,
in two processes; the two files were identical.

How they were generated: with the parent commit's package (its Python files and
its built libcheb_mi355.so) first on PYTHONPATH,

    PYTHONPATH=<parent checkout> python tests/golden/make_resgnn_steps.py OUT.npz
    PYTHONPATH=<parent checkout> python tests/golden/make_resgnn_steps.py --models OUT.npz
    PYTHONPATH=<parent checkout> python tests/golden/make_resgnn_steps.py --branch-models OUT.npz

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
# the branch models read C = 8 columns: T = (2, 1, 1) windows of F = 2 flows
BRANCH_T = (2, 1, 1)
_PERIOD = dict(T=BRANCH_T, feat_in=2, num_hidden=8, K=2, conv_layer_num=1, **_LSTM)
_NET = dict(T=BRANCH_T, num_hidden=8, K=2, conv_layer_num=1)
_RNN = dict(num_hidden=8, K=3, keep_prob=0.8)
BRANCH_CASES = {
    "period_expand_cheby": ("GLSTMPeriodModel", dict(infer_func="inference_glstm_period_expand",
                                                     filter="cheby_conv", **_PERIOD)),
    "period_expand_fourier": ("GLSTMPeriodModel", dict(infer_func="inference_glstm_period_expand",
                                                       filter="fourier_conv", **_PERIOD)),
    "period_gconv1_cheby": ("GLSTMPeriodModel", dict(infer_func="inference_glstm_period_expand_gconv1",
                                                     filter="cheby_conv", **_PERIOD)),
    "period_gconv3_cheby": ("GLSTMPeriodModel", dict(infer_func="inference_glstm_period_expand_gconv3",
                                                     filter="cheby_conv", **_PERIOD)),
    "period_gconv3_fourier": ("GLSTMPeriodModel", dict(infer_func="inference_glstm_period_expand_gconv3",
                                                       filter="fourier_conv", **_PERIOD)),
    "period_split_cheby": ("GLSTMPeriodModel", dict(infer_func="inference_glstm_gconv_split",
                                                    filter="cheby_conv", **_PERIOD)),
    "gconv_cheby": ("GConvNetModel", dict(infer_func="inference_gconv", filter="cheby_conv", **_NET)),
    "gconv_expand_cheby": ("GConvNetModel", dict(infer_func="inference_gconv_period_expand",
                                                 filter="cheby_conv", **_NET)),
    "gconv_no_expand_cheby": ("GConvNetModel", dict(infer_func="inference_gconv_period_no_expand",
                                                    filter="cheby_conv", **_NET)),
    "gconv_no_expand_fourier": ("GConvNetModel", dict(infer_func="inference_gconv_period_no_expand",
                                                      filter="fourier_conv", **_NET)),
    "rnn_fused_clip": ("GConvRNNModel", dict(seam="fused", max_grad_norm=0.05, **_RNN)),
    "rnn_unfused_clip": ("GConvRNNModel", dict(seam="unfused", max_grad_norm=0.05, **_RNN)),
    "rnn_adam": ("GConvRNNModel", dict(optimizer="adam", **_RNN)),
}
MODEL_CASES.update(BRANCH_CASES)


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


@functools.lru_cache(maxsize=None)
def branch_case():
    """(x [N, M, 8], labels [N, M, Fout], x_seq [N, M, F, T], vertex labels [N, T]
    int64) of BRANCH_CASES, on ``model_case``'s Laplacian."""
    c = MODEL
    rng = np.random.default_rng(2026)
    x = (0.5 * rng.standard_normal((c["N"], c["M"], c["F"] * sum(BRANCH_T)))).astype(np.float32)
    labels = rng.standard_normal((c["N"], c["M"], c["Fout"])).astype(np.float32)
    x_seq = (0.5 * rng.standard_normal((c["N"], c["M"], c["F"], c["T"]))).astype(np.float32)
    vertices = rng.integers(0, c["M"], size=(c["N"], c["T"]), dtype=np.int64)
    return x, labels, x_seq, vertices


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
    if cls == "GLSTMPeriodModel":
        from cnn_graph_amd.glstm_period import GLSTMPeriodModel
        return GLSTMPeriodModel(L, c["N"], out_features=c["Fout"], **common, **kw)
    if cls == "GConvNetModel":
        from cnn_graph_amd.gconv_net import GConvNetModel
        return GConvNetModel(L, c["N"], out_features=c["Fout"], **common, **kw)
    if cls == "GConvRNNModel":  # a constant learning rate: no decay to set
        from cnn_graph_amd.gconv_rnn import GConvRNNModel
        return GConvRNNModel(L, c["N"], c["T"], c["F"], device=dev, seed=c["seed"], **kw)
    if cls == "StackedResGNN":
        return StackedResGNN(L, c["N"], c["F"] * c["T"], c["C"], 3, 1, groups=((0, 4), (4, 6)),
                             Fout_last=c["Fout"], **common, **kw)
    ctor = GLSTMModel if cls == "GLSTMModel" else GLSTMGconvModel
    return ctor(L, c["N"], c["T"], c["F"], out_features=c["Fout"], **common, **kw)


def run_model_steps(name):
    """(flat, loss, ema) after MODEL['steps'] steps of a fresh MODEL_CASES[name]
    (GConvRNNModel's loss is not FlatTrainer's: its ema stays zero)."""
    import torch
    dev = torch.device("cuda", 0)
    m = build_model(name, dev)
    if name not in BRANCH_CASES:
        _, x, labels = model_case()
    elif MODEL_CASES[name][0] == "GConvRNNModel":
        x, labels = branch_case()[2:]
    else:
        x, labels = branch_case()[:2]
    xt, lt = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    for _ in range(MODEL["steps"]):
        loss = m.train_step(xt, lt)
    torch.cuda.synchronize()
    assert m.step_count == MODEL["steps"]
    return m.flat.detach().cpu().numpy(), loss.cpu().numpy(), m.ema.cpu().numpy()


if __name__ == "__main__":
    out = {}
    if sys.argv[1] in ("--models", "--branch-models"):
        for name in MODEL_CASES:
            if (name in BRANCH_CASES) != (sys.argv[1] == "--branch-models"):
                continue
            out[f"{name}_flat"], out[f"{name}_loss"], out[f"{name}_ema"] = run_model_steps(name)
    else:
        for f in ("chebyshev5", "fourier"):
            out[f"{f}_flat"], out[f"{f}_loss"] = run_steps(f)
    np.savez(sys.argv[-1], **out)
    print({k: v.shape for k, v in out.items()})
