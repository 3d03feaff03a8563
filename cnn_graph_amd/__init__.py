"""cnn_graph_amd -- MI355X-native Chebyshev spectral graph convolution.

A drop-in for the hot path of xu-wang11/cnn_graph: ``GraphConv.chebyshev5`` /
``cgcnn.chebyshev5`` / ``filter.cheby_conv`` (lib/graph_conv.py:144-176), with
the K-step recurrence, the weight contraction and the backward as hand-written
HIP kernels for gfx950 behind a C ABI (include/cheb_mi355.h), plus the graph
pooling / permutation ops around it and data-parallel gradient exchange.

Modules
  graph       host Laplacian math (lib/graph.py API)
  plan        device plan of L~ (the TF graph constant of lib/graph_conv.py:148-153)
  ops         torch autograd ops over the HIP kernels
  graph_conv  GraphConv filter plumbing (name-bound chebyshev5, residual stack)
  filter      functional cheby_conv (lib/filter.py API)
  coarsening  graph coarsening + perm_data (lib/coarsening.py API)
  dist        one-process-per-GPU data parallelism (RCCL all-reduce)
  glstm_period  GLSTMPeriodModel: the closeness / period / trend gconv-LSTM networks
  gconv_net   GConvNetModel: the pure graph-convolution networks (inference_gconv*)
  cgcnn       CGCNNModel: the pooled cgcnn classifier (lib/models.py), trained on device
  dense_rnn   LSTMRNNModel: the dense LSTM baseline of gconvRNN.Model (model_type='lstm')
"""
__version__ = "0.1.0"

__all__ = ["graph", "plan", "ops", "graph_conv", "filter", "coarsening", "dist", "GLSTMPeriodModel",
           "GConvNetModel", "CGCNNModel", "LSTMRNNModel"]


def __getattr__(name):
    # the model class, imported on first use (importing the package stays free of torch)
    if name == "GLSTMPeriodModel":
        from .glstm_period import GLSTMPeriodModel
        return GLSTMPeriodModel
    if name == "GConvNetModel":
        from .gconv_net import GConvNetModel
        return GConvNetModel
    if name == "CGCNNModel":
        from .cgcnn import CGCNNModel
        return CGCNNModel
    if name == "LSTMRNNModel":
        from .dense_rnn import LSTMRNNModel
        return LSTMRNNModel
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
