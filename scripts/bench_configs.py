#!/usr/bin/env python3
"""Timing of the non-headline configurations of SURVEY.md §8d on one GPU
(bench.py measures the headline config B).  One JSON line per config:

  C1  20NEWS-like 10k-vertex graph, layer 1: N=128, Fin=1, K=5, Fout=32
  C2  same graph, layer 2:                  N=128, Fin=32, K=5, Fout=32
  D   Chung-Lu 2^18 vertices, nnz 4.19M:    N=--d-batch (default 32), Fin=Fout=64, K=3
  E   gconv-LSTM layer on grid(32) 8-NN:    T=12, N=128, Fin=2, H=32, K=3 (fwd+bwd, BPTT)
  EF  the same layer with the Fourier filter (filter_type="fourier_conv"): hconv="fused"
      against hconv="unfused", the h-step's launches and the transforms' share of peak
  RF  the ResGNN training step with the Fourier filter at the reference's published shape
      (M=1024, batch 100, 10 channels, nfilter 32, 4 residual layers) against forward +
      backward of the same network on the older unfused ops under autograd
  S   the gconvRNN sequence model at config E's graph and shape (T=12, N=128, Fin=2, H=32,
      K=3, keep 0.8): the fused per-step softmax head against its composition from
      ops.dropout and torch ops, and the training step with each seam

  SL  the dense LSTM baseline (dense_rnn.LSTMRNNModel) at N=512, T=12, C=1024, H=32 and 128:
      the training step over the two one-launch sequence kernels (path "seq") against the
      per-step composition from cg_gemm_f32 and cg_lstm_cell_* (path "steps"), interleaved

  EP  the closeness / period / trend step (glstm_period.GLSTMPeriodModel) on config E's
      graph: N=50, T=(3, 3, 3), K=2, at H=128 with fourier_conv and H=32 with cheby_conv,
      in both merge modes; and the two seams alone against their composition from
      existing ops

  GC  the training step of the three pure graph-convolution networks (gconv_net.
      GConvNetModel: inference_gconv, ..._period_no_expand, ..._period_expand) on config E's
      graph at the driver's shape (batch 100, T=(3, 3, 3), num_hidden 64, K=2, 4 residual
      layers, out 2) against the same network composed from ops.cheb_conv + add +
      ops.bias_act under autograd, interleaved

  CG  the training step of the pooled cgcnn classifier (cgcnn.CGCNNModel) at usage.ipynb's
      network (F [32, 64], K [20, 20], p [4, 2], M [512, 10], batch 100) on the MNIST pyramid
      of golden_B, against GraphConv.cgcnn_inference under torch autograd with
      torch.nn.functional.cross_entropy and torch.optim.SGD(momentum, weight_decay), interleaved

  FIT the training loop around a step: ResGNN at config R's shape and GLSTMModel at config
      E's model step, 2 048 synthetic samples on the device -- (a) train_step on one static
      batch (the floor), (b) the loop a user writes without fit, train_step(data[i],
      labels[i]) with a device index tensor, (c) fit's inner loop (cg_batch_gather +
      train_step); HIP events over 200 steps, interleaved repeats

fwd / bwd are HIP-event timings (torch's current stream, where every C-ABI
call is enqueued) of one chebyshev5 forward and backward (dx + dW), median of
rounds; alg_GBps uses SURVEY.md §8d's algorithmic bytes.  Each line carries a
`cpu_baseline`: the oracle's fwd+bwd of the same config on the host cores
(bench.py's CPU legs -- the only place outside tests/ that runs oracle/),
median of the timed passes, with the sub-batch and pass count stated.
Usage: python scripts/bench_configs.py [A C1 C2 CG D E EF EP FIT GC R RF S SL] [--d-batch N] [--layout auto|rows|planes]
                                       [--no-cpu] [--cpu-seconds S]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench  # noqa: E402  (the CPU legs)
from cnn_graph_amd import ops  # noqa: E402
from cnn_graph_amd.plan import ChebPlan  # noqa: E402


ROUNDS = 3


def ev_ms(fn, reps=5, rounds=None):
    rounds = ROUNDS if rounds is None else rounds
    vals = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        vals.append(e0.elapsed_time(e1) / reps)
    return float(np.median(vals))


def alg_bytes(M, nnz, B, K):
    csr = 8 * nnz + 4 * (M + 1)
    return (K - 1) * csr + 4 * M * B * (2 + 3 * (K - 2)), (K - 1) * csr + 4 * M * B * (3 + 5 * (K - 2))


def filter_config(name, Lt, N, Fin, K, Fout, dev, variant="auto", layout="auto", copy_x=False):
    M = Lt.shape[0]
    plan = ChebPlan(Lt, device=0, variant=variant)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.rand((N, M, Fin), device=dev, generator=g)
    W = torch.randn((Fin * K, Fout), device=dev, generator=g) * 0.1
    dy = torch.randn((N, M, Fout), device=dev, generator=g)
    if layout == "auto":  # what the autograd layers use (ops.basis_layout_for)
        layout = ops.basis_layout_for(plan, N, Fin, K, Fout)
    if layout != "rows" and plan.basis_elems(N, Fin, K, Fout, layout) is None:
        return None  # the layout does not apply to this shape
    r = ops.ChebRunner(plan, N, Fin, K, Fout, dev, basis_layout=layout)
    x_in = "separate buffer (copied into plane 0)" if layout == "planes" else "separate buffer"
    if layout == "planes" and not copy_x:  # the input lives in plane 0: no copy of x
        r.input_plane().copy_(x)
        x = r.input_plane()
        x_in = "plane 0 of the basis (T_0 read in place)"
    r.forward(x, W)
    r.backward(dy, W)
    torch.cuda.synchronize()
    reps = 5 if M * N * Fin > 1e8 else 20
    f = ev_ms(lambda: r.forward(x, W), reps)
    b = ev_ms(lambda: r.backward(dy, W), reps)
    bf, bb = alg_bytes(M, plan.nnz, N * Fin, K)
    return {"config": name, "M": M, "nnz": plan.nnz, "N": N, "Fin": Fin, "K": K, "Fout": Fout,
            "path": r.path, "variant": variant, "basis_layout": layout, "input": x_in,
            "fwd_ms": round(f, 4), "bwd_ms": round(b, 4),
            "samples_per_s": round(N / ((f + b) * 1e-3), 1),
            "fwd_alg_GBps": round(bf / (f * 1e-3) / 1e9, 1),
            "bwd_alg_GBps": round(bb / (b * 1e-3) / 1e9, 1)}


def graph_e():
    """config E's grid graph: (L~, L = L~ + I so that rescale_L(L, 2) = L~)."""
    with np.load(os.path.join(ROOT, "tests", "golden", "golden_E.npz"), allow_pickle=False) as z:
        M = int(z["M"])
        Lt = scipy.sparse.csr_matrix((z["Lt_val"], z["Lt_col"], z["Lt_rowptr"]), shape=(M, M))
    return Lt, (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr()


def lstm_config(dev, T=12, N=128, Fin=2, H=32, K=3, hconv="auto"):
    from cnn_graph_amd.gconv_lstm import GConvLSTMCell, layer
    with np.load(os.path.join(ROOT, "tests", "golden", "golden_E.npz"), allow_pickle=False) as z:
        M = int(z["M"])
        Lt = scipy.sparse.csr_matrix((z["Lt_val"], z["Lt_col"], z["Lt_rowptr"]), shape=(M, M))
    # L = L~ + I  (rescale_L(L, 2) = L - I gives back this L~)
    L = (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr()
    cell = GConvLSTMCell(H, laplacian=L, lmax=2, K=K, feat_in=Fin, device=dev, hconv=hconv)
    M = L.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    xs = torch.rand((T, N, M, Fin), device=dev, generator=g)
    gh = torch.randn((T, N, M, H), device=dev, generator=g)

    def fwd():
        with torch.no_grad():
            layer(cell, xs)

    def fwdbwd():
        hs, _ = layer(cell, xs)
        hs.backward(gh)

    fwdbwd()
    torch.cuda.synchronize()
    f = ev_ms(fwd, 3)
    fb = ev_ms(fwdbwd, 3)
    return {"config": "E", "hconv": "seq" if cell.seq else "fused" if cell.fused else "unfused",
            "M": M, "T": T, "N": N, "Fin": Fin, "H": H, "K": K,
            "fwd_ms": round(f, 3), "fwd_bwd_ms": round(fb, 3),
            "samples_per_s": round(N / (fb * 1e-3), 1)}


F32_MATRIX_PEAK = 155e12  # measured v_mfma_f32_32x32x2_f32 rate; the x3 roof is 2.7x it


def flstm_config(dev, T=12, N=128, Fin=2, H=32, samples=8):
    """EF: one gconv-LSTM layer with the Fourier filter on config E's grid graph,
    forward + backward.  hconv="fused" against hconv="unfused" (the composition
    of ops.fourier_conv and the pointwise gate kernel: code that predates the
    fused path, the baseline), alternating, one event pair per pass; plus the
    three launches of the h-step and the transforms' share of the matrix peaks."""
    from cnn_graph_amd.gconv_lstm import GConvLSTMCell, layer
    _, L = graph_e()
    M = L.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    cells = {h: GConvLSTMCell(H, laplacian=L, lmax=2, feat_in=Fin, device=dev, hconv=h,
                              filter_type="fourier_conv") for h in ("fused", "unfused")}
    xs = torch.rand((T, N, M, Fin), device=dev, generator=g)
    gh = torch.randn((T, N, M, H), device=dev, generator=g)

    def fwdbwd(cell):
        hs, _ = layer(cell, xs)
        hs.backward(gh)
        for p in cell.parameters():
            p.grad = None

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for c in cells.values():  # warm every shape of the timed window
        fwdbwd(c)
        fwdbwd(c)
    torch.cuda.synchronize()
    ms = {h: [] for h in cells}
    for _ in range(samples):  # alternate the two legs
        for h, c in cells.items():
            ms[h].append(one(lambda: fwdbwd(c)))
    stat = {h: [float(np.percentile(v, q)) for q in (50, 10, 90)] for h, v in ms.items()}
    # the h-step's launches and the backward's wide analysis, alone
    cell = cells["fused"]
    B = cell.gft_basis
    f32 = dict(device=dev, dtype=torch.float32)
    h_prev, c_prev = torch.randn((N, M, H), generator=g, **f32), torch.randn((N, M, H), generator=g, **f32)
    ghx = torch.randn((N, M, 4 * H), generator=g, **f32) * 0.1
    hhat, gsum = ops.gft(B, h_prev), torch.empty((N, M, 4 * H), **f32)
    co, ho, act = (torch.empty(s, **f32) for s in ((N, M, H), (N, M, H), (N, M, 4 * H)))
    launches = {
        "analysis_H": lambda: ops.gft(B, h_prev, out=hhat),
        "mix_accumulate": lambda: ops.fourier_mix("fwd", cell.Wh, x=hhat, add=ghx, out=gsum),
        "synthesis_gates": lambda: ops.flstm_step(B, None, c_prev, gsum, None, cell.b, out_c=co,
                                                  out_h=ho, out_act=act),
        "analysis_4H": lambda: ops.gft(B, ghx, out=gsum),
    }
    lt = {}
    for name, fn in launches.items():
        fn()
        torch.cuda.synchronize()
        lt[name] = ev_ms(fn, 10)
    flop = {"analysis_H": 2.0 * M * M * N * H, "synthesis_gates": 2.0 * M * M * N * 4 * H,
            "analysis_4H": 2.0 * M * M * N * 4 * H}
    tflops = {k: flop[k] / (lt[k] * 1e-3) / 1e12 for k in flop}
    # transform FLOP of a layer's forward + backward (xs needs no gradient)
    layer_flop = 2.0 * M * M * N * (T * Fin + (T - 1) * H + T * 4 * H + T * 4 * H + (T - 1) * H)
    f, u = stat["fused"], stat["unfused"]
    from cnn_graph_amd import _lib
    return {"config": "EF", "M": M, "T": T, "N": N, "Fin": Fin, "H": H, "samples": samples,
            "gemm_x3": _lib.get_option("gemm_x3"),
            "fused_ms": round(f[0], 3), "fused_p10_p90": [round(f[1], 3), round(f[2], 3)],
            "unfused_ms": round(u[0], 3), "unfused_p10_p90": [round(u[1], 3), round(u[2], 3)],
            "ratio_unfused_over_fused": round(u[0] / f[0], 3),
            "fused_wins_by_more_than_baseline_spread": bool(u[0] - f[0] > u[2] - u[1]),
            "launch_ms": {k: round(v, 4) for k, v in lt.items()},
            "transform_TFLOPs": {k: round(v, 1) for k, v in tflops.items()},
            "transform_frac_f32_matrix_peak": {k: round(v * 1e12 / F32_MATRIX_PEAK, 3)
                                               for k, v in tflops.items()},
            "transform_frac_x3_roof": {k: round(v * 1e12 / (2.7 * F32_MATRIX_PEAK), 3)
                                       for k, v in tflops.items()},
            "layer_transform_GFLOP": round(layer_flop / 1e9, 1),
            "layer_transform_TFLOPs_end_to_end": round(layer_flop / (f[0] * 1e-3) / 1e12, 1)}


def resgnn_config(dev, N=100, Fin=2, nfilter=32, K=20, nres=4):
    """ResGNN training step (§8f-1, lib/graph_model.py:246-310 with
    lib/graph_conv.py:305-330): the humanflow-ln-period shape (M = 1024,
    nfilter 32, 4 residual layers, K 20, batch 100) on config E's
    1024-vertex graph -- 2*nres + 2 = 10 chebyshev5 calls per forward, the
    hidden ones with Fin = Fout = 32 (streaming path)."""
    from cnn_graph_amd.model import ResGNN
    with np.load(os.path.join(ROOT, "tests", "golden", "golden_E.npz"), allow_pickle=False) as z:
        M = int(z["M"])
        Lt = scipy.sparse.csr_matrix((z["Lt_val"], z["Lt_col"], z["Lt_rowptr"]), shape=(M, M))
    L = (Lt + scipy.sparse.identity(M, dtype=np.float32, format="csr")).tocsr()
    model = ResGNN(L, N=N, Fin=Fin, nfilter=nfilter, K=K, nres_layer_count=nres, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x = torch.rand((N, M, Fin), device=dev, generator=g)
    labels = torch.rand((N, M, 2), device=dev, generator=g)
    paths = sorted({model.plan.query_path(N, fi, K, fo) for fi, fo in
                    ((Fin, nfilter), (nfilter, nfilter), (nfilter, 2))})
    ms = ev_ms(lambda: model.train_step(x, labels), reps=5)
    return {"config": "R", "M": M, "N": N, "Fin": Fin, "nfilter": nfilter, "K": K,
            "nres_layer_count": nres, "filter_calls_per_step": 2 * nres + 2, "paths": paths,
            "step_ms": round(ms, 3), "samples_per_s": round(N / (ms * 1e-3), 1)}


PUBLISHED_RF_MS = 222.8  # nips2016/humanflow-ln-period.ipynb: 22.28 s per 100 steps


def resgnn_fourier_config(dev, N=100, Fin=10, nfilter=32, nres=4, samples=8):
    """RF: the reference's published ResGNN runs (params['filter'] = 'fourier',
    M = 1024, batch 100, 10 input channels, nfilter 32, 4 residual layers,
    Fout_last 2) on config R's graph recipe.  The training step of
    ResGNN(filter="fourier") and, interleaved in the same process, forward +
    backward of the same network composed from the older unfused ops
    (GraphConv(filter="fourier") under autograd: no loss kernel, no Adam), one
    event pair per pass; plus the transform launches at the hidden-layer shape."""
    from cnn_graph_amd import _lib
    from cnn_graph_amd.graph_conv import GraphConv
    from cnn_graph_amd.model import ResGNN
    _, L = graph_e()
    M = L.shape[0]
    model = ResGNN(L, N=N, Fin=Fin, nfilter=nfilter, K=20, nres_layer_count=nres, device=dev,
                   filter="fourier")
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x = torch.rand((N, M, Fin), device=dev, generator=g)
    labels = torch.rand((N, M, 2), device=dev, generator=g)
    nets = {}
    for key, fused in (("unfused", False), ("fused_autograd", True)):
        gc = GraphConv(filter="fourier", device=dev, fourier_fused=fused)
        gc.residual_network(x, L, nfilter, 20, nres, Fout_last=2)
        with torch.no_grad():
            for name, w in model.parameters().items():
                gc.weights[name].copy_(w)
        nets[key] = gc

    def fwdbwd(gc):
        out = gc.residual_network(x, L, nfilter, 20, nres, Fout_last=2)
        out.backward(labels)
        for p in gc.parameters():
            p.grad = None

    legs = {"step": lambda: model.train_step(x, labels),
            "unfused": lambda: fwdbwd(nets["unfused"]),
            "fused_autograd": lambda: fwdbwd(nets["fused_autograd"])}

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for fn in legs.values():  # warm every shape of the timed window
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(samples):  # alternate the legs
        for k, fn in legs.items():
            ms[k].append(one(fn))
    stat = {k: [float(np.percentile(v, q)) for q in (50, 10, 90)] for k, v in ms.items()}
    # the transforms of a hidden filter (C = nfilter), alone
    f32 = dict(device=dev, dtype=torch.float32)
    B, F = model.gft, nfilter
    a, b, c = (torch.randn((N, M, F), generator=g, **f32) for _ in range(3))
    W = model.W[1]
    y, xh, dz = (torch.empty((N, M, F), **f32) for _ in range(3))
    dW = torch.empty_like(W)
    launches = {
        "analysis": lambda: ops.gft(B, a, out=xh),
        "mix": lambda: ops.fourier_mix("fwd", W, x=xh, out=y),
        "forward_3_launches": lambda: ops.fres_forward(B, W, a, b, "relu", out_xhat=xh, out_y=y),
        "backward_4_launches": lambda: ops.fres_backward(B, W, xh, c, y, "relu", dx=a, out_dz=dz,
                                                         out_dW=dW),
    }
    lt = {}
    for name, fn in launches.items():
        fn()
        torch.cuda.synchronize()
        lt[name] = ev_ms(fn, 10)
    flop = 2.0 * M * M * N * F  # one transform at C = nfilter
    synth_ms = lt["forward_3_launches"] - lt["analysis"] - lt["mix"]
    tf = {"analysis": flop / (lt["analysis"] * 1e-3) / 1e12,
          "synthesis_act_by_difference": flop / (max(synth_ms, 1e-6) * 1e-3) / 1e12}
    # transform FLOP of a training step: 2 per filter forward, 2 per backward (1 without dx)
    chans = [(Fin, F)] + [(F, F)] * (2 * nres) + [(F, 2)]
    step_flop = sum(2.0 * M * M * N * (fi + fo) * 2 for fi, fo in chans) - 2.0 * M * M * N * Fin
    s, u, fa = stat["step"], stat["unfused"], stat["fused_autograd"]
    return {"config": "RF", "M": M, "N": N, "Fin": Fin, "nfilter": F, "nres_layer_count": nres,
            "samples": samples, "gemm_x3": _lib.get_option("gemm_x3"),
            "filter_calls_per_step": 2 * nres + 2,
            "step_ms": round(s[0], 3), "step_p10_p90": [round(s[1], 3), round(s[2], 3)],
            "samples_per_s": round(N / (s[0] * 1e-3), 1),
            "unfused_fwd_bwd_ms": round(u[0], 3),
            "unfused_p10_p90": [round(u[1], 3), round(u[2], 3)],
            "fused_autograd_fwd_bwd_ms": round(fa[0], 3),
            "fused_autograd_p10_p90": [round(fa[1], 3), round(fa[2], 3)],
            "ratio_unfused_over_step": round(u[0] / s[0], 3),
            "published_step_ms_unknown_gpu_one_evaluation_included": PUBLISHED_RF_MS,
            "launch_ms": {k: round(v, 4) for k, v in lt.items()},
            "transform_TFLOPs": {k: round(v, 1) for k, v in tf.items()},
            "transform_frac_x3_roof": {k: round(v * 1e12 / (2.7 * F32_MATRIX_PEAK), 3)
                                       for k, v in tf.items()},
            "step_transform_GFLOP": round(step_flop / 1e9, 1),
            "step_transform_TFLOPs_end_to_end": round(step_flop / (s[0] * 1e-3) / 1e12, 1)}


def glstm_gconv_config(dev, filter="fourier_conv", T=6, N=50, Fin=2, H=128, C=32, K=2, nres=2,
                       runs=5):
    """EG: one GLSTMGconvModel training step at the shape nips2016/gconvTest.py
    runs (config E's 32 x 32 grid graph, batch 50, filter_num 128,
    num_hidden_conv 32, kernel_num 2, keep 0.8).  With the Fourier filter the
    step is timed for seam "fused" and "unfused" (the latter entirely kernels
    that predate the seam calls) in INTERLEAVED runs: per-run numbers, the
    medians and the unfused range, which is what "auto" is decided on."""
    from cnn_graph_amd.glstm_gconv import GLSTMGconvModel
    _, L = graph_e()
    M = L.shape[0]
    seams = ("fused", "unfused") if filter == "fourier_conv" else ("unfused",)
    models = {s: GLSTMGconvModel(L, N, T, Fin, num_hidden=H, num_hidden_conv=C, K=K, layer_count=1,
                                 conv_layer_num=nres, keep_prob=0.8, filter=filter, seam=s, device=dev)
              for s in seams}
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    x = 0.5 * torch.randn((N, M, Fin * T), device=dev, generator=g)
    labels = torch.randn((N, M, 2), device=dev, generator=g)
    for m in models.values():  # warm every shape of the timed window
        for _ in range(3):
            m.train_step(x, labels)
    torch.cuda.synchronize()
    per_run = {s: [] for s in seams}
    for _ in range(runs):
        for s in seams:  # interleaved: drift hits both alike
            per_run[s].append(round(ev_ms(lambda: models[s].train_step(x, labels), 5), 4))
    out = {"config": "EG", "filter": filter, "M": M, "T": T, "N": N, "Fin": Fin, "H": H, "C": C, "K": K,
           "conv_layer_num": nres, "keep_prob": 0.8, "runs_ms": per_run,
           "median_ms": {s: round(float(np.median(v)), 4) for s, v in per_run.items()}}
    if len(seams) == 2:
        lo, hi = min(per_run["unfused"]), max(per_run["unfused"])
        out["unfused_range_ms"] = [lo, hi]
        out["fused_below_unfused_range"] = bool(out["median_ms"]["fused"] < lo)
    out["samples_per_s"] = round(N / (min(out["median_ms"].values()) * 1e-3), 1)
    return out


def period_config(dev, N=50, T=(3, 3, 3), Fin=2, K=2, keep=0.8, runs=5):
    """EP: (a) one GLSTMPeriodModel training step on config E's graph at the
    driver's width (H = 128, fourier_conv) and at H = 32 with cheby_conv, merge by
    weights (inference_glstm_period_expand) and by concat (..._expand_gconv3);
    (b) the two seams alone, forward + backward, against their composition from
    existing ops: torch mul / add plus one sum over n for the merge at [N, M, 2],
    ops.dropout x B plus torch.cat (and its autograd) for the concat at H per
    branch.  HIP events, the variants interleaved run by run; per-run numbers,
    medians and the composition's range."""
    from cnn_graph_amd.glstm_period import GLSTMPeriodModel
    _, L = graph_e()
    M, B = L.shape[0], len(T)
    g = torch.Generator(device=dev)
    g.manual_seed(8)
    modes = {"weights": "inference_glstm_period_expand", "concat": "inference_glstm_period_expand_gconv3"}
    x = 0.5 * torch.randn((N, M, Fin * sum(T)), device=dev, generator=g)
    labels = torch.randn((N, M, 2), device=dev, generator=g)
    models = {f"{filt}_H{H}_{mode}": GLSTMPeriodModel(L, N, T, Fin, num_hidden=H, K=K, layer_count=1,
                                                      conv_layer_num=1, keep_prob=keep, filter=filt,
                                                      infer_func=fn, device=dev)
              for filt, H in (("fourier_conv", 128), ("cheby_conv", 32)) for mode, fn in modes.items()}
    for m in models.values():
        for _ in range(3):
            m.train_step(x, labels)
    torch.cuda.synchronize()
    step = {k: [] for k in models}
    for _ in range(runs):
        for k, m in models.items():
            step[k].append(round(ev_ms(lambda: m.train_step(x, labels), 5), 4))
    out = {"config": "EP", "M": M, "N": N, "T": list(T), "Fin": Fin, "K": K, "keep_prob": keep,
           "step_runs_ms": step,
           "step_median_ms": {k: round(float(np.median(v)), 4) for k, v in step.items()}}

    # -- the seams alone ---------------------------------------------------------------------
    F = 2
    ys = [torch.randn((N, M, F), device=dev, generator=g) for _ in range(B)]
    ws = [torch.randn((M, F), device=dev, generator=g) for _ in range(B)]
    dout = torch.randn((N, M, F), device=dev, generator=g)

    def merge_kernel():
        ops.branch_merge_forward(ys, ws)
        return ops.branch_merge_backward(dout, ys, ws)

    def merge_composed():
        acc = ys[0] * ws[0]
        for y, w in zip(ys[1:], ws[1:]):
            acc = acc + y * w
        return [dout * w for w in ws], [(dout * y).sum(0) for y in ys]

    seeds = [11, 22, 33, 44][:B]
    seam = {}
    for H in (128, 32):
        hs = [torch.randn((N, M, H), device=dev, generator=g) for _ in range(B)]
        dx = torch.randn((N, M, B * H), device=dev, generator=g)

        def concat_kernel():
            ops.concat_drop_forward(hs, keep, seeds)
            return ops.concat_drop_backward(dx, [H] * B, keep, seeds)

        def concat_composed():
            leaves = [h.detach().requires_grad_() for h in hs]
            torch.cat([ops.dropout(h, keep, s) for h, s in zip(leaves, seeds)], dim=2).backward(dx)
            return [h.grad for h in leaves]

        pairs = {f"concat_H{H}": (concat_kernel, concat_composed)}
        if H == 128:
            pairs["merge"] = (merge_kernel, merge_composed)
        for name, (kern, comp) in pairs.items():
            for _ in range(3):
                kern(), comp()
            r = {"kernel": [], "composed": []}
            for _ in range(runs):
                r["kernel"].append(round(ev_ms(kern, 20), 4))
                r["composed"].append(round(ev_ms(comp, 20), 4))
            seam[name] = {"runs_ms": r, "median_ms": {k: round(float(np.median(v)), 4) for k, v in r.items()},
                          "composed_range_ms": [min(r["composed"]), max(r["composed"])],
                          "kernel_range_ms": [min(r["kernel"]), max(r["kernel"])]}
    out["seams_fwd_bwd"] = seam
    # bytes one kernel pass moves: merge fwd reads B y + B w, writes out; bwd reads dout, B y, B w,
    # writes B dy + B dw.  concat fwd / bwd: read and write the B branches once each
    out["merge_alg_bytes"] = 4 * ((B + 1) * N * M * F + B * M * F) + 4 * ((2 * B + 1) * N * M * F + 2 * B * M * F)
    out["concat_alg_bytes"] = {f"H{H}": 4 * 4 * B * N * M * H for H in (128, 32)}
    return out


def gconv_net_config(dev, N=100, T=(3, 3, 3), H=64, K=2, nres=4, out_f=2, runs=5):
    """GC: one GConvNetModel training step of each of the three pure graph-
    convolution networks at the driver's shape (nips2016/gconvTest.py: grid(32)
    8-NN, M = 1024, batch 100, T = (3, 3, 3) so C = 18, num_hidden 64, kernel_num
    2, conv_layer_num 4, out 2), against the same network composed from the
    unfused ops under autograd: ops.cheb_conv, a torch add for the residual,
    ops.bias_act for the activation, ops.mse_loss and one ops.adam_update per
    variable, on copies of the model's weights.  HIP events, fused and unfused
    interleaved run by run; per-run numbers, medians and the unfused range."""
    from cnn_graph_amd import gconv_net as GN
    _, L = graph_e()
    M = L.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(10)
    C = GN.FLOWS * sum(T)
    x = 0.5 * torch.randn((N, M, C), device=dev, generator=g)
    labels = torch.randn((N, M, out_f), device=dev, generator=g)
    legs = {}
    for fn in GN.INFER_FUNCS:
        model = GN.GConvNetModel(L, N, T=T, num_hidden=H, K=K, conv_layer_num=nres, out_features=out_f,
                                 infer_func=fn, device=dev)
        Ws = [w.detach().clone().requires_grad_() for w in model.W]
        slots = [(torch.zeros_like(w), torch.zeros_like(w)) for w in Ws]
        plan, per = model.plan, 2 * nres + 2
        count = [0]

        def act(v, a):
            return v if a == "none" else ops.bias_act(v, None, a)

        def net(h, ws, acts):
            a_init, a_res, a_last = acts
            h = act(ops.cheb_conv(h, ws[0], plan, K), a_init)
            for i in range(nres):
                t = act(ops.cheb_conv(h, ws[1 + 2 * i], plan, K), a_res)
                h = act(ops.cheb_conv(t, ws[2 + 2 * i], plan, K) + h, a_res)
            return act(ops.cheb_conv(h, ws[per - 1], plan, K), a_last)

        def unfused(fn=fn, Ws=Ws, slots=slots, net=net, count=count, model=model):
            if fn in GN.SINGLE:
                out = net(x, Ws, GN.SINGLE[fn])
            else:
                outs = [net(x[:, :, a:b].contiguous(), Ws[j * per:(j + 1) * per], GN.EXPAND_ACTS)
                        for j, (a, b) in enumerate(model.columns)]
                out = ops.cheb_conv(torch.cat(outs, dim=2), Ws[-1], plan, K)
            _, dout = ops.mse_loss(out, labels)
            out.backward(dout)
            count[0] += 1
            for w, (m, v) in zip(Ws, slots):
                ops.adam_update(w.data, w.grad, m, v, count[0])
                w.grad = None

        legs[fn] = (lambda model=model: model.train_step(x, labels), unfused)
    for fused, unf in legs.values():  # warm every shape of the timed window
        for _ in range(3):
            fused(), unf()
    torch.cuda.synchronize()
    res = {}
    for fn, (fused, unf) in legs.items():
        r = {"fused": [], "unfused": []}
        for _ in range(runs):
            r["fused"].append(round(ev_ms(fused, 5), 4))
            r["unfused"].append(round(ev_ms(unf, 5), 4))
        med = {k: round(float(np.median(v)), 4) for k, v in r.items()}
        res[fn] = {"runs_ms": r, "median_ms": med, "unfused_range_ms": [min(r["unfused"]), max(r["unfused"])],
                   "fused_range_ms": [min(r["fused"]), max(r["fused"])],
                   "fused_below_unfused_range": bool(med["fused"] < min(r["unfused"])),
                   "samples_per_s": round(N / (med["fused"] * 1e-3), 1)}
    return {"config": "GC", "M": M, "N": N, "T": list(T), "C": C, "H": H, "K": K, "conv_layer_num": nres,
            "out": out_f, "steps": res}


def cgcnn_config(dev, N=100, F=(32, 64), K=(20, 20), p=(4, 2), Mfc=(512, 10), reg=5e-4, keep=0.5,
                 runs=5):
    """CG: one CGCNNModel training step of usage.ipynb's network (F [32, 64], K
    [20, 20], p [4, 2], M [512, 10], batch 100, mpool1, b1relu, regularization
    5e-4, dropout 0.5, momentum 0.9) on the MNIST pyramid of golden_B, against
    the same network as GraphConv.cgcnn_inference under torch autograd with
    torch.nn.functional.cross_entropy and torch.optim.SGD(momentum 0.9,
    weight_decay on the fc / logits variables) -- the composition has no
    dropout (cgcnn_inference applies none), so it does less.  HIP events, the
    two interleaved run by run; per-run numbers, medians and ranges."""
    from cnn_graph_amd import CGCNNModel, coarsening, graph
    from cnn_graph_amd.graph_conv import GraphConv
    with np.load(os.path.join(ROOT, "tests", "golden", "golden_B.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    A = scipy.sparse.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=tuple(g["A_shape"]))
    graphs, perm = coarsening.coarsen(A, 4, rids=[g[f"rid{i}"] for i in range(4)], verbose=False)
    L = [graph.laplacian(G, normalized=True) for G in graphs]
    rng = np.random.default_rng(3)
    x = torch.from_numpy(coarsening.perm_data(rng.random((N, A.shape[0])), perm).astype(np.float32)).to(dev)
    labels_h = rng.integers(0, Mfc[-1], N)
    labels = ops.class_labels(labels_h, Mfc[-1], dev)
    labels64 = labels.long()
    model = CGCNNModel(L, N, list(F), list(K), list(p), list(Mfc), regularization=reg, dropout=keep,
                       learning_rate=0.02, decay_rate=0.95, decay_steps=550, momentum=0.9, device=dev)
    gc = GraphConv(filter="chebyshev5", brelu="b1relu", pool="mpool1", device=dev)
    gc.cgcnn_inference(x, L, F, K, p, Mfc)  # creates the variables
    conv = [w for n, w in gc.weights.items() if n.startswith("conv")]
    dense = [w for n, w in gc.weights.items() if not n.startswith("conv")]
    opt = torch.optim.SGD([{"params": conv, "weight_decay": 0.0}, {"params": dense, "weight_decay": reg}],
                          lr=0.02, momentum=0.9)

    def autograd_step():
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(gc.cgcnn_inference(x, L, F, K, p, Mfc), labels64)
        loss.backward()
        opt.step()

    def device_step():
        model.train_step(x, labels)

    for _ in range(3):
        device_step(), autograd_step()
    torch.cuda.synchronize()
    r = {"device": [], "autograd": []}
    for _ in range(runs):
        r["device"].append(round(ev_ms(device_step, 5), 4))
        r["autograd"].append(round(ev_ms(autograd_step, 5), 4))
    med = {k: round(float(np.median(v)), 4) for k, v in r.items()}
    return {"config": "CG", "M": [int(l.shape[0]) for l in L], "N": N, "F": list(F), "K": list(K),
            "p": list(p), "M_fc": list(Mfc), "params": int(model.flat.numel()),
            "runs_ms": r, "median_ms": med,
            "device_range_ms": [min(r["device"]), max(r["device"])],
            "autograd_range_ms": [min(r["autograd"]), max(r["autograd"])],
            "device_below_autograd_range": bool(med["device"] < min(r["autograd"])),
            "samples_per_s": round(N / (med["device"] * 1e-3), 1)}


def seq_head_config(dev, T=12, N=128, Fin=2, H=32, K=3, keep=0.8, runs=5):
    """S: the gconvRNN sequence model (gconv_rnn.GConvRNNModel) at config E's
    graph and shape.  (a) the fused head (cg_seq_xent_head: mask, logits,
    softmax loss and every gradient in one pass over hs [T, N, M, H]) against
    the same math composed from ops.dropout and torch's matmul / log_softmax /
    autograd -- the baseline; (b) one training step with each seam.  HIP events,
    the variants interleaved run by run; per-run numbers, medians and the
    unfused range that ``seam="auto"`` is decided on."""
    from cnn_graph_amd.gconv_rnn import GConvRNNModel
    _, L = graph_e()
    M = L.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    hs = torch.randn((T, N, M, H), device=dev, generator=g).requires_grad_()
    w = torch.randn((H, 1), device=dev, generator=g).requires_grad_()
    b = torch.randn((1,), device=dev, generator=g).requires_grad_()
    lab_host = np.random.default_rng(7).integers(0, M, (T, N))
    lab = ops.seq_xent_labels(lab_host, M, dev)
    lab64 = lab.long()
    seed, scale = 0x5EED, 1.0 / T
    ws = torch.empty(ops.seq_xent_workspace_bytes(T, N, M, H), device=dev, dtype=torch.uint8)
    dhs, dw, db = torch.empty_like(hs), torch.empty((H,), device=dev), torch.empty((1,), device=dev)

    def fused():
        return ops.seq_xent_call(hs.detach(), w.detach(), b.detach(), lab, keep, seed, scale, ws=ws,
                                 out_dhs=dhs, out_dw=dw, out_db=db)

    def composed():
        for p in (hs, w, b):
            p.grad = None
        logits = (ops.dropout(hs, keep, seed) @ w).squeeze(-1) + b  # [T, N, M]
        ce = -torch.log_softmax(logits, dim=-1).gather(-1, lab64.unsqueeze(-1))
        loss = scale * ce.sum()
        loss.backward()
        return loss

    r, loss_c = fused(), composed()
    torch.cuda.synchronize()
    agree = {"loss_rel": abs(float(r.loss) - float(loss_c)) / abs(float(loss_c)),
             "dhs_normwise": float((r.dhs - hs.grad).abs().max() / hs.grad.abs().max()),
             "dw_normwise": float((r.dw - w.grad.view(-1)).abs().max() / w.grad.abs().max())}
    head = {"fused": [], "composed": []}
    for _ in range(3):
        fused(), composed()
    for _ in range(runs):
        head["fused"].append(round(ev_ms(fused, 10), 4))
        head["composed"].append(round(ev_ms(composed, 3), 4))
    del hs.grad, dhs
    tile = T * N * M * H * 4
    med = {k: float(np.median(v)) for k, v in head.items()}
    out = {"config": "S", "M": M, "T": T, "N": N, "Fin": Fin, "H": H, "K": K, "keep_prob": keep,
           "head_runs_ms": head, "head_median_ms": {k: round(v, 4) for k, v in med.items()},
           "head_speedup": round(med["composed"] / med["fused"], 2), "head_agreement": agree,
           # read hs once, write dhs once
           "head_alg_bytes": 2 * tile, "head_alg_GBps": round(2 * tile / (med["fused"] * 1e-3) / 1e9, 1),
           "head_share_of_8TBps": round(2 * tile / (med["fused"] * 1e-3) / 8e12, 3)}
    seams = ("fused", "unfused")
    models = {s: GConvRNNModel(L, N, T, Fin, num_hidden=H, K=K, keep_prob=keep, seam=s, device=dev)
              for s in seams}
    x = 0.5 * torch.randn((N, M, Fin, T), device=dev, generator=g)
    labels = torch.from_numpy(np.ascontiguousarray(lab_host.T)).to(dev)
    for m in models.values():
        for _ in range(3):
            m.train_step(x, labels)
    torch.cuda.synchronize()
    per_run = {s: [] for s in seams}
    for _ in range(runs):
        for s in seams:  # interleaved: drift hits both alike
            per_run[s].append(round(ev_ms(lambda: models[s].train_step(x, labels), 5), 4))
    lo, hi = min(per_run["unfused"]), max(per_run["unfused"])
    out.update({"step_runs_ms": per_run,
                "step_median_ms": {s: round(float(np.median(v)), 4) for s, v in per_run.items()},
                "unfused_range_ms": [lo, hi]})
    out["fused_below_unfused_range"] = bool(out["step_median_ms"]["fused"] < lo)
    out["samples_per_s"] = round(N / (min(out["step_median_ms"].values()) * 1e-3), 1)
    return out


def dense_lstm_config(dev, N=512, T=12, C=1024, hidden=(32, 128), keep=0.8, runs=5):
    """SL: the training step of the dense LSTM baseline (dense_rnn.LSTMRNNModel)
    with the recurrence on the two sequence launches (path "seq") and on the
    per-step composition of existing entries (path "steps": cg_gemm_f32 for
    h Wh plus cg_lstm_cell_forward / _backward, standard gates).  HIP events,
    the two paths interleaved run by run; per-run numbers, medians and ranges
    per H, and whether "seq" lies below the range of "steps" (the rule
    ``path="auto"`` is decided on: at BOTH H, by more than the spread)."""
    from cnn_graph_amd.dense_rnn import LSTMRNNModel
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    x = 0.5 * torch.randn((N, C, T), device=dev, generator=g)
    labels = torch.from_numpy(np.random.default_rng(7).integers(0, C, (N, T))).to(dev)
    out = {"config": "SL", "N": N, "T": T, "C": C, "keep_prob": keep, "runs": runs, "H": {}}
    paths = ("seq", "steps")
    for H in hidden:
        models = {p: LSTMRNNModel(N, T, C, num_hidden=H, keep_prob=keep, device=dev, path=p) for p in paths}
        losses = {}
        for p, m in models.items():
            for _ in range(3):
                losses[p] = m.train_step(x, labels)
        torch.cuda.synchronize()
        per_run = {p: [] for p in paths}
        for _ in range(runs):
            for p in paths:  # interleaved: drift hits both alike
                per_run[p].append(round(ev_ms(lambda: models[p].train_step(x, labels), 5), 4))
        med = {p: round(float(np.median(v)), 4) for p, v in per_run.items()}
        rng = {p: [min(v), max(v)] for p, v in per_run.items()}
        out["H"][str(H)] = {
            "step_runs_ms": per_run, "step_median_ms": med, "step_range_ms": rng,
            "loss_after_3_steps": {p: float(v) for p, v in losses.items()},
            "seq_below_steps_range": bool(rng["seq"][1] < rng["steps"][0]),
            "steps_below_seq_range": bool(rng["steps"][1] < rng["seq"][0]),
            "samples_per_s": {p: round(N / (v * 1e-3), 1) for p, v in med.items()}}
        del models
    out["seq_wins_at_every_H"] = all(v["seq_below_steps_range"] for v in out["H"].values())
    return out


def fit_config(dev, samples=2048, steps=200, runs=5):
    """FIT: what the loop around a training step costs.  Per model, on a
    synthetic dataset of ``samples`` samples that lives on the device and one
    seeded fit_schedule: (a) ``train_step`` on one static batch, the floor;
    (b) the loop a user writes without ``fit``, ``train_step(data[i], labels[i])``
    with i a device index tensor per step (made before the timed window);
    (c) ``fit``'s inner loop, one cg_batch_gather from the uploaded schedule
    into two fixed buffers and ``train_step`` on them.  HIP events around
    ``steps`` steps, the three loops interleaved run by run; per-run numbers,
    medians and ranges, per step."""
    from cnn_graph_amd import _lib
    from cnn_graph_amd.gconv_lstm import GLSTMModel
    from cnn_graph_amd.model import ResGNN
    from cnn_graph_amd.trainer import fit_schedule
    _, L = graph_e()
    M = L.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    gather = _lib.lib().cg_batch_gather
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"config": "FIT", "M": M, "samples": samples, "steps_per_run": steps, "runs": runs, "models": {}}
    builds = {
        "R_ResGNN": (100, 2, lambda: ResGNN(L, N=100, Fin=2, nfilter=32, K=20, nres_layer_count=4, device=dev)),
        "E_GLSTMModel": (128, 24, lambda: GLSTMModel(L, 128, T=12, feat_in=2, num_hidden=32, K=3, device=dev)),
    }
    for name, (N, C, build) in builds.items():
        model = build()
        data = 0.5 * torch.randn((samples, M, C), device=dev, generator=g)
        labels = torch.randn((samples, M * 2), device=dev, generator=g)
        sched = fit_schedule(samples, N, steps, 9)
        idx32 = torch.from_numpy(sched).to(dev)
        idx64 = [row for row in idx32.long()]  # one device index tensor per step
        x_b = torch.empty((N, M, C), device=dev)
        y_b = torch.empty((N, M, 2), device=dev)
        x0, y0 = data[:N].clone(), labels[:N].view(N, M, 2).clone()
        lab3 = labels.view(samples, M, 2)
        dp, lp, ip, xp, yp = (t.data_ptr() for t in (data, labels, idx32, x_b, y_b))
        row, lrow = M * C, M * 2

        def static():
            for _ in range(steps):
                model.train_step(x0, y0)

        def indexed():
            for i in idx64:
                model.train_step(data[i], lab3[i])

        def gathered():
            for k in range(steps):
                _lib.check("cg_batch_gather", gather(dp, lp, ip + 4 * N * k, N, samples, row, lrow, xp, yp, stream))
                model.train_step(x_b, y_b)

        loops = {"a_static_batch": static, "b_torch_indexing": indexed, "c_fit_gather": gathered}
        for fn in loops.values():  # warm every shape the timed windows use
            fn()
        torch.cuda.synchronize()
        per_run = {k: [] for k in loops}
        for _ in range(runs):
            for k, fn in loops.items():  # interleaved: drift hits all alike
                per_run[k].append(round(ev_ms(fn, 1, rounds=1) / steps * 1e3, 2))
        med = {k: round(float(np.median(v)), 2) for k, v in per_run.items()}
        rng = {k: [min(v), max(v)] for k, v in per_run.items()}
        out["models"][name] = {
            "N": N, "C": C, "batch_bytes": 4 * N * (row + lrow), "step_runs_us": per_run,
            "step_median_us": med, "step_range_us": rng,
            "c_minus_a_us": round(med["c_fit_gather"] - med["a_static_batch"], 2),
            "b_minus_a_us": round(med["b_torch_indexing"] - med["a_static_batch"], 2),
            "c_below_b_range": bool(rng["c_fit_gather"][1] < rng["b_torch_indexing"][0])}
        del model, data, labels
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C1", "C2", "D", "E"])
    ap.add_argument("--d-batch", type=int, default=32)
    ap.add_argument("--variant", default="auto", help="plan variant (auto / narrow / ...)")
    ap.add_argument("--layout", default="auto", choices=["auto", "rows", "planes"],
                    help="basis layout of the C1/C2/D filters (auto: the autograd layers' choice, "
                         "ops.basis_layout_for -- planes where it applies, else rows)")
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per measurement (median)")
    ap.add_argument("--opt", action="append", default=[],
                    help="kernel-selection option name=value (cg_set_option), e.g. dw_direct=3")
    ap.add_argument("--copy-x", action="store_true",
                    help="planes layout: keep x in its own buffer (the forward copies it into plane 0)")
    ap.add_argument("--filter", default="fourier_conv", choices=["fourier_conv", "cheby_conv"],
                    help="EG: the filter of the cells and the head")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline legs")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    args = ap.parse_args()
    global ROUNDS
    ROUNDS = args.rounds
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from cnn_graph_amd import _lib
    for kv in args.opt:
        name, val = kv.split("=")
        _lib.set_option(name, int(val))
    from cnn_graph_amd.graph import rescale_L
    for name in args.configs:
        cpu = None
        if name == "A":  # the usage recipe's 4-NN graph, M = 100
            with np.load(os.path.join(ROOT, "tests", "golden", "golden_A.npz"), allow_pickle=False) as z:
                M = int(z["M"])
                Lt = scipy.sparse.csr_matrix((z["Lt_val"], z["Lt_col"], z["Lt_rowptr"]), shape=(M, M))
            out = filter_config("A", Lt, 32, 1, 5, 4, dev, args.variant, args.layout, args.copy_x)
            cpu = lambda: bench.cpu_baseline_filter("A", Lt, 32, 32, 1, 5, 4,  # noqa: E731
                                                    seconds=args.cpu_seconds)
        elif name in ("C1", "C2"):
            with np.load(os.path.join(ROOT, "tests", "golden", "golden_C.npz"), allow_pickle=False) as z:
                M = int(z["M"])
                Lt = scipy.sparse.csr_matrix((z["Lt_val"], z["Lt_col"], z["Lt_rowptr"]), shape=(M, M))
            Fin = 1 if name == "C1" else 32
            out = filter_config(name, Lt, 128, Fin, 5, 32, dev, args.variant, args.layout, args.copy_x)
            # the oracle's C2 pass is ~27 s at N = 128: a sub-batch of 8
            nc = 128 if name == "C1" else 8
            cpu = lambda: bench.cpu_baseline_filter(name, Lt, nc, 128, Fin, 5, 32,  # noqa: E731
                                                    seconds=args.cpu_seconds,
                                                    warmup=10 if nc == 128 else 2)
        elif name == "D":
            import synth_graphs
            Lt = rescale_L(synth_graphs.config_d_laplacian(), 2)
            out = filter_config("D", Lt, args.d_batch, 64, 3, 64, dev, args.variant, args.layout, args.copy_x)
            cpu = lambda: bench.cpu_baseline_filter("D", Lt, 1, args.d_batch, 64, 3, 64,  # noqa: E731
                                                    seconds=args.cpu_seconds, warmup=1,
                                                    min_passes=3)
        elif name == "E":
            out = lstm_config(dev)
            cpu = lambda: bench.cpu_baseline_lstm(graph_e()[0], 8, 128, 12, 2, 32, 3,  # noqa: E731
                                                  seconds=args.cpu_seconds)
        elif name == "EF":
            out = flstm_config(dev)
        elif name == "E_unfused":
            out = lstm_config(dev, hconv="unfused")
        elif name == "E_step":
            out = lstm_config(dev, hconv="fused")
        elif name == "RF":
            out = resgnn_fourier_config(dev)
        elif name == "EG":
            out = glstm_gconv_config(dev, filter=args.filter)
        elif name == "S":
            out = seq_head_config(dev)
        elif name == "SL":
            out = dense_lstm_config(dev)
        elif name == "EP":
            out = period_config(dev)
        elif name == "FIT":
            out = fit_config(dev)
        elif name == "GC":
            out = gconv_net_config(dev)
        elif name == "CG":
            out = cgcnn_config(dev)
        elif name == "R":
            out = resgnn_config(dev)
            cpu = lambda: bench.cpu_baseline_resgnn(graph_e()[1], 2, 100, 2, 32, 20, 4,  # noqa: E731
                                                    seconds=args.cpu_seconds)
        else:
            raise SystemExit(f"unknown config {name}")
        if out is not None:
            if not args.no_cpu and cpu is not None:
                out["cpu_baseline"] = cpu()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
