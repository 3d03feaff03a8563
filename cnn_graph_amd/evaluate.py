"""``GraphModel.predict`` / ``GraphModel.evaluate`` (lib/graph_model.py:64-122) for
the device models: one helper behind ``GLSTMGconvModel``, ``GLSTMModel``,
``ResGNN`` and ``StackedResGNN``.

The training loop calls ``evaluate`` every ``eval_frequency`` steps
(lib/graph_model.py:167-171); both only run the model's forward (and the MSE
kernel when labels are given), under ``torch.no_grad()``: the parameters, the
optimizer slots, the loss moving average and the step count are not touched.
"""
from __future__ import annotations

import torch

from . import ops


def predict(forward, batch_size: int, device, data, labels=None):
    """lib/graph_model.py:64-94.  ``forward(batch [batch_size, M, C]) ->
    [batch_size, M, out]`` is the model's inference on one full batch.

    The data is walked in batches of ``batch_size``; the ragged last batch is
    zero-padded to it (:72-76) and its padded rows are not returned.  Returns
    the predictions [size, M, out] (a device tensor); with ``labels`` also the
    reference's ``loss * batch_size / size`` (:92) as a float, where ``loss`` is
    the PLAIN SUM of the per-batch mean losses -- each over a whole padded
    batch, so the zero rows of the last batch contribute (prediction of a zero
    input against zero labels) and a short last batch weighs as much as a full
    one.  That quirk is the reference's and is kept."""
    f32 = dict(device=device, dtype=torch.float32)
    data = torch.as_tensor(data).to(**f32)
    size, N = int(data.shape[0]), int(batch_size)
    if labels is not None:
        labels = torch.as_tensor(labels).to(**f32)
        if int(labels.shape[0]) != size:
            raise ValueError("data and labels differ in their number of samples")
    preds, loss = None, 0.0
    with torch.no_grad():
        for begin in range(0, size, N):
            end = min(begin + N, size)
            batch = data[begin:end]
            if end - begin < N:
                batch = torch.zeros((N,) + tuple(data.shape[1:]), **f32)
                batch[:end - begin] = data[begin:end]
            out = forward(batch.contiguous())
            if preds is None:
                preds = torch.empty((size,) + tuple(out.shape[1:]), **f32)
            if labels is not None:
                bl = labels[begin:end]
                if end - begin < N:
                    bl = torch.zeros(tuple(out.shape), **f32)
                    bl[:end - begin] = labels[begin:end].reshape((end - begin,) + tuple(out.shape[1:]))
                loss += float(ops.mse_loss(out, bl.contiguous(), need_grad=False)[0])
            preds[begin:end] = out[:end - begin]  # a copy: ``out`` may be a buffer the model reuses
    if labels is None:
        return preds
    return preds, loss * N / size


def evaluate(predict_fn, data, labels):
    """lib/graph_model.py:96-122: ``(string, mse, 0, loss, predictions)`` with
    ``mse = sum((labels - predictions)^2) / predictions.size`` (:116, summed in
    float64 as the reference's numpy does) and ``loss`` predict's."""
    preds, loss = predict_fn(data, labels)
    lab = torch.as_tensor(labels).to(device=preds.device, dtype=torch.float64).reshape(preds.shape)
    mse = float(((lab - preds.double()) ** 2).sum()) / preds.numel()
    string = "mse: {:.5f} ( {:d}), f1 (weighted), loss: {:.2e}".format(mse, len(labels), loss)
    return string, mse, 0, loss, preds
