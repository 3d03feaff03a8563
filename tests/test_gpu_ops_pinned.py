"""The LSTM, gradient, loss and flstm wrappers of cnn_graph_amd/ops.py refuse
what they refused and compute the bits they computed when
tests/golden/ops_pinned.json was recorded (scripts/record_ops_pinned.py; the
cases are tests/ops_pinned_cases.py).  A refusal whose text was changed on
purpose carries the earlier one as "old_message"."""
import json
import os

import pytest

import ops_pinned_cases as cases
from conftest import GOLDEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OPS = ("cell_forward", "cell_backward", "hconv_step", "seq_forward", "seq_forward_x", "bwd_step",
       "weight_grad", "weight_grad_planes", "lstm_weight_grads", "bias_grad", "bias_act", "mse_loss",
       "flstm_step")


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "ops_pinned.json")) as f:
        return json.load(f)


def test_refusals(dev, recorded):
    now, want = cases.refused(dev), recorded["refusals"]
    assert sorted(now) == sorted(want)
    for op in OPS:
        assert any(k.startswith(op + "/") for k in want), op
    assert {k: v["type"] for k, v in now.items()} == {k: v["type"] for k, v in want.items()}
    wrong = {k: (v["message"], want[k]["message"]) for k, v in now.items()
             if v["message"] != want[k]["message"]}
    assert wrong == {}


def test_abi_refusals_that_need_a_plan(dev, recorded):
    now, want = cases.abi_refused(dev), recorded["abi_refusals"]
    assert sorted(now) == sorted(want)
    assert {k: v["status"] for k, v in now.items()} == {k: v["status"] for k, v in want.items()}
    wrong = {k: (v["message"], want[k]["message"]) for k, v in now.items()
             if v["message"] != want[k]["message"]}
    assert wrong == {}


def test_recorded_bits(dev, recorded):
    now, want = cases.results(dev), recorded["results"]
    assert sorted(now) == sorted(want)
    for op in OPS:
        assert any(k.startswith(op + "_") for k in want), op
    wrong = {(k, o): (now[k][o], want[k][o]) for k in want for o in want[k] if now[k][o] != want[k][o]}
    assert wrong == {}
