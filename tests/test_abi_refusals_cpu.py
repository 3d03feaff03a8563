"""The C entries refuse the calls of tests/abi_refusal_cases.py with the status
and the text recorded in tests/golden/abi_refusals.json
(scripts/record_abi_refusals.py).  No GPU: every call fails an argument check
before any HIP call, and the pointers are never memory.  A case whose text was
changed on purpose carries the earlier one as "old_message"."""
import json
import os

import pytest

import abi_refusal_cases
from cnn_graph_amd import _lib
from conftest import GOLDEN


@pytest.fixture(scope="module")
def now(built_lib):
    return abi_refusal_cases.run()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "abi_refusals.json")) as f:
        return json.load(f)


def test_table_and_recording_cover_the_same_cases(now, recorded):
    assert sorted(now) == sorted(recorded)
    assert len(now) >= 130


def test_statuses(now, recorded):
    wrong = {k: (v["status"], recorded[k]["status"]) for k, v in now.items()
             if v["status"] != recorded[k]["status"]}
    assert wrong == {}
    assert {v["status"] for v in now.values()} == {_lib.CG_ERR_ARG, _lib.CG_ERR_UNSUPPORTED}


def test_messages(now, recorded):
    wrong = {k: (v["message"], recorded[k]["message"]) for k, v in now.items()
             if v["message"] != recorded[k]["message"]}
    assert wrong == {}


def test_every_kind_of_refusal_is_in_the_table(recorded):
    for kind in ("null", "workspace_small", "misaligned", "alias", "_is_", "H_300", "_0"):
        assert any(kind in k for k in recorded), kind
