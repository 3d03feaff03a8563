"""tests/dp_harness.py on the CPU: two gloo ranks carry arrays of every dtype
the data-parallel cases gather, the shards are dist.shard's, a rank that raises
fails the launch with its traceback and no hang, and only the known cases run."""
import numpy as np
import pytest

import dp_harness as DP
import dp_selfcheck_case as Case
import dp_selfcheck_raises_case as Raises

torch = pytest.importorskip("torch")


@pytest.mark.timeout(300)
def test_world2_gathers_every_ranks_arrays(tmp_path):
    d = DP.launch_world2("dp_selfcheck_case", tmp_path / "selfcheck.npz", 120)
    assert int(d["world"]) == 2
    for r in range(2):
        for k, mine in Case.arrays(r).items():
            assert d[k][r].dtype == mine.dtype and d[k][r].shape == mine.shape, (k, r)
            assert np.array_equal(d[k][r], mine), (k, r)
    assert d["shards"].tolist() == [[0, 2], [2, 5]]  # the last rank takes the remainder


@pytest.mark.timeout(300)
def test_a_failing_rank_fails_the_launch_with_its_traceback(tmp_path):
    with pytest.raises(AssertionError) as e:
        DP.launch_world2("dp_selfcheck_raises_case", tmp_path / "never.npz", 120)
    assert "Traceback" in str(e.value) and f"RuntimeError: {Raises.MESSAGE}" in str(e.value)
    assert not (tmp_path / "never.npz").exists()


def test_an_unknown_case_is_refused_before_anything_starts(tmp_path, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a child was started")
    monkeypatch.setattr(DP.subprocess, "run", no_launch)
    monkeypatch.setattr(DP.sys, "path", list(DP.sys.path))  # main() prepends to it
    with pytest.raises(ValueError, match="unknown data-parallel case 'dp_resgnn_wroker'"):
        DP.launch_world2("dp_resgnn_wroker", tmp_path / "x.npz", 120)
    with pytest.raises(ValueError, match="unknown data-parallel case"):
        DP.main("conftest", str(tmp_path / "x.npz"))
