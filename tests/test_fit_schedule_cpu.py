"""trainer.fit_schedule against the loop it restates (lib/graph_model.py:139-147):
a deque refilled with a permutation whenever fewer than a batch of indices are
left, a batch being its first entries.  No GPU, no library."""
import collections

import numpy as np
import pytest

from cnn_graph_amd.trainer import fit_schedule

CASES = [(10, 4, 3), (8, 4, 2), (5, 5, 2), (7, 3, 5)]  # (S, batch, epochs)


def deque_loop(S, batch, num_steps, rs):
    """The reference's loop, literally; also returns the draw number at which each refill happened."""
    indices, out, refills = collections.deque(), [], []
    for step in range(num_steps):
        if len(indices) < batch:
            refills.append(step * batch + len(indices))
            indices.extend(rs.permutation(S))
        out.append([indices.popleft() for i in range(batch)])
    return np.array(out, np.int32).reshape(num_steps, batch), refills


@pytest.mark.parametrize("S,batch,epochs", CASES)
def test_equals_the_deque_loop(S, batch, epochs):
    num_steps = int(epochs * S / batch)
    want, _ = deque_loop(S, batch, num_steps, np.random.RandomState(11))
    got = fit_schedule(S, batch, num_steps, np.random.RandomState(11))
    assert got.dtype == np.int32 and got.shape == (num_steps, batch)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("S,batch,epochs", CASES)
def test_every_refill_starts_a_permutation(S, batch, epochs):
    num_steps = int(epochs * S / batch)
    _, refills = deque_loop(S, batch, num_steps, np.random.RandomState(11))
    flat = fit_schedule(S, batch, num_steps, np.random.RandomState(11)).reshape(-1)
    assert refills[0] == 0
    whole = [r for r in refills if r + S <= flat.size]
    assert whole, "no whole epoch in the schedule"
    for r in whole:
        assert sorted(flat[r:r + S]) == list(range(S)), r
    # leftovers carry over: where S is no multiple of the batch, some refill is not at a batch start
    if S % batch:
        assert any(r % batch for r in refills)


def test_short_dataset_is_refused():
    with pytest.raises(ValueError, match="IndexError"):
        fit_schedule(3, 4, 2, 0)


def test_seed_forms_agree():
    a = fit_schedule(9, 4, 6, 5)
    assert np.array_equal(a, fit_schedule(9, 4, 6, np.random.RandomState(5)))
    # None: the global numpy state, the reference's source
    saved = np.random.get_state()
    try:
        np.random.seed(5)
        assert np.array_equal(a, fit_schedule(9, 4, 6, None))
    finally:
        np.random.set_state(saved)
    assert not np.array_equal(a, fit_schedule(9, 4, 6, 6))
