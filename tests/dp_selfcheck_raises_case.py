"""Case of tests/test_dp_harness_cpu.py (not a test module): rank 1 fails before
the first exchange, while rank 0 waits in it.  Run through tests/dp_harness.py
(case ``dp_selfcheck_raises_case``)."""
import numpy as np

import dp_harness as DP

DEVICE = "cpu"
MESSAGE = "rank 1 gives up on purpose"


def rank_result(rank, world, dev, comm):
    if rank == 1:
        raise RuntimeError(MESSAGE)
    return dict(never=DP.gather_ranks(np.zeros(2))[0])
