"""Case of tests/test_dp_harness_cpu.py (not a test module): what the harness
itself carries between ranks, on the CPU.  Run through tests/dp_harness.py (case
``dp_selfcheck_case``)."""
import numpy as np

import dp_harness as DP

DEVICE = "cpu"


def arrays(rank):
    """What rank ``rank`` contributes: one array per dtype the cases gather."""
    return dict(f32=np.full((3, 5), rank + 0.5, np.float32), f64=np.arange(4, dtype=np.float64) - rank,
                i64=np.array([rank, -1 - rank, (1 << 62) + rank], dtype=np.int64))


def rank_result(rank, world, dev, comm):
    assert dev is None and (comm.rank, comm.world) == (rank, world)
    res = {k: np.stack(DP.gather_ranks(v)) for k, v in arrays(rank).items()}
    res["shards"] = np.stack(DP.gather_ranks(np.array(DP.shard_of(5, rank, world))))
    return res
