"""The cases behind tests/golden/fres_bits.json: SHA-256 digests of the raw
bytes of xhat, y, dx, dW, dz from ops.fres_forward[_drop] / ops.fres_backward[_drop].

scripts/record_fres_bits.py records them, tests/test_gpu_fres_bits.py replays
them.  The kernels have no atomics, so the bits are a function of the inputs
(numpy.random.default_rng on the host), the shape and the gemm_x3 option.

Shapes (M, N, Fin, Fout): (17, 3, 8, 1) is one ragged row tile with Fout 1;
(129, 2, 33, 32) crosses the 128-row tile and leaves a ragged column tile."""
import hashlib
import itertools

import numpy as np

SHAPES = [(17, 3, 8, 1), (129, 2, 33, 32)]
# the seed as the seam passes it: a base with a slice offset folded in
SEED = (0xC0FFEE1234567 + 0x9E3779B97F4A7C15 * 4242) & ((1 << 64) - 1)
# (api, keep): the plain entries, and the seam entries at the identity and below it
APIS = [("plain", 1.0), ("drop", 1.0), ("drop", 0.8)]
ACTS = [("relu", True), ("none", False)]  # (act, with a residual)
OUTPUTS = ("xhat", "y", "dx", "dW", "dz")


def digest(t):
    if t is None:
        return None
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def run(dev):
    """{case id: {output: digest}} of every case, on device ``dev``."""
    import torch

    from cnn_graph_amd import _lib, ops

    out = {}
    for (M, N, Fin, Fout), x3 in itertools.product(SHAPES, (1, 0)):
        shape = f"M{M}_N{N}_Fin{Fin}_Fout{Fout}_x3{x3}"
        rng = np.random.default_rng(1000 * M + 10 * N + Fin)

        def draw(*s):
            return torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(dev)

        U = draw(M, M) / M ** 0.5
        W, x, res, dy, dx_in = draw(M, Fout, Fin), draw(N, M, Fin), draw(N, M, Fout), draw(N, M, Fout), draw(N, M, Fin)
        prev = _lib.set_option("gemm_x3", x3)
        try:
            B = ops.gft_prepare(U)
            for (api, keep), (act, with_res) in itertools.product(APIS, ACTS):
                r = res if with_res else None
                if api == "plain":
                    xhat, y = ops.fres_forward(B, W, x, r, act)
                    dx, dW, dz = ops.fres_backward(B, W, xhat, dy, y, act)
                else:
                    xhat, y = ops.fres_forward_drop(B, W, x, keep, SEED, r, act)
                    dx, dW, dz = ops.fres_backward_drop(B, W, xhat, dy, keep, SEED, y, act)
                out[f"{shape}_{api}_keep{keep}_{act}"] = dict(zip(OUTPUTS, map(digest, (xhat, y, dx, dW, dz))))
            # the plain backward only: dx += into a given tensor, and no dx at all
            xhat, y = ops.fres_forward(B, W, x, res, "relu")
            dx, dW, dz = ops.fres_backward(B, W, xhat, dy, y, "relu", dx=dx_in.clone(), dx_accumulate=True)
            out[f"{shape}_plain_dx_accumulate"] = dict(zip(OUTPUTS, map(digest, (xhat, y, dx, dW, dz))))
            dx, dW, dz = ops.fres_backward(B, W, xhat, dy, y, "relu", need_dx=False)
            out[f"{shape}_plain_no_dx"] = dict(zip(OUTPUTS, map(digest, (xhat, y, dx, dW, dz))))
        finally:
            _lib.set_option("gemm_x3", prev)
    torch.cuda.synchronize()
    return out
