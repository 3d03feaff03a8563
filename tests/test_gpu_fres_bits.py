"""The residual Fourier filter and its dropout seam give the recorded bits:
tests/golden/fres_bits.json holds SHA-256 digests of xhat, y, dx, dW, dz of the
cases in tests/fres_bits_cases.py (scripts/record_fres_bits.py records them;
no atomics in these kernels, so equality is the bar)."""
import ctypes
import json
import os

import pytest

import fres_bits_cases
from conftest import GOLDEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def test_recorded_bits(dev):
    with open(os.path.join(GOLDEN, "fres_bits.json")) as f:
        want = json.load(f)
    got = fres_bits_cases.run(dev)
    assert sorted(got) == sorted(want)
    differ = {k: [o for o in fres_bits_cases.OUTPUTS if got[k][o] != want[k][o]] for k in want if got[k] != want[k]}
    assert not differ, differ


def test_keywords_and_wrappers_agree(dev):
    """keep_prob / seed on fres_forward / fres_backward are the _drop wrappers."""
    from cnn_graph_amd import ops
    M, N, Fin, Fout = 17, 3, 8, 4
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    r = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
    B = ops.gft_prepare(r(M, M) / M ** 0.5)
    W, x, res, dy = r(M, Fout, Fin), r(N, M, Fin), r(N, M, Fout), r(N, M, Fout)
    seed = fres_bits_cases.SEED
    a = ops.fres_forward_drop(B, W, x, 0.8, seed, res, "relu")
    b = ops.fres_forward(B, W, x, res, "relu", keep_prob=0.8, seed=seed)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    c = ops.fres_backward_drop(B, W, a[0], dy, 0.8, seed, a[1], "relu")
    d = ops.fres_backward(B, W, a[0], dy, a[1], "relu", keep_prob=0.8, seed=seed)
    assert all(torch.equal(p, q) for p, q in zip(c, d))
    assert bool((c[0] == 0).any()) and int(torch.count_nonzero(c[0])) > 0  # a mask, not a constant


def test_drop_has_no_accumulate_and_no_skipped_dx():
    """keep_prob < 1 with dx_accumulate or need_dx=False has no C entry: a
    ValueError before any device work (the tensors are not even looked at)."""
    from cnn_graph_amd import ops
    for kw in (dict(dx_accumulate=True, dx=object()), dict(need_dx=False)):
        with pytest.raises(ValueError, match="keep_prob < 1"):
            ops.fres_backward(None, None, None, None, keep_prob=0.8, seed=1, **kw)


def test_reported_workspace_is_enough(dev):
    """Each of the four entries runs in exactly cg_fres_workspace_bytes and
    refuses one byte less (dx given)."""
    from cnn_graph_amd import _lib, ops
    h = _lib.lib()
    N, M, Fin, Fout = 2, 17, 8, 4
    B = ops.gft_prepare(torch.eye(M, device=dev))
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    W, x, xhat, y, dy, dz, dx, dW = (z(M, Fout, Fin), z(N, M, Fin), z(N, M, Fin), z(N, M, Fout),
                                     z(N, M, Fout), z(N, M, Fout), z(N, M, Fin), z(M, Fout, Fin))
    fb, bb = ops.fres_workspace_bytes(N, M, Fin, Fout)
    ws = torch.empty(max(fb, bb), device=dev, dtype=torch.uint8)
    p = lambda a: a.data_ptr()  # noqa: E731
    head = (N, M, Fin, Fout, p(B), B.numel(), p(W))
    for keep in (None, 0.8, 1.0):
        drop = () if keep is None else (ctypes.c_float(keep), 5)
        fwd = h.cg_fres_forward if keep is None else h.cg_fres_forward_drop
        bwd = h.cg_fres_backward if keep is None else h.cg_fres_backward_drop
        acc = (0,) if keep is None else ()
        for n, want in ((fb - 1, _lib.CG_ERR_ARG), (fb, _lib.CG_OK)):
            assert fwd(*head, p(x), *drop, None, 0, p(xhat), p(y), p(ws), n, None) == want, (keep, n)
        for n, want in ((bb - 1, _lib.CG_ERR_ARG), (bb, _lib.CG_OK)):
            assert bwd(*head, p(xhat), p(dy), None, 0, *drop, p(dz), p(dx), *acc, p(dW), p(ws), n,
                       None) == want, (keep, n)
    torch.cuda.synchronize()
