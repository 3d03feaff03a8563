"""cg_momentum_update on the GPU against float64: three steps of TF 1.x Momentum
(and of gradient descent, momentum == 0) with the L2 term on a range of the flat
buffer.  Bar: 1e-5 normwise."""
import numpy as np
import pytest

from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def _ranges(n):
    """(reg_begin, reg_n): empty, starting and ending off a 16-byte boundary, the whole buffer."""
    out = [(0, 0), (0, n)]
    if n >= 5:
        out.append((1, n - 3))
    return out


@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_three_steps_vs_float64(dev, n, momentum):
    from cnn_graph_amd import ops
    lr, scale, reg = 0.1, 0.5, 5e-2
    for rb, rn in _ranges(n):
        rng = np.random.default_rng(n * 10 + rb)
        p0 = rng.standard_normal(n).astype(np.float32)
        p = torch.from_numpy(p0.copy()).to(dev)
        acc = torch.zeros(n, device=dev) if momentum else None
        rp, ra = p0.astype(np.float64), np.zeros(n)
        in_range = (np.arange(n) >= rb) & (np.arange(n) < rb + rn)
        for step in range(3):
            g0 = rng.standard_normal(n).astype(np.float32)
            ops.momentum_update(p, torch.from_numpy(g0).to(dev), acc, lr=lr, momentum=momentum,
                                grad_scale=scale, reg=reg, reg_begin=rb, reg_n=rn)
            g = g0.astype(np.float64) * scale + np.where(in_range, reg * rp, 0.0)
            ra = momentum * ra + g
            rp = rp - lr * ra
            torch.cuda.synchronize()
            assert O.normwise_err(p.cpu().numpy(), rp) < TOL, (rb, rn, step)
            if momentum:
                assert O.normwise_err(acc.cpu().numpy(), ra) < TOL, (rb, rn, step)
        if rn and n > 1:  # the term is visible at the bar, and only inside the range
            q = torch.from_numpy(p0.copy()).to(dev)
            a2 = torch.zeros(n, device=dev) if momentum else None
            g1 = torch.zeros(n, device=dev)
            ops.momentum_update(q, g1, a2, lr=lr, momentum=momentum, reg=reg, reg_begin=rb, reg_n=rn)
            torch.cuda.synchronize()
            moved = q.cpu().numpy() != p0
            assert np.array_equal(moved, in_range & (p0 != 0))


def test_scalar_lanes_for_an_unaligned_buffer(dev):
    """Views 4 bytes into their storage: the scalar kernel, the same numbers."""
    from cnn_graph_amd import ops
    n = 1027
    rng = np.random.default_rng(7)
    p0, g0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    outs = []
    for off in (0, 1):
        bufs = [torch.zeros(n + 4, device=dev) for _ in range(3)]
        p, g, a = (b[off:off + n] for b in bufs)
        p.copy_(torch.from_numpy(p0))
        g.copy_(torch.from_numpy(g0))
        for _ in range(2):
            ops.momentum_update(p, g, a, lr=0.05, momentum=0.9, reg=1e-2, reg_begin=5, reg_n=1000)
        torch.cuda.synchronize()
        assert all(float(b[off + n:].abs().max()) == 0.0 for b in bufs)  # nothing past the end
        outs.append((p.cpu().numpy(), a.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_momentum_zero_without_range_is_sgd_update(dev):
    from cnn_graph_amd import ops
    rng = np.random.default_rng(9)
    p0, g0 = rng.standard_normal(1027).astype(np.float32), rng.standard_normal(1027).astype(np.float32)
    a, b = torch.from_numpy(p0.copy()).to(dev), torch.from_numpy(p0.copy()).to(dev)
    g = torch.from_numpy(g0).to(dev)
    ops.momentum_update(a, g, None, lr=0.1, momentum=0.0, grad_scale=0.5)
    ops.sgd_update(b, g, lr=0.1, grad_scale=0.5)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
