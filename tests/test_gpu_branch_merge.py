"""The two seams of the closeness / period / trend networks on the GPU
(cnn_graph_amd/csrc/branch_merge.hip): cg_branch_merge_forward / _backward and
cg_concat_drop_forward / _backward.

Bars.  Everything elementwise is BITWISE against the composition it replaces,
computed by torch / ops.dropout on the device: the merge chain
((y0*w0) + y1*w1) + ..., dy_b = dout * w_b, the concat of the dropped branches and
the split of the gradient through the masks.  dw_b, a sum over the batch in an
order of its own, is within 1e-6 (max |a - ref| / max |ref|) of the float64 sum,
and two calls agree bitwise.  The backward cases draw dout and y positive: at
M F = 1 the tensor is ONE sum, and a relative bar on a sum of signed terms
measures how far the data happens to cancel, not the kernel (any fp32 order
misses 1e-6 there).  Same-sign terms leave the summation error alone: at most
(ceil(N / 8) + 7) roundings of eps / 2 = 6e-8 each, 8e-7 at N = 50, a few 1e-8
typically."""
import ctypes
import itertools
import zlib

import numpy as np
import pytest

from oracle import cheb_oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
# the backward's batch lanes per workgroup (BM_LANES of branch_merge.hip): batch lane r
# sums n = r, r + 8, ...; N = 1 and 3 leave lanes idle, 8 fills them once, 9 and 50 cross
BATCH_LANES = 8
MS = [1, 15, 17, 129, 200]
NS = [1, 3, 50]
FS = [1, 2, 3, 8]
BS = [1, 2, 3, 4]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def _gen(dev, *key):
    g = torch.Generator(device=dev)
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _merge_inputs(dev, B, N, M, F, positive=False):
    """positive: y and dout in [0.5, 1.5) (the dw sums then do not cancel); w stays signed."""
    g = _gen(dev, B, N, M, F)
    draw = (lambda s: torch.rand(s, device=dev, generator=g) + 0.5) if positive else \
        (lambda s: torch.randn(s, device=dev, generator=g))
    ys = [draw((N, M, F)) for _ in range(B)]
    ws = [torch.randn((M, F), device=dev, generator=g) for _ in range(B)]
    dout = draw((N, M, F))
    return ys, ws, dout


def _chain(ys, ws):
    acc = ys[0] * ws[0]
    for y, w in zip(ys[1:], ws[1:]):
        acc = acc + y * w
    return acc


def _offset_view(t):
    """The same values in a view that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ===== the merge, forward ============================================================
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_merge_forward_bitwise(dev, M, N):
    from cnn_graph_amd import ops
    widths = set()
    for B, F in itertools.product(BS, FS):
        ys, ws, _ = _merge_inputs(dev, B, N, M, F)
        out = ops.branch_merge_forward(ys, ws)
        assert torch.equal(out, _chain(ys, ws)), (B, N, M, F)
        widths.add((M * F) % 4 == 0)
    torch.cuda.synchronize()
    assert widths == ({True} if M % 4 == 0 else {True, False})  # both access widths ran


def test_merge_forward_scalar_path_on_an_offset_view(dev):
    """M F = 136 is a multiple of four, but one y_b starts 4 bytes past a 16-byte
    boundary: the call must take the scalar kernels (a dwordx4 load there is
    misaligned) and give the same bits."""
    from cnn_graph_amd import ops
    ys, ws, dout = _merge_inputs(dev, 3, 3, 17, 8)
    ref = _chain(ys, ws)
    ys[1] = _offset_view(ys[1])
    assert torch.equal(ops.branch_merge_forward(ys, ws), ref)
    ws[2] = _offset_view(ws[2])
    assert torch.equal(ops.branch_merge_forward(ys, ws), ref)
    dys, dws = ops.branch_merge_backward(dout, ys, ws)
    dys0, dws0 = ops.branch_merge_backward(dout, [y.clone() for y in ys], [w.clone() for w in ws])
    assert all(torch.equal(a, b) for a, b in zip(dys + dws, dys0 + dws0))
    torch.cuda.synchronize()


# ===== the merge, backward ===========================================================
@pytest.mark.parametrize("N", [1, 3, BATCH_LANES, BATCH_LANES + 1, 50])
@pytest.mark.parametrize("M", MS)
def test_merge_backward(dev, M, N):
    from cnn_graph_amd import ops
    for B, F in itertools.product(BS, FS):
        ys, ws, dout = _merge_inputs(dev, B, N, M, F, positive=True)
        dys, dws = ops.branch_merge_backward(dout, ys, ws)
        dys2, dws2 = ops.branch_merge_backward(dout, ys, ws)
        for b in range(B):
            tag = (B, N, M, F, b)
            assert torch.equal(dys[b], dout * ws[b]), tag
            ref = (dout.double() * ys[b].double()).sum(0).cpu().numpy()
            err = O.normwise_err(dws[b].cpu().numpy(), ref)
            assert err <= 1e-6, (tag, err)
            assert torch.equal(dws[b], dws2[b]) and torch.equal(dys[b], dys2[b]), tag
        # accumulate_dw adds the very sum into what is there
        base = [torch.randn_like(w) for w in ws]
        acc = [t.clone() for t in base]
        ops.branch_merge_backward(dout, ys, ws, out_dw=acc, accumulate_dw=True)
        assert all(torch.equal(a, t + d) for a, t, d in zip(acc, base, dws)), (B, N, M, F)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,F", [(17, 3), (17, 8)], ids=["scalar", "dwordx4"])
def test_merge_backward_null_entries_touch_nothing(dev, M, F):
    """dy_1 and dw_0, dw_2 are NULL.  The outputs that are asked for sit in one
    sentinel-filled arena with guard bands between them: the bands stay
    sentinels, the outputs are those of the full call."""
    from cnn_graph_amd import _lib, ops
    B, N = 3, 9
    ys, ws, dout = _merge_inputs(dev, B, N, M, F)
    full_dy, full_dw = ops.branch_merge_backward(dout, ys, ws)
    n, mf, guard = N * M * F, M * F, 64
    sentinel = -12345.5
    arena = torch.full((2 * n + mf + 4 * guard,), sentinel, device=dev)
    at = lambda off, cnt: arena[off:off + cnt]  # noqa: E731
    dy0, dy2, dw1 = at(guard, n), at(2 * guard + n, n), at(3 * guard + 2 * n, mf)
    if F == 8:  # the dwordx4 case really is one: every pointer of the call is aligned
        assert all(t.data_ptr() % 16 == 0 for t in (dy0, dy2, dw1))
    ptrs = lambda ts: (ctypes.c_void_p * B)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    _lib.call("cg_branch_merge_backward", B, N, M, F, dout.data_ptr(), ptrs(ys), ptrs(ws),
              ptrs([dy0, None, dy2]), ptrs([None, dw1, None]), 0,
              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(dy0.view(N, M, F), full_dy[0]) and torch.equal(dy2.view(N, M, F), full_dy[2])
    assert torch.equal(dw1.view(M, F), full_dw[1])
    mask = torch.ones_like(arena, dtype=torch.bool)
    for t in (dy0, dy2, dw1):
        o = (t.data_ptr() - arena.data_ptr()) // 4
        mask[o:o + t.numel()] = False
    assert int(mask.sum()) == 4 * guard and bool((arena[mask] == sentinel).all())
    # the per-branch flags of the op: skipped entries come back as None
    dys, dws = ops.branch_merge_backward(dout, ys, ws, need_dy=[False, True, False],
                                         need_dw=[True, False, False])
    assert dys[0] is None and dys[2] is None and dws[1] is None and dws[2] is None
    assert torch.equal(dys[1], full_dy[1]) and torch.equal(dws[0], full_dw[0])


def test_branch_merge_autograd(dev):
    from cnn_graph_amd import ops
    ys, ws, dout = _merge_inputs(dev, 3, 5, 40, 2)
    ys = [y.requires_grad_(True) for y in ys]
    ws = [w.requires_grad_(b != 1) for b, w in enumerate(ws)]  # w_1 frozen: its dw is skipped
    out = ops.branch_merge(ys, ws)
    assert torch.equal(out, _chain(ys, ws))
    out.backward(dout)
    dys, dws = ops.branch_merge_backward(dout, [y.detach() for y in ys], [w.detach() for w in ws])
    assert all(torch.equal(y.grad, d) for y, d in zip(ys, dys))
    assert torch.equal(ws[0].grad, dws[0]) and ws[1].grad is None and torch.equal(ws[2].grad, dws[2])
    with pytest.raises(ValueError):
        ops.branch_merge(ys, ws[:2])
    with pytest.raises(ValueError):
        ops.branch_merge_forward([y.detach() for y in ys] * 2, [w.detach() for w in ws] * 2)  # B = 6


# ===== concat-drop =====================================================================
def _dropout_backward(dy, keep, seed):
    from cnn_graph_amd import _lib
    if keep >= 1.0:
        return dy
    dx = torch.empty_like(dy)
    _lib.call("cg_dropout_backward", dy.data_ptr(), dy.numel(), float(keep), int(seed), dx.data_ptr(),
              torch.cuda.current_stream(dy.device).cuda_stream)
    return dx


H_SETS = [(8, 12, 32), (1, 3, 2), (4,), (8, 8), (4, 4, 4, 4), (5, 32)]


@pytest.mark.parametrize("keep", [0.8, 0.5, 1.0])
@pytest.mark.parametrize("N,M", [(1, 1), (3, 17), (2, 129), (50, 200)])
def test_concat_drop_bitwise(dev, N, M, keep):
    from cnn_graph_amd import ops
    for Hs in H_SETS:
        g = _gen(dev, N, M, Hs)
        hs = [torch.randn((N, M, H), device=dev, generator=g) for H in Hs]
        for h in hs:
            h[h == 0] = 1.0
        # every branch the slice at a non-zero element offset of its own larger stream
        bases = [0xC0FFEE1234567 + 977 * b for b in range(len(Hs))]
        offs = [(b + 1) * 5 * N * M * H for b, H in enumerate(Hs)]
        seeds = [(s + ops.DROP_WEYL * o) & M64 for s, o in zip(bases, offs)]
        ref = torch.cat([ops.dropout(h, keep, s, offset=o) for h, s, o in zip(hs, bases, offs)], dim=2)
        out = ops.concat_drop_forward(hs, keep, seeds)
        assert torch.equal(out, ref), (N, M, Hs, keep)
        if keep < 1.0 and N * M * sum(Hs) >= 64:
            assert bool(((out == 0) & (torch.cat(hs, dim=2) != 0)).any()), "the masks drop nothing"
        dx = torch.randn((N, M, sum(Hs)), device=dev, generator=g)
        dhs = ops.concat_drop_backward(dx, list(Hs), keep, seeds)
        edges = np.cumsum((0,) + Hs)
        for b, dh in enumerate(dhs):
            sl = dx[:, :, edges[b]:edges[b + 1]].contiguous()
            assert torch.equal(dh, _dropout_backward(sl, keep, seeds[b])), (N, M, Hs, keep, b)
    torch.cuda.synchronize()


def test_concat_drop_offset_view_and_autograd(dev):
    from cnn_graph_amd import ops
    N, M, Hs, keep = 3, 17, (8, 12, 32), 0.8
    g = _gen(dev, "cd")
    hs = [torch.randn((N, M, H), device=dev, generator=g) for H in Hs]
    seeds = [11, 22, 33]
    ref = ops.concat_drop_forward(hs, keep, seeds)
    moved = [hs[0], _offset_view(hs[1]), hs[2]]  # every H_b % 4 == 0, one pointer is not aligned
    assert torch.equal(ops.concat_drop_forward(moved, keep, seeds), ref)
    leaves = [h.clone().requires_grad_(True) for h in hs]
    out = ops.concat_drop(leaves, keep, seeds)
    assert torch.equal(out, ref)
    dx = torch.randn_like(out)
    out.backward(dx)
    for leaf, dh in zip(leaves, ops.concat_drop_backward(dx, list(Hs), keep, seeds)):
        assert torch.equal(leaf.grad, dh)
    # keep == 1 is the plain concat, seeds or none
    assert torch.equal(ops.concat_drop(hs), torch.cat(hs, dim=2))
    assert torch.equal(ops.concat_drop(hs, 1.0, seeds), torch.cat(hs, dim=2))
    with pytest.raises(ValueError):
        ops.concat_drop_forward(hs, 0.0, seeds)
    torch.cuda.synchronize()
