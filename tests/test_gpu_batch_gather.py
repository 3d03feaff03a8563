"""cg_batch_gather / ops.batch_gather on the GPU: a batch of a device-resident
dataset in one launch, EXACT (np.array_equal) against numpy fancy indexing with
a zero row wherever the index is outside [0, S).  The index vector of every
small case holds a duplicate, a negative index and an index equal to S, and the
outputs sit between canaries that must stay untouched."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

S, N = 7, 5
IDX = [3, -1, 3, 7, 0]
CANARY = -12345.0
PAD = 8  # floats either side of an output: 32 bytes, so the output keeps its alignment


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_graph_amd import _lib
    _lib.lib()
    return torch.device("cuda", 0)


def expected(a, idx):
    """a[idx] with zero rows for indices outside [0, len(a))."""
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < a.shape[0])
    out = np.zeros((len(idx),) + a.shape[1:], a.dtype)
    out[ok] = a[idx[ok]]
    return out


def guarded(n, shape, dev):
    """(buffer, view of ``shape`` inside it) with PAD canary floats on both sides."""
    buf = torch.full((n + 2 * PAD,), CANARY, device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def run(dev, row_shape, lrow_shape, idx, n, s=S, misalign=False, seed=0):
    """Gather through ops.batch_gather into guarded outputs; returns what a test compares."""
    from cnn_graph_amd import ops
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((s,) + row_shape).astype(np.float32)
    labels = None if lrow_shape is None else rng.standard_normal((s,) + lrow_shape).astype(np.float32)
    if misalign:  # a contiguous view one float into its buffer: 4-byte aligned only
        store = torch.empty(data.size + 1, device=dev)
        d = store[1:].view(data.shape)
        d.copy_(torch.from_numpy(data))
        assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    else:
        d = torch.from_numpy(data).to(dev)
        assert d.data_ptr() % 16 == 0
    l = None if labels is None else torch.from_numpy(labels).to(dev)
    it = torch.tensor(idx, dtype=torch.int32, device=dev)
    xbuf, x = guarded(n * int(np.prod(row_shape)), (n,) + row_shape, dev)
    ybuf, y = (None, None) if labels is None else guarded(n * int(np.prod(lrow_shape)), (n,) + lrow_shape, dev)
    gx, gy = ops.batch_gather(d, l, it, n, out_x=x, out_y=y)
    torch.cuda.synchronize()
    assert gx.data_ptr() == x.data_ptr() and (gy is None) == (labels is None)
    for name, buf in (("x", xbuf), ("y", ybuf)):
        if buf is not None:
            b = buf.cpu().numpy()
            assert (b[:PAD] == CANARY).all() and (b[-PAD:] == CANARY).all(), f"canary around {name}"
    assert np.array_equal(gx.cpu().numpy(), expected(data, idx[:n]))
    if labels is not None:
        assert np.array_equal(gy.cpu().numpy(), expected(labels, idx[:n]))


def test_scalar_body(dev):
    run(dev, (3, 2), (2,), IDX, N)  # row 6, lrow 2


def test_float4_body(dev):
    run(dev, (4, 2), (2, 2), IDX, N)  # row 8, lrow 4


def test_float4_row_with_a_scalar_label_row(dev):
    run(dev, (4, 2), (2,), IDX, N)  # row 8, lrow 2: lrow decides, the scalar body


def test_misaligned_data(dev):
    run(dev, (4, 2), (2, 2), IDX, N, misalign=True)  # row 8, data 4 bytes off 16


def test_without_labels(dev):
    run(dev, (4, 2), None, IDX, N)
    run(dev, (3, 2), None, IDX, N)


def test_one_long_row(dev):
    """row = 2052 = 4 * 513 with N = 1: the row is longer than one workgroup's
    pass of 256 lanes, and the last workgroup is a tail of one float4."""
    run(dev, (2052,), (4,), [3], 1)
    run(dev, (2052,), (4,), [-1], 1)  # the padded row of a ragged batch
    run(dev, (2053,), (4,), [6], 1)   # the same in the scalar body


def test_more_elements_than_one_grid_pass(dev):
    """More lanes than the largest grid has (256 CUs * 8 workgroups * 256 lanes =
    524 288): the grid-stride loop runs, in both bodies."""
    n, s = 130, 9
    idx = [(5 * k) % (s + 2) - 1 for k in range(n)]  # -1 .. s, every kind of index
    run(dev, (16400,), (36,), idx, n, s=s)       # float4: 130 * (4100 + 9) = 534 170 lanes
    run(dev, (16390,), (6,), idx[:40], 40, s=s)  # scalar: 40 * (16390 + 6) = 655 840 lanes


def test_idx_longer_than_n_reads_only_n(dev):
    run(dev, (4, 2), (2, 2), IDX + [0, 1, 2], N)


def test_source_offsets_past_2_31(dev):
    """S * row = 2050 * 2^20 floats is past 2^31 elements (8.6 GB): the source
    offset is 64-bit.  Only the rows that are read are written first."""
    from cnn_graph_amd import ops
    row, s = 1 << 20, 2050
    data = torch.empty((s, row), device=dev)
    labels = torch.empty((s, 4), device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    picks = [s - 1, 0, 2048]  # 2048 * 2^20 = 2^31 exactly
    for p in picks:
        data[p] = torch.randn(row, device=dev, generator=g)
        labels[p] = torch.randn(4, device=dev, generator=g)
    it = torch.tensor(picks, dtype=torch.int32, device=dev)
    x, y = ops.batch_gather(data, labels, it, 3)
    torch.cuda.synchronize()
    for n, p in enumerate(picks):
        assert torch.equal(x[n], data[p]) and torch.equal(y[n], labels[p]), p


def test_ops_checks(dev):
    from cnn_graph_amd import ops
    d = torch.zeros((S, 8), device=dev)
    l = torch.zeros((S, 4), device=dev)
    it = torch.tensor(IDX, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError):
        ops.batch_gather(d, l, it.long(), N)
    with pytest.raises(ValueError):
        ops.batch_gather(d, l, it.cpu(), N)
    with pytest.raises(ValueError):
        ops.batch_gather(d.cpu(), l, it, N)
    with pytest.raises(ValueError):
        ops.batch_gather(d, l, it, N + 1)  # idx shorter than N
    with pytest.raises(ValueError):
        ops.batch_gather(d, l[:-1], it, N)  # sample counts differ
    with pytest.raises(ValueError):
        ops.batch_gather(d.t(), None, it, N)  # not contiguous
    with pytest.raises(ValueError):
        ops.batch_gather(d, l, it, N, out_x=torch.zeros((N, 7), device=dev))
    with pytest.raises(ValueError):
        ops.batch_gather(d, None, it, N, out_y=torch.zeros((N, 4), device=dev))
