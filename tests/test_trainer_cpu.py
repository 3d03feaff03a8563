"""trainer.FlatTrainer without a GPU: cg_mse_loss_workspace_bytes is host
arithmetic, so the trainer's buffers, its carving, the learning-rate staircase
and the bucket check can be built and exercised on device="cpu".  Nothing here
launches a kernel."""
import pytest

torch = pytest.importorskip("torch")


def make(built_lib, total=20, optimizer="adam", lr=0.5, decay_rate=0.5, decay_steps=4):
    from cnn_graph_amd.trainer import FlatTrainer
    return FlatTrainer(total, (2, 3, 2), optimizer, lr, decay_rate, decay_steps, "cpu", None)


def span(t):
    return t.data_ptr(), t.data_ptr() + 4 * t.numel()


def test_carved_views_tile_the_flat_buffers_in_order(built_lib):
    m = make(built_lib)
    init = torch.arange(6, dtype=torch.float32).view(2, 3)
    p, pg = m.carve((2, 3), "a/Wx", init=init)
    w, wg = m.carve((4, 2), "b/weights")
    v, vg = m.carve((6,), "c/weights")
    m._carved()
    assert m.names == ["a/Wx", "b/weights", "c/weights"]
    assert list(m.parameters()) == m.names and list(m.gradients()) == m.names
    for buf, views in ((m.flat, (p, w, v)), (m.grad, (pg, wg, vg))):
        at = buf.data_ptr()
        for t, shape in zip(views, ((2, 3), (4, 2), (6,))):
            assert tuple(t.shape) == shape and t.is_contiguous() and t.data_ptr() == at
            at += 4 * t.numel()
        assert at == span(buf)[1]
    # the Parameter form aliases flat, its .grad aliases grad; the plain form is a plain view
    assert isinstance(p, torch.nn.Parameter) and m.params == [p]
    assert not isinstance(w, torch.nn.Parameter)
    assert torch.equal(m.flat[:6], init.reshape(-1))
    with torch.no_grad():
        p[1, 2] = 7.0
        w[0, 1] = 9.0
    assert float(m.flat[5]) == 7.0 and float(m.flat[7]) == 9.0
    assert p.grad.data_ptr() == pg.data_ptr() == m.grad.data_ptr()
    p.grad[0, 1] = 3.0
    wg[3, 1] = 4.0
    assert float(m.grad[1]) == 3.0 and float(m.grad[13]) == 4.0
    g = m.gradients()
    assert g["a/Wx"].data_ptr() == pg.data_ptr() and g["b/weights"].data_ptr() == wg.data_ptr()
    assert m.parameters()["a/Wx"] is p


def test_carving_must_end_at_the_total(built_lib):
    m = make(built_lib)
    m.carve((4, 4), "w")
    with pytest.raises(AssertionError):
        m._carved()


def test_staircase_learning_rate(built_lib):
    m = make(built_lib, lr=0.5, decay_rate=0.5, decay_steps=4)
    assert m.learning_rate(0) == 0.5 and m.learning_rate(3) == 0.5
    assert m.learning_rate(4) == 0.25 and m.learning_rate(8) == 0.125
    for steps in (None, 0):
        m = make(built_lib, lr=0.5, decay_rate=0.5, decay_steps=steps)
        assert m.learning_rate(0) == m.learning_rate(1000) == 0.5
    m = make(built_lib, lr=0.5, decay_rate=1, decay_steps=4)
    assert m.learning_rate(4) == 0.5


def test_slots_and_buffers(built_lib):
    for opt in ("adam", "sgd"):
        m = make(built_lib, optimizer=opt)
        assert not m.s1.any() and not m.s2.any()
    m = make(built_lib, optimizer="rmsprop")
    assert bool((m.s1 == 1).all()) and not m.s2.any()  # TF's RMSProp: ms ones, mom zeros
    assert m.s1.numel() == m.s2.numel() == m.flat.numel() == m.grad.numel() == 20
    assert not m.grad.any() and not m.ema.any() and tuple(m.ema.shape) == (3,)
    assert tuple(m.dout.shape) == (2, 3, 2) and tuple(m.loss.shape) == (1,)
    assert m.step_count == 0 and m.world == 1 and m.mws.numel() >= max(m.mws_n, 1)
    assert m.loss_average.data_ptr() == m.ema[1:2].data_ptr()
    with pytest.raises(ValueError):
        make(built_lib, optimizer="adagrad")


def test_a_grad_outside_the_bucket_raises_before_any_launch(built_lib):
    class Comm:
        world, calls = 2, 0

        def allreduce_sum_(self, tensor, stream):
            self.calls += 1

    m = make(built_lib)
    m.comm = Comm()
    p, _ = m.carve((4, 5), "w", init=torch.zeros(4, 5))
    m._carved()
    launched = []
    m._update = lambda *a: launched.append(a) or 0
    flat0 = m.flat.clone()
    for bad in (torch.zeros(4, 5), None):
        p.grad = bad
        with pytest.raises(RuntimeError, match="left the flat gradient bucket"):
            m._exchange_and_update(None)
    assert m.comm.calls == 0 and not launched and m.step_count == 0
    assert torch.equal(m.flat, flat0)
