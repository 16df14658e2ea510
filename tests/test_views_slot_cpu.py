"""What the multi-view frame pipeline refuses and how its frames are grouped, without a GPU: pipeline.ViewsSlot's
construction checks (they come before any device allocation), ViewsBinding.batch_key and ops.max_view_frames."""
import pytest

torch = pytest.importorskip("torch")


def _net(kind, v_n):
    from monoport_amd.modeling import PIFuNetC, PIFuNetG, heads
    net = PIFuNetG() if kind == "G" else PIFuNetC()
    ch = [257, 1024, 512, 256, 128, 1] if kind == "G" else [513, 1024, 512, 256, 128, 3]
    net.surface_classifier = heads.SurfaceClassifier(ch, v_n, False, "sigmoid" if kind == "G" else "tanh")
    return net.eval()


def test_views_slot_wants_a_multi_view_netg():
    from monoport_amd import pipeline
    with pytest.raises(ValueError, match="single-view"):
        pipeline.ViewsSlot(_net("G", 1), "cpu")
    with pytest.raises(ValueError, match="view=3"):
        pipeline.ViewsSlot(_net("G", 3), "cpu", view=3)
    with pytest.raises(ValueError):
        pipeline.ViewsSlot(_net("G", 3), "cpu", projection="fisheye")


def test_views_slot_refuses_colours():
    from monoport_amd import pipeline
    net_g = _net("G", 2)
    for net_c in (_net("C", 1), _net("C", 2)):
        with pytest.raises(NotImplementedError, match="netC"):
            pipeline.ViewsSlot(net_g, "cpu", netC=net_c)
    with pytest.raises(NotImplementedError, match="colours"):
        pipeline.ViewsSlot(net_g, "cpu", mesh={"normals": "accumulate", "colors": True})


def test_frame_pipeline_takes_the_slot_class():
    from monoport_amd import pipeline
    with pytest.raises(NotImplementedError, match="ViewsSlot"):  # the default stays FrameSlot, whose message names the new class
        pipeline.FramePipeline(_net("G", 2), "cpu")
    with pytest.raises(ValueError, match="single-view"):
        pipeline.FramePipeline(_net("G", 1), "cpu", slot_class=pipeline.ViewsSlot)


def test_bindings_that_batch_together():
    """Two ViewsBindings share a recon_views_batch call iff head, V, view, projection (and map size) agree;
    ``batchable`` -- "a frame of recon_batch" -- stays False."""
    from monoport_amd.modeling.MonoPortNet import QueryBinding, ViewsBinding

    class Head:
        precision = "f32"

    head, other = Head(), Head()
    maps = [torch.zeros(4, 4, 256)] * 3
    a = ViewsBinding(None, head, maps, "calibs a", 2, projection=0)
    b = ViewsBinding(None, head, list(maps), "calibs b", 2, projection=0)
    assert not a.batchable and not b.batchable
    assert a.batch_key(1) == b.batch_key(1) and a.batch_key() == b.batch_key(0)
    assert a.batch_key(0) != b.batch_key(1)                                                      # view
    assert a.batch_key(0) != ViewsBinding(None, other, maps, "c", 2, projection=0).batch_key(0)  # head
    assert a.batch_key(0) != ViewsBinding(None, head, maps[:2], "c", 2, projection=0).batch_key(0)  # V
    assert a.batch_key(0) != ViewsBinding(None, head, maps, "c", 2, projection=1).batch_key(0)   # projection
    assert a.batch_key(0) != ViewsBinding(None, head, [torch.zeros(4, 8, 256)] * 3, "c", 2, projection=0).batch_key(0)
    assert callable(ViewsBinding.batch_many) and not hasattr(QueryBinding, "batch_many")
    with pytest.raises(ValueError, match="differ"):
        ViewsBinding.batch_many([a, ViewsBinding(None, head, maps[:2], "c", 2, projection=0)], [-1] * 3, [1] * 3,
                                [17, 33], 0.5, "dilate3")


def test_max_view_frames():
    from monoport_amd import _lib, ops
    assert [ops.max_view_frames(v) for v in (2, 3, 4, 8)] == [32, 21, 16, 8]
    assert ops.max_view_frames(1) == ops.MAX_FRAMES == 32 and ops.MAX_FRAME_VIEWS == _lib.MAX_FRAME_VIEWS == 64


def test_recon_views_batch_checks_its_lists_before_any_device_work():
    from monoport_amd import ops

    class Mlp:
        ctx = None

    maps = [[torch.zeros(4, 4, 256)] * 3] * 2
    cal = torch.eye(4)[None, None].repeat(2, 3, 1, 1)
    for bad_maps, bad_cal in (([], cal), (maps, cal[:1]), ([maps[0], maps[1][:2]], cal), ([maps[0]] * 22, [cal[0]] * 22),
                              ([[torch.zeros(4, 4, 256)] * 9], cal[:1])):
        with pytest.raises(ValueError, match="recon_views_batch"):
            ops.recon_views_batch(Mlp(), bad_maps, bad_cal, "orthogonal", 1.0, [-1] * 3, [1] * 3, [17, 33])
