"""What the multi-view colour path refuses before any device work: the list checks of ops.query_views_counted_batch, the
construction of pipeline.ColorViewsSlot and the ``view`` keyword of recon.reconstruct_mesh / reconstruct_mesh_many.  No
GPU: every call here must raise before it reaches the library."""
import pytest

torch = pytest.importorskip("torch")


class Mlp:
    ctx = None  # a call that got as far as the library would fail on this with AttributeError


def _frames(n, v_n, cap=10):
    maps = [[torch.zeros((4, 6, 512)) for _ in range(v_n)] for _ in range(n)]
    points = [torch.zeros((3, cap)) for _ in range(n)]
    counts = [torch.zeros(1, dtype=torch.int32) for _ in range(n)]
    calibs = torch.eye(4)[None, None].repeat(n, v_n, 1, 1)
    return maps, points, counts, calibs


def _call(maps, points, counts, calibs, **kw):
    from monoport_amd import ops
    return ops.query_views_counted_batch(Mlp(), maps, points, counts, calibs, "orthogonal", 1.28, **kw)


def test_list_checks_come_before_device_work():
    from monoport_amd import ops
    maps, points, counts, calibs = _frames(3, 2)
    who = "query_views_counted_batch"
    with pytest.raises(ValueError, match=who):  # no frames at all
        _call([], [], [], [])
    for change in (dict(points=points[:2]), dict(counts=counts[:2]), dict(calibs=calibs[:2])):  # wrong lengths
        with pytest.raises(ValueError, match=who):
            _call(**dict(dict(maps=maps, points=points, counts=counts, calibs=calibs), **change))
    with pytest.raises(ValueError, match=who):  # a frame with another number of views
        _call([maps[0], maps[1][:1], maps[2]], points, counts, calibs)
    with pytest.raises(ValueError, match=who):  # calibrations of another number of views
        _call(maps, points, counts, [calibs[0], calibs[1][:1], calibs[2]])
    with pytest.raises(ValueError, match=who):  # more than MP_MAX_VIEWS views
        m9, p9, c9, k9 = _frames(1, 9)
        _call(m9, p9, c9, k9)
    with pytest.raises(ValueError, match=who + ".*float32 \\[3,10\\]"):  # mixed capacities
        _call(maps, [points[0], torch.zeros((3, 11)), points[2]], counts, calibs)
    with pytest.raises(ValueError, match=who + ".*contiguous"):  # points that are not contiguous
        _call(maps, [points[0], torch.zeros((10, 3)).t(), points[2]], counts, calibs)
    with pytest.raises(ValueError, match=who):  # points of another type
        _call(maps, [points[0], points[1].double(), points[2]], counts, calibs)
    with pytest.raises(ValueError, match=who + ".*int32"):
        _call(maps, points, [counts[0], counts[1].long(), counts[2]], calibs)
    with pytest.raises(ValueError, match=who):  # maps of two sizes
        _call([maps[0], [torch.zeros((4, 8, 512))] * 2, maps[2]], points, counts, calibs)
    with pytest.raises(ValueError, match=who):  # outputs: wrong number, wrong capacity
        _call(maps, points, counts, calibs, outs=[torch.zeros((3, 10))] * 2)
    with pytest.raises(ValueError, match=who):
        _call(maps, points, counts, calibs, outs=[torch.zeros((3, 11))] * 3)
    for v_n in (2, 3, 8):  # more than max_view_frames(V) frames
        most = ops.max_view_frames(v_n)
        assert most == min(32, 64 // v_n)
        with pytest.raises(ValueError, match=who + ".*1\\.\\.%d frames of %d views" % (most, v_n)):
            _call(*_frames(most + 1, v_n))


def _nets():
    from monoport_amd.modeling import PIFuNetC, PIFuNetG, heads

    def net(kind, v_n):
        n = PIFuNetG() if kind == "G" else PIFuNetC()
        ch = heads.PIFuNetGMLP().filter_channels if kind == "G" else heads.PIFuNetCMLP().filter_channels
        n.surface_classifier = heads.SurfaceClassifier(ch, v_n, False, "sigmoid" if kind == "G" else "tanh")
        return n.eval()

    return net


def test_color_views_slot_construction_refusals(monkeypatch):
    from monoport_amd import pipeline
    net = _nets()
    g1, g2, c1, c2, c3 = net("G", 1), net("G", 2), net("C", 1), net("C", 2), net("C", 3)

    def no_stream(*a, **k):
        raise AssertionError("the slot allocated before it had checked its heads")

    monkeypatch.setattr(torch.cuda, "Stream", no_stream)
    kw = dict(batch=2, resolutions=(17, 33))
    with pytest.raises(ValueError, match="netC is required"):
        pipeline.ColorViewsSlot(g2, "cpu", **kw)
    with pytest.raises(ValueError, match="num_views = 1"):
        pipeline.ColorViewsSlot(g2, "cpu", netC=c1, **kw)
    with pytest.raises(ValueError, match="num_views = 3, netG has 2"):
        pipeline.ColorViewsSlot(g2, "cpu", netC=c3, **kw)
    with pytest.raises(ValueError, match="single-view head"):
        pipeline.ColorViewsSlot(g1, "cpu", netC=c2, **kw)
    with pytest.raises(ValueError, match="view=2"):
        pipeline.ColorViewsSlot(g2, "cpu", netC=c2, view=2, **kw)
    with pytest.raises(ValueError, match="unknown keys"):  # the option records too come before any allocation
        pipeline.ColorViewsSlot(g2, "cpu", netC=c2, mesh={"colours": True}, **kw)
    with pytest.raises(ValueError, match="cameras|views"):
        pipeline.ColorViewsSlot(g2, "cpu", netC=c2, mesh={"colors": True}, pictures={"views": 0}, **kw)
    # the slots without colours refuse what they refused before
    with pytest.raises(NotImplementedError, match="netC"):
        pipeline.ViewsSlot(g2, "cpu", netC=c2, **kw)
    with pytest.raises(NotImplementedError, match="colours need netC"):
        pipeline.ViewsSlot(g2, "cpu", mesh={"colors": True}, **kw)
    with pytest.raises(NotImplementedError, match="multi-view head"):
        pipeline.FrameSlot(g1, "cpu", netC=c2, **kw)


def test_reconstruct_mesh_view_validation():
    from monoport_amd import recon
    net = _nets()
    c1, c2 = net("C", 1), net("C", 2)
    sdf = torch.zeros((9, 9, 9))  # on the CPU: a call that passed the checks would fail in the library, not here
    feats = [[torch.zeros((2, 512, 4, 4))]]
    calib = torch.eye(4)[None].repeat(2, 1, 1)
    for call, extra in ((recon.reconstruct_mesh, dict(feat_tensor_C=feats, calib_tensor=calib)),
                        (lambda s, **k: recon.reconstruct_mesh_many([s, None], **k),
                         dict(feat_tensors_C=[feats, None], calib_tensors=[calib, None]))):
        with pytest.raises(NotImplementedError, match="vertex_colors"):  # view=None keeps today's refusal
            call(sdf, netC=c2, **extra)
        with pytest.raises(ValueError, match="multi-view netC"):  # view= with a single-view head
            call(sdf, netC=c1, view=0, **extra)
        for view in (-1, 2, 1.0, True, "0"):
            with pytest.raises(ValueError, match="view must be an int in 0..1"):
                call(sdf, netC=c2, view=view, **extra)
        with pytest.raises(ValueError, match="no netC"):
            call(sdf, view=0)
    assert recon.reconstruct_mesh(None, netC=c2, view=5) is None  # nothing to mesh: nothing is looked at, as before
    with pytest.raises(ValueError, match="needs feat_tensors_C"):
        recon.reconstruct_mesh_many([sdf], netC=c2, view=0)
