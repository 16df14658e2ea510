"""The multi-view frame pipeline on the GPU: pipeline.ViewsSlot (n frames x V views: one encoder pass, the octree
through ops.recon_views_batch, then the per-volume stages) and Seg3dLossless(fuse_views=True).forward_many.  Every
result is held, bit for bit, to the per-frame calls fed the slot's own maps and calibrations.  Needs an MI355X."""
import warnings

import numpy as np
import pytest

import test_query_views_gpu as tv
import test_recon_views_gpu as rv
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
RES = [17, 33, 65]
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
V = 2


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops
    return ops


@pytest.fixture(scope="module")
def net():
    """The multi-view netG of test_recon_views_gpu (body head, V views) with seeded encoder weights."""
    net = tv._net("G", syn.body_mlp("G", noise=0.05, seed=251), V)
    shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
    net.image_filter.load_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in syn.seeded_state_dict(shapes, 71).items()})
    return net


def body_hook():
    """Channels 0 / 1 of every image's map are the body's depth planes (bench.make_pipeline's synthetic-data hook)."""
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(DEV)
    planes_hwc = planes.permute(1, 2, 0).contiguous()

    def hook(feat):
        feat[:, 0:2].copy_(planes[None].expand(feat.shape[0], -1, -1, -1))

    def hook_hwc(feat_hwc):
        feat_hwc[..., 0:2].copy_(planes_hwc[None].expand(feat_hwc.shape[0], -1, -1, -1))

    hook.hwc = hook_hwc
    return hook


def frames():
    """Two frames of V views: a live one, and one whose camera `view` = 0 looks past the box (every value 0)."""
    images = torch.from_numpy(np.stack([[syn.synthetic_image(10 * f + v) for v in range(V)] for f in range(2)])).to(DEV)
    calibs = torch.from_numpy(np.stack([tv.calibs_of(dict(proj="orthogonal", steps=[6 * v + 7 * f for v in range(V)]))
                                        for f in range(2)])).to(DEV)
    calibs[1, 0, 0, 3] = 5.0
    return images, calibs


def make_slot(net, batch=2, **kw):
    from monoport_amd.pipeline import ViewsSlot
    return ViewsSlot(net, torch.device(DEV), batch=batch, resolutions=RES, b_min=LO, b_max=HI, feature_hook=body_hook(),
                     **kw)


def vertices_equal(a, b):
    ca, cb = int(a[4].item()), int(b[4].item())
    return ca == cb and all(torch.equal(a[k][:ca], b[k][:cb]) for k in range(4))


def same_mesh(got, want, what):
    from monoport_amd.recon import Mesh
    assert isinstance(got, Mesh) and isinstance(want, Mesh), what
    for name, a, b in zip(Mesh._fields, got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, name)


def own_frame(ops, slot, f):
    """ops.recon_views on the slot's OWN maps and calibrations of frame f -> (volume, status list)"""
    mlp = slot.net.surface_classifier.packed()
    vol, st = ops.recon_views(mlp, slot.feats_hwc[f * V:(f + 1) * V], slot.calib_in[f], "orthogonal", syn.Z_SCALE, LO, HI,
                              RES, view=slot.view)
    return vol, st.tolist()


# ---- 1. reconstruction ------------------------------------------------------------------------------------------------
def test_views_slot_reconstruction(ops, net):
    from monoport_amd.recon import reconstruct_mesh
    images, calibs = frames()
    slot = make_slot(net, mesh={"normals": "accumulate"})
    try:
        assert slot.views == V and slot.tables is None and tuple(slot.image.shape) == (2 * V, 3, 512, 512)
        slot.submit(images, calibs)
        slot.wait()
        status = slot.status.tolist()
        print("ViewsSlot: status %s" % status)
        assert status[0][0] == 1 and min(status[0][1:]) > 0 and status[1] == [0, 17 ** 3, 0, 0]
        assert torch.equal(slot.calib_in[:2], calibs)
        maps = torch.stack(slot.feats_hwc)
        assert not torch.equal(maps[0], maps[1])  # the views' maps differ: the encoder saw batch * V images
        for f in range(2):
            vol, st = own_frame(ops, slot, f)
            assert st == status[f]
            if f == 0:
                assert torch.equal(vol, slot.volumes[0]) and bool((vol > 0.5).any()) and bool((vol < 0.5).any())
        vol = slot.volumes[0]
        raw = ops.forward_vertices_raw(vol, "front")
        x, y, z, nrm, count = raw
        assert int(count.item()) > 100 and vertices_equal(raw, slot.vertices[0])
        assert torch.equal(ops.paint(x, y, nrm, 0, count, RES[-1], 0.5, 0.5, 0.0, 1.0), slot.renders[0])
        meshes = slot.meshes()
        assert len(meshes) == 2 and meshes[1] is None
        same_mesh(meshes[0], reconstruct_mesh(vol, 0.5, LO, HI, normals="accumulate"), "slot frame 0")
        assert meshes[0].verts.shape[0] > 500 and meshes[0].colors is None
    finally:
        slot.close()


# ---- 2. lifecycle -------------------------------------------------------------------------------------------------------
def test_views_slot_lifecycle(ops, net):
    from monoport_amd.pipeline import FramePipeline, ViewsSlot
    images, calibs = frames()
    live_i, live_c = images[[0, 0]].clone(), calibs[[0, 0]].clone()
    live_c[1, :, 0, 3] += 0.05  # a second live frame, shifted a little
    slot = make_slot(net)
    graphed = make_slot(net, use_graph=True)
    pipe = FramePipeline(net, torch.device(DEV), depth=1, batch=2, slot_class=ViewsSlot, resolutions=RES, b_min=LO,
                         b_max=HI, feature_hook=body_hook())
    try:
        slot.submit(live_i, live_c)
        slot.wait()
        first = ([v.clone() for v in slot.volumes], slot.status.tolist())
        print("two live frames: %s" % first[1])
        assert first[1][0][0] == 1 and first[1][1][0] == 1 and not torch.equal(first[0][0], first[0][1])
        for f in range(2):
            vol, st = own_frame(ops, slot, f)
            assert st == first[1][f] and torch.equal(vol, slot.volumes[f])
        # a short batch: one frame of two (the encoder still runs the slot's batch; the octree sees one frame)
        slot.submit(live_i[1:], live_c[1:])
        slot.wait()
        vol, st = own_frame(ops, slot, 0)
        assert slot.n_active == 1 and st[0] == 1 and slot.status[0].tolist() == st and torch.equal(slot.volumes[0], vol)
        assert torch.equal(slot.calib_in[0], live_c[1])
        # a second submit overwrites the first
        slot.submit(images, calibs)
        slot.wait()
        assert slot.status[1].tolist() == [0, 17 ** 3, 0, 0] and slot.status[0].tolist() == first[1][0]
        assert torch.equal(slot.volumes[0], first[0][0])
        # the encoder as a hipGraph: the same bits as eager
        graphed.prepare()
        graphed.submit(live_i, live_c)
        graphed.wait()
        assert graphed.graph is not None and graphed.status.tolist() == first[1]
        assert all(torch.equal(a, b) for a, b in zip(graphed.volumes, first[0]))
        assert torch.equal(graphed.renders[1], ops.paint(*[graphed.vertices[1][k] for k in (0, 1, 3)], 0,
                                                         graphed.vertices[1][4], RES[-1], 0.5, 0.5, 0.0, 1.0))
        # FramePipeline with the slot class as a keyword
        got = pipe.submit(live_i, live_c)
        got.wait()
        assert isinstance(got, ViewsSlot) and got.status.tolist() == first[1]
        assert all(torch.equal(a, b) for a, b in zip(got.volumes, first[0]))
    finally:
        slot.close()
        graphed.close()
        pipe.close()


# ---- 3. the coalescing engine path ----------------------------------------------------------------------------------------
def _count_calls(ops, monkeypatch):
    """-> the list that every fused multi-view reconstruction from now on appends its kind to."""
    kinds = []
    for kind in ("recon_views", "recon_views_batch"):
        def counted(*args, _real=getattr(ops, kind), _kind=kind, **kw):
            kinds.append(_kind)
            return _real(*args, **kw)

        monkeypatch.setattr(ops, kind, counted)
    return kinds


def test_forward_many_batches_multi_view_frames(ops, monkeypatch):
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    net3, feats3, calib3 = rv.body_case(3)
    net2, feats2, calib2 = rv.body_case(2)
    shifted = []
    for f in range(3):
        c = calib3.clone()
        c[:, 0, 3] += 0.04 * f
        shifted.append(c)
    shifted[2][1, 0, 3] += 0.7  # view 1 partly off its image: rows 0 and 1 differ (test_view_row_selection)
    state = dict(row=0)

    def query_func(points, im_feat_list, calib_tensor, head):
        head_net, v_n = head
        samples = points.repeat(v_n, 1, 1).permute(0, 2, 1)
        return head_net.query(im_feat_list, points=samples, calibs=calib_tensor)[0][state["row"]:state["row"] + 1]

    kws3 = [dict(im_feat_list=feats3, calib_tensor=c, head=(net3, 3)) for c in shifted]
    kw2 = dict(im_feat_list=feats2, calib_tensor=calib2, head=(net2, 2))

    def fresh(kw, row=0):
        state["row"] = row
        try:
            return rv.engine(query_func, RES, fuse_views=True, view=row)(**kw).clone()
        finally:
            state["row"] = 0

    want3 = [fresh(kw) for kw in kws3]
    want2 = fresh(kw2)
    want_row1 = [fresh(kw, row=1) for kw in kws3]
    assert not torch.equal(want3[0], want3[1]) and not torch.equal(want3[2], want_row1[2])

    eng = rv.engine(query_func, RES, fuse_views=True, validate="first")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for _ in range(Seg3dLossless.VALIDATE_CALLS):
            assert torch.equal(eng(**kws3[0]), want3[0]) and eng.last_path == "fused"
        kinds = _count_calls(ops, monkeypatch)
        # trusted: three frames, ONE batched call
        out = eng.forward_many(kws3)
        assert kinds == ["recon_views_batch"], kinds
        assert eng.last_path == "fused" and all(torch.equal(o, w) for o, w in zip(out, want3))
        assert eng.last_status.tolist()[0] == 1
        # a frame of another head with V = 2 among them: frame by frame, validated again, the right volumes
        del kinds[:]
        out = eng.forward_many([kws3[0], kw2, kws3[1]])
        assert "recon_views_batch" not in kinds and kinds.count("recon_views") == 3, kinds
        assert torch.equal(out[0], want3[0]) and torch.equal(out[1], want2) and torch.equal(out[2], want3[1])
        # the caller switches to row 1 and says so: the old trust does not cover it
        for _ in range(Seg3dLossless.VALIDATE_CALLS):
            eng(**kws3[0])
        del kinds[:]
        state["row"], eng.view = 1, 1
        out = eng.forward_many(kws3)
        assert "recon_views_batch" not in kinds and kinds.count("recon_views") == 3, kinds
        assert all(torch.equal(o, w) for o, w in zip(out, want_row1))
        # ... and once validated, row 1 is batched too
        del kinds[:]
        out = eng.forward_many(kws3)
        assert kinds == ["recon_views_batch"] and all(torch.equal(o, w) for o, w in zip(out, want_row1))
