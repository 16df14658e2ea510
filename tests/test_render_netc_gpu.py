"""Pictures coloured per pixel on the GPU: recon.render_mesh(_many)(shade="netC") and FrameSlot / ColorViewsSlot
(pictures={"shade": "netC"}).  Depth and face ids are held to the shade=None call, the image to the counted netC query
on the point list that the numpy restatement (tests/picture_ref.py) makes of the position picture, bit for bit; the
slots to recon.render_mesh on the meshes they hand out.  Needs an MI355X."""
import numpy as np
import pytest

import picture_ref as ref
import test_query_views_gpu as tv
from monoport_amd import synthetic as syn
from test_color_views_slot_gpu import colour_slot, netc as views_netc, own_maps  # noqa: F401  (netc: the fixture)
from test_mesh_batch_gpu import BMAX, BMIN, _body_hook, _seeded_netC, nets  # noqa: F401  (nets: the fixture)
from test_views_slot_gpu import V, frames as views_frames, make_slot as make_views_slot, net as views_net  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BACKGROUND = 0.25


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def mesh33(recon):
    """The 33^3 body of test_mesh_render_gpu.py as a Mesh with neither normals nor colours."""
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    mesh = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, normals=None)
    assert mesh.normals is None and mesh.colors is None and mesh.verts.shape[0] > 500
    return mesh


@pytest.fixture(scope="module")
def heads():
    """The seeded netC under an orthogonal and under a perspective input calibration, and its maps: 48 x 80 and square."""
    from monoport_amd.modeling import geometry
    persp = _seeded_netC()
    persp.projection = geometry.perspective
    return {"nets": {"orthogonal": _seeded_netC(), "perspective": persp},
            "calibs": {"orthogonal": (torch.eye(4, device=DEV) * 0.9)[None].contiguous(),
                       "perspective": torch.tensor([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 1.0, 3.0], [0, 0, 0, 1.0]],
                                                   device=DEV)[None]},
            "maps": {"48x80": [[torch.from_numpy(syn.rand_feat(512, 48, 80, 63))[None].to(DEV)]],
                     "64x64": [[torch.from_numpy(syn.rand_feat(512, 64, 64, 64))[None].to(DEV)]]}}


def picture_cameras():
    turned = torch.eye(4)
    a = np.deg2rad(35.0)
    turned[0, 0], turned[0, 2], turned[2, 0], turned[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    turned[:3] *= 0.9
    near = torch.eye(4)
    near[0, 0] = near[1, 1] = 1.5
    near[:3, 3] = torch.tensor([0.1, 0.0, 1.2])  # the body at z = 0.6 .. 1.7: the plane at 0.9 cuts it
    return {"orthogonal": dict(calibs=torch.stack([torch.eye(4), turned]), res=(40, 24), projection="orthogonal",
                               nearest="max"),
            "clipped": dict(calibs=near, res=33, projection="perspective", nearest="min", near=0.9,
                            perspective_correct=True)}


def want_image(ops, recon, mesh, cam, binding, query):
    """shade=None's depth and face, and the image the definition gives: the position picture (the mesh's vertices as its
    colours), the restatement's list of its covered pixels, ``query`` on that list, the restatement's paint."""
    plain = recon.render_mesh(mesh, shade=None, background=BACKGROUND, **cam)
    position = recon.render_mesh(mesh._replace(colors=mesh.verts), shade="colors", background=BACKGROUND, **cam)
    assert torch.equal(position.face, plain.face)
    face, pos = plain.face.cpu().numpy(), position.image.cpu().numpy()
    pts, pix, count = ref.points(face, pos)
    preds = query(binding, torch.from_numpy(pts).to(DEV), torch.from_numpy(count).to(DEV))
    image = ref.paint(preds.cpu().numpy(), pix, count, pos.copy())
    return plain, image, int(count[1])


def single_view_query(ops):
    def query(b, pts, count):
        if b.projection == ops.PROJECTIONS["orthogonal"]:
            return ops.query_counted(b.mlp, b.feat_hwc, pts, count, b.calib, b.z_scale)
        return ops.query_counted_batch(b.mlp, [b.feat_hwc], [pts], [count], [b.calib], b.z_scale,
                                       projections=[b.projection])[0]
    return query


@pytest.mark.parametrize("camera", ["orthogonal", "clipped"])
@pytest.mark.parametrize("maps", ["48x80", "64x64"])
@pytest.mark.parametrize("calibration", ["orthogonal", "perspective"])
def test_render_mesh_netc(ops, recon, mesh33, heads, calibration, maps, camera):
    net, calib, feat = heads["nets"][calibration], heads["calibs"][calibration], heads["maps"][maps]
    cam = picture_cameras()[camera]
    got = recon.render_mesh(mesh33, shade="netC", background=BACKGROUND, netC=net, feat_tensor_C=feat, calib_tensor=calib,
                            **cam)
    binding = recon._bind_netC("test", net, [(feat, calib, torch.device(DEV))])[0]
    assert binding.projection == ops.PROJECTIONS[calibration]
    plain, image, covered = want_image(ops, recon, mesh33, cam, binding, single_view_query(ops))
    n_pix = plain.face.numel()
    print("%s / %s / %s: %d of %d pixels covered" % (calibration, maps, camera, covered, n_pix))
    assert covered >= 100 and n_pix - covered >= 100
    assert bits_equal(got.depth, plain.depth) and torch.equal(got.face, plain.face)
    assert got.image.shape == plain.face.shape + (3,)
    assert np.array_equal(bits(got.image), bits(image))
    hit = got.face >= 0
    assert bool((got.image[~hit] == BACKGROUND).all())
    assert float(got.image[hit].min()) >= 0 and float(got.image[hit].max()) <= 1 and float(got.image[hit].std()) > 0.01


def test_render_mesh_many_netc(ops, recon, mesh33, heads):
    """A None mesh in the list, per-mesh cameras, feature maps and calibrations == the per-mesh calls."""
    net, feat = heads["nets"]["orthogonal"], heads["maps"]["48x80"]
    other = recon.Mesh(mesh33.verts[:900].contiguous(), mesh33.faces[(mesh33.faces < 900).all(1)].contiguous(), None, None)
    cams = picture_cameras()["orthogonal"]["calibs"]
    meshes = [mesh33, None, other]
    calibs = [cams, None, cams.flip(0).contiguous()]
    in_calibs = [heads["calibs"]["orthogonal"], None, torch.eye(4, device=DEV)[None]]
    feats = [feat, None, heads["maps"]["48x80"]]
    got = recon.render_mesh_many(meshes, calibs, (40, 24), "netC", background=BACKGROUND, netC=net, feat_tensors_C=feats,
                                 calib_tensors=in_calibs)
    assert len(got) == 3 and got[1] is None
    for i in (0, 2):
        want = recon.render_mesh(meshes[i], calibs[i], (40, 24), "netC", background=BACKGROUND, netC=net,
                                 feat_tensor_C=feats[i], calib_tensor=in_calibs[i])
        assert int((want.face >= 0).sum()) >= 100
        for a, b in zip(got[i], want):
            assert bits_equal(a, b), i
    assert not bits_equal(got[0].image, got[2].image)
    # one camera set for all meshes, one [4,4] camera: no leading views dimension
    one = recon.render_mesh_many([other], cams[1], 33, "netC", netC=net, feat_tensors_C=[feat], calib_tensors=[in_calibs[0]])
    assert tuple(one[0].image.shape) == (33, 33, 3) and tuple(one[0].face.shape) == (33, 33)


def test_multi_view_head(ops, recon, mesh33):
    """view=k of a V = 2 head: row k of ops.query_views on the same points."""
    net2 = tv._net("C", syn.rand_mlp("C", 61, 2.0), V)
    feat = [[torch.from_numpy(np.stack([syn.rand_feat(512, 48, 80, 70 + v) for v in range(V)])).to(DEV)]]
    calibs = torch.stack([torch.eye(4) * 0.9, torch.eye(4)]).to(DEV)
    calibs[1, 0, 3] = -0.7  # view 1 sees part of the body (x in -0.55 .. 0.24) left of its image: row 1 is masked there
    cam = picture_cameras()["orthogonal"]
    images = []
    for k in range(V):
        got = recon.render_mesh(mesh33, shade="netC", background=BACKGROUND, netC=net2, feat_tensor_C=feat,
                                calib_tensor=calibs, view=k, **cam)
        binding = recon._bind_netC("test", net2, [(feat, calibs, torch.device(DEV))], view=k)[0]

        def query(b, pts, count, k=k):
            n = int(count[0])
            out = torch.zeros_like(pts)
            out[:, :n] = ops.query_views(b.mlp, b.maps, pts[:, :n][None].expand(V, 3, n), b.calibs, b.projection,
                                         b.z_scale)[k]
            return out

        plain, image, covered = want_image(ops, recon, mesh33, cam, binding, query)
        assert covered >= 100
        assert bits_equal(got.depth, plain.depth) and torch.equal(got.face, plain.face)
        assert np.array_equal(bits(got.image), bits(image)), k
        images.append(got.image)
    assert not torch.equal(images[0], images[1])
    single = _seeded_netC()
    with pytest.raises(ValueError, match="multi-view"):
        recon.render_mesh(mesh33, shade="netC", netC=single, feat_tensor_C=feat, calib_tensor=calibs, view=0, **cam)
    with pytest.raises(NotImplementedError, match="view="):
        recon.render_mesh(mesh33, shade="netC", netC=net2, feat_tensor_C=feat, calib_tensor=calibs, **cam)


def test_agreement_with_vertex_colours(recon, heads):
    """A sanity check, not on the bits: on the un-simplified 33^3 mesh the picture coloured per pixel and the picture of
    the per-vertex colours cover the same pixels and both stay in [0, 1]; how far they differ is printed (DESIGN.md
    section 4.8.7 records it), no tolerance is fixed."""
    net, calib, feat = heads["nets"]["orthogonal"], heads["calibs"]["orthogonal"], heads["maps"]["64x64"]
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    mesh = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, normals=None, netC=net, feat_tensor_C=feat, calib_tensor=calib)
    cam = picture_cameras()["orthogonal"]
    today = recon.render_mesh(mesh, shade="colors", **cam)
    deferred = recon.render_mesh(mesh, shade="netC", netC=net, feat_tensor_C=feat, calib_tensor=calib, **cam)
    assert torch.equal(today.face, deferred.face) and bits_equal(today.depth, deferred.depth)
    hit = today.face >= 0
    assert int(hit.sum()) >= 100
    for pic in (today, deferred):
        assert float(pic.image[hit].min()) >= 0 and float(pic.image[hit].max()) <= 1
        assert bool((pic.image[~hit] == 1.0).all())
    diff = (today.image - deferred.image).abs()
    print("per-pixel netC against interpolated vertex colours, 33^3 mesh, random 64x64 maps: max abs difference %.4f, "
          "mean %.4f over %d covered pixels" % (float(diff[hit].max()), float(diff[hit].mean()), int(hit.sum())))


# ---- the slots --------------------------------------------------------------------------------------------------------
RES = (9, 17, 33)
PICTURES = {"shade": "netC", "views": 2, "res": (40, 24)}


def slot_frames():
    """Frame 0: a synthetic body.  Frame 1: a camera that looks past the box, so its coarsest level is empty.  Frame 2:
    the body under another camera."""
    from monoport_amd.recon import pifu_calib
    images = torch.stack([torch.from_numpy(syn.synthetic_image(0)), torch.zeros(3, 512, 512),
                          torch.from_numpy(syn.synthetic_image(3))]).to(DEV)
    away = torch.eye(4, device=DEV)[None]
    away[0, 0, 3] = 5.0
    return images, [pifu_calib(*syn.scene_camera(0), device=DEV), away, pifu_calib(*syn.scene_camera(3), device=DEV)]


def slot_cameras(n):
    cams = picture_cameras()["orthogonal"]["calibs"]
    per_frame = torch.stack([cams] * n).clone()
    for f in range(n):
        per_frame[f, :, 0, 3] += 0.05 * f
    return per_frame


def count_colour_queries(ops, monkeypatch):
    """-> the list that every counted colour query and every vertex -> point-list call from now on appends (its kind,
    the capacity of its point lists) to."""
    calls = []
    for kind, where in (("query_counted", 2), ("query_counted_batch", 2), ("query_views_counted_batch", 2),
                        ("mesh_points_raw_batch", 0)):
        def counted(*args, _real=getattr(ops, kind), _kind=kind, _where=where, **kw):
            arg = args[_where]
            calls.append((_kind, (arg[0] if isinstance(arg, (list, tuple)) else arg).shape[-1]))
            return _real(*args, **kw)

        monkeypatch.setattr(ops, kind, counted)
    return calls


def test_frame_slot(ops, recon, nets, monkeypatch):
    from monoport_amd.pipeline import FrameSlot
    images, calibs = slot_frames()
    cameras = slot_cameras(3)
    slot = FrameSlot(nets[0], torch.device(DEV), netC=nets[1], batch=3, resolutions=RES, b_min=BMIN, b_max=BMAX,
                     feature_hook=_body_hook(), mesh={"colors": False}, pictures=dict(PICTURES, background=BACKGROUND))
    try:
        n_pix = 2 * 40 * 24
        assert not slot.mesh.colors and "preds" not in slot.mesh_buffers and "points" not in slot.mesh_buffers
        assert {k: tuple(v.shape) for k, v in slot.picture_lists.items()} == {
            "points": (3, 3, n_pix), "pixels": (3, n_pix), "preds": (3, 3, n_pix), "count": (3, 2)}
        assert sum(v[0].numel() * v.element_size() for v in slot.picture_lists.values()) == 28 * n_pix + 8
        calls = count_colour_queries(ops, monkeypatch)
        slot.submit(images, calibs, cameras=cameras)
        slot.wait()
        monkeypatch.undo()
        assert slot.status[:, 0].tolist() == [1, 0, 1]
        # the colour queries of the submission: the textured render's over the r^2 columns, the pictures' over their
        # pixels -- none over the mesh's vertex capacity, and no vertex list was made
        assert sorted(set(calls)) == [("query_counted_batch", 33 * 33), ("query_counted_batch", n_pix)], calls
        meshes, pics = slot.meshes(), slot.pictures()
        assert meshes[1] is None and pics[1] is None and meshes[0].colors is None
        assert bool((slot.pictures_image[1] == BACKGROUND).all()) and bool((slot.pictures_face[1] == -1).all())
        assert slot.picture_lists["count"].tolist()[1] == [0, 0]
        for b in (0, 2):
            nchw = slot.feats_hwc_c[b].permute(2, 0, 1)[None].contiguous()
            want = recon.render_mesh(meshes[b], cameras[b], (40, 24), "netC", background=BACKGROUND, netC=slot.netC,
                                     feat_tensor_C=[[nchw]], calib_tensor=slot.calib[b:b + 1])
            covered = int((want.face >= 0).sum())
            print("FrameSlot frame %d: %d of %d pixels covered, %d vertices" % (b, covered, n_pix, meshes[b].verts.shape[0]))
            assert covered >= 100 and slot.picture_lists["count"].tolist()[b] == [covered, covered]
            assert pics[b].image.data_ptr() == slot.pictures_image[b].data_ptr()
            for a, w in zip(pics[b], want):
                assert bits_equal(a, w), b
            hit = want.face >= 0
            assert float(want.image[hit].std()) > 0.01 and bool((pics[b].image[~hit] == BACKGROUND).all())
        first = [t.clone() for t in pics[0]]
        # a second, short submission reproduces frame 0
        slot.submit(images[:1], calibs[:1], cameras=cameras[:1])
        again = slot.pictures()
        assert len(again) == 1
        for a, b in zip(again[0], first):
            assert bits_equal(a, b)
        # a mesh that overflowed the slot's capacities is rendered again from the re-run mesh: the same bits
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(1)
            slot._render_pictures(1)
        slot._busy = True
        rerun = slot.pictures()
        assert slot._reran == [0]
        for a, b, own in zip(rerun[0], first, (slot.pictures_image, slot.pictures_depth, slot.pictures_face)):
            assert bits_equal(a, b) and a.data_ptr() != own[0].data_ptr()
    finally:
        slot.close()


def test_color_views_slot(ops, recon, views_net, views_netc, monkeypatch):
    images, calibs = views_frames()
    cameras = slot_cameras(2)
    slot = colour_slot(views_net, views_netc, mesh={"normals": None, "colors": False},
                       pictures=dict(PICTURES, background=BACKGROUND))
    try:
        n_pix = 2 * 40 * 24
        calls = count_colour_queries(ops, monkeypatch)
        slot.submit(images, calibs, cameras=cameras)
        slot.wait()
        monkeypatch.undo()
        assert slot.status[:, 0].tolist() == [1, 0]
        assert sorted(set(calls)) == [("query_views_counted_batch", n_pix), ("query_views_counted_batch", 65 * 65)], calls  # 1920 < 4225
        meshes, pics = slot.meshes(), slot.pictures()
        assert meshes[1] is None and pics[1] is None and meshes[0].colors is None
        nchw = torch.stack(own_maps(slot, 0)).permute(0, 3, 1, 2).contiguous()
        want = recon.render_mesh(meshes[0], cameras[0], (40, 24), "netC", background=BACKGROUND, netC=slot.netC,
                                 feat_tensor_C=[[nchw]], calib_tensor=slot.calib_in[0], view=slot.view)
        covered = int((want.face >= 0).sum())
        print("ColorViewsSlot frame 0: %d of %d pixels covered" % (covered, n_pix))
        assert covered >= 100
        for a, w in zip(pics[0], want):
            assert bits_equal(a, w)
        assert float(want.image[want.face >= 0].std()) > 0.01
    finally:
        slot.close()


def test_views_slot_refuses(views_net):
    with pytest.raises(ValueError, match="netC"):
        make_views_slot(views_net, mesh={"normals": None}, pictures=PICTURES)
