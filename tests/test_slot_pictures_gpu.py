"""Free-viewpoint pictures in the frame pipeline on the GPU: FrameSlot / ViewsSlot(pictures=...), submit(cameras=...) and
slot.pictures().  Every picture the slot makes behind its mesh chain -- from its own mesh buffers and device counts,
without a host value in between -- is held bit for bit to recon.render_mesh on the mesh slot.meshes() hands out.
Needs an MI355X."""
import math

import pytest

import mesh_render_clip_ref as clip_ref
from monoport_amd import synthetic as syn
from test_mesh_batch_gpu import BMAX, BMIN, DEV, _body_hook, nets  # noqa: F401  (nets: the fixture)
from test_mesh_render_clip_gpu import CAMERAS, assert_same, camera_space
from test_views_slot_gpu import V, frames as views_frames, make_slot as make_views_slot, net as views_net  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
RES = (17, 33, 65)
SIZE = (40, 24)
# the body fills the box [-1, 1]^3; the "front" camera sees it at z = 2 .. 4 and "turned" at 1.6 .. 3.6: the plane cuts it
PICTURES = dict(views=2, res=SIZE, projection="perspective", nearest="min", near=2.7, perspective_correct=True,
                background=0.25)
TWO = torch.stack([CAMERAS["front"], CAMERAS["turned"]])


def other_cameras():
    c = TWO.flip(0).clone()
    c[:, 0, 3] += 0.3
    return c


def frames():
    """Frame 0: a synthetic body.  Frame 1: a camera that looks past the box, so its coarsest level is empty."""
    from monoport_amd.recon import pifu_calib
    images = torch.stack([torch.from_numpy(syn.synthetic_image(0)), torch.zeros(3, 512, 512)]).to(DEV)
    away = torch.eye(4, device=DEV)[None]
    away[0, 0, 3] = 5.0
    return images, [pifu_calib(*syn.scene_camera(0), device=DEV), away]


def make_slot(nets, mesh, pictures, netc=True, **kw):
    from monoport_amd.pipeline import FrameSlot
    return FrameSlot(nets[0], torch.device(DEV), netC=nets[1] if netc else None, batch=2, resolutions=RES, b_min=BMIN,
                     b_max=BMAX, feature_hook=_body_hook(), mesh=mesh, pictures=pictures, **kw)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_pictures(slot, cameras, live=(True, False), what=""):
    """slot.pictures() against recon.render_mesh of slot.meshes(), frame by frame; returns the pictures."""
    from monoport_amd.recon import MeshRender, render_mesh
    po = slot.picture_options
    meshes, pics = slot.meshes(), slot.pictures()
    assert len(meshes) == len(pics) == slot.n_active == len(live), what
    cameras = cameras if cameras.dim() == 4 else cameras[None].expand(len(pics), -1, -1, -1)
    for b, (mesh, pic) in enumerate(zip(meshes, pics)):
        if not live[b]:
            assert mesh is None and pic is None, (what, b)
            assert slot.pictures_image is None or (slot.pictures_image[b] == po.background).all()
            assert (slot.pictures_depth[b] == 0).all() and (slot.pictures_face[b] == -1).all()
            continue
        assert isinstance(pic, MeshRender) and tuple(pic.depth.shape) == (po.views,) + po.res, (what, b)
        assert pic.depth.data_ptr() == slot.pictures_depth[b].data_ptr()  # a view of the slot's buffer
        want = render_mesh(mesh, cameras[b], po.res, po.shade, po.projection, po.nearest, po.background, po.near,
                           po.perspective_correct)
        assert bits_equal(pic.depth, want.depth) and torch.equal(pic.face, want.face), (what, b)
        assert (pic.face >= 0).sum() > 60 * po.views, (what, b)
        assert (pic.image is None) == (po.shade is None)
        if po.shade == "normals":
            assert bits_equal(pic.image, want.image), (what, b)
    return pics


def test_slot_pictures_normals(nets):
    from monoport_amd.recon import render_mesh
    images, calibs = frames()
    slot = make_slot(nets, {"normals": "accumulate"}, dict(PICTURES, shade="normals"))
    plain = make_slot(nets, {"normals": "accumulate"}, None)
    try:
        assert slot.picture_options.views == 2 and tuple(slot.pictures_image.shape) == (2, 2) + SIZE + (3,)
        assert plain.picture_options is None and plain.pictures_depth is None
        with pytest.raises(RuntimeError):
            plain.pictures()
        with pytest.raises(ValueError, match="cameras"):
            slot.submit(images, calibs)
        with pytest.raises(ValueError, match="cameras"):
            plain.submit(images, calibs, cameras=TWO)
        with pytest.raises(ValueError, match="cameras"):
            slot.submit(images, calibs, cameras=TWO[:1])
        slot.submit(images, calibs, cameras=TWO)  # one camera set for all frames
        slot.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        first = [t.clone() for t in check_pictures(slot, TWO, what="shared cameras")[0]]
        mesh = slot.meshes()[0]
        unclipped = render_mesh(mesh, TWO, SIZE, "normals", "perspective", "min", 0.25)
        assert not torch.equal(unclipped.face, first[2])  # the plane does cut
        # the slot without pictures computes the same meshes
        plain.submit(images, calibs)
        assert torch.equal(plain.meshes()[0].verts, mesh.verts)
        # a second submission with other cameras, per frame, overwrites the first
        per_frame = torch.stack([other_cameras(), TWO])
        slot.submit(images, calibs, cameras=per_frame)
        second = check_pictures(slot, per_frame, what="per-frame cameras")[0]
        assert not torch.equal(second.face, first[2])
        # a short batch: one frame
        slot.submit(images[:1], calibs[:1], cameras=TWO[None])
        short = check_pictures(slot, TWO[None], live=(True,), what="short")[0]
        for a, b in zip(short, first):
            assert bits_equal(a, b)
    finally:
        slot.close()
        plain.close()


@pytest.mark.parametrize("mesh", [{"normals": "accumulate", "simplify": 16}, {"normals": "accumulate", "smooth": 2}],
                         ids=["simplify16", "smooth2"])
def test_slot_pictures_of_the_final_mesh(nets, mesh):
    images, calibs = frames()
    slot = make_slot(nets, dict(mesh, colors=False), dict(PICTURES, shade="normals"), netc=False)
    try:
        slot.submit(images, calibs, cameras=TWO)
        check_pictures(slot, TWO, what=str(mesh))
        key = "simple_verts" if "simplify" in mesh else "smooth_verts"
        assert slot.meshes()[0].verts.data_ptr() == slot.mesh_buffers[key].data_ptr()
    finally:
        slot.close()


def test_overflowed_frame_is_rendered_again(nets):
    """The slot's capacity cut to 100 vertices / 200 faces behind a good submission: ``meshes()`` makes the frame's mesh
    again with exact capacities, and ``pictures()`` renders that mesh into fresh tensors -- the bits of the picture the
    slot made at full capacity, while the slot's own buffers hold the picture of the truncated mesh."""
    images, calibs = frames()
    slot = make_slot(nets, {"normals": "accumulate", "colors": False}, dict(PICTURES, shade="normals"), netc=False)
    try:
        slot.submit(images, calibs, cameras=TWO)
        first = [t.clone() for t in check_pictures(slot, TWO, what="full capacity")[0]]
        assert slot._reran == []
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
            slot._render_pictures(2)
        slot._busy = True
        again = slot.pictures()
        assert slot._reran == [0] and again[1] is None
        for a, b, own in zip(again[0], first, (slot.pictures_image, slot.pictures_depth, slot.pictures_face)):
            assert bits_equal(a, b) and a.data_ptr() != own[0].data_ptr()
        assert not torch.equal(slot.pictures_face[0], first[2])  # 200 of its faces alone
    finally:
        slot.close()


def test_slot_pictures_colors(nets):
    """shade="colors": the slot paints netC's raw predictions [3,cap] as a * 0.5 + 0.5 behind the interpolation, where
    render_mesh interpolates the finished colours p * 0.5 + 0.5 of the Mesh.  Depth and face ids are the same bits; the
    image is the same bits as the rasteriser's own call on the slot's buffers, and within 5e-6 of render_mesh's: both are
    the same real number, |p| <= 1 (tanh), each a dozen f32 roundings (6e-8) away from it."""
    from monoport_amd import ops
    from monoport_amd.recon import render_mesh
    images, calibs = frames()
    slot = make_slot(nets, {"normals": None}, dict(PICTURES, views=1))
    try:
        assert slot.picture_options.shade == "colors" and slot.mesh.colors
        cam = CAMERAS["turned"][None]
        slot.submit(images, calibs, cameras=cam)
        pic = check_pictures(slot, cam, what="colors")[0]
        mesh = slot.meshes()[0]
        po = slot.picture_options
        want = render_mesh(mesh, cam, SIZE, "colors", po.projection, po.nearest, po.background, po.near, True)
        hit = pic.face >= 0
        assert (pic.image[~hit] == 0.25).all() and float((pic.image - want.image).abs().max()) < 5e-6
        assert float(pic.image[hit].min()) >= 0 and float(pic.image[hit].max()) <= 1 and pic.image[hit].std() > 0.01
        raw = ops.mesh_render_raw(slot.mesh_buffers["verts"][0], slot.mesh_buffers["faces"][0],
                                  slot.mesh_buffers["counts"][0], slot.mesh_buffers["preds"][0], cam, SIZE, "perspective",
                                  "min", channel_major=True, scale=0.5, bias=0.5, background=0.25, near=po.near,
                                  perspective_correct=True)
        assert bits_equal(raw[0], pic.image)
        # and, independently of the device's rasteriser: the restatement fed the raw predictions, channel-major
        nv, nf = slot.mesh_buffers["counts"][0].cpu().tolist()
        xyz = camera_space(ops, slot.mesh_buffers["verts"][0][:nv], cam[0])
        ref = clip_ref.render(xyz, slot.mesh_buffers["faces"][0][:nf].cpu().numpy(), *SIZE, po.near, True,
                              attr=slot.mesh_buffers["preds"][0][:, :nv].cpu().numpy(), channel_major=True,
                              nearest="min", scale=0.5, bias=0.5, background=0.25)
        assert all((ref.kind == k).sum() >= 10 for k in range(4))
        assert_same([pic.image[0], pic.depth[0], pic.face[0]], ref, "colours against the restatement")
    finally:
        slot.close()


def test_slot_pictures_under_a_graph(nets):
    images, calibs = frames()
    opts = dict(PICTURES, shade="normals")
    eager = make_slot(nets, {"normals": "accumulate"}, opts)
    graphed = make_slot(nets, {"normals": "accumulate"}, opts, use_graph=True)
    try:
        graphed.prepare()
        assert graphed.graph is not None
        for slot in (eager, graphed):
            slot.submit(images, calibs, cameras=TWO)
        a, b = check_pictures(eager, TWO)[0], check_pictures(graphed, TWO, what="graph")[0]
        for x, y in zip(a, b):
            assert bits_equal(x, y)
    finally:
        eager.close()
        graphed.close()


def test_views_slot_pictures(views_net):
    images, calibs = views_frames()
    slot = make_views_slot(views_net, mesh={"normals": "accumulate"}, pictures=dict(PICTURES, shade="normals"))
    try:
        assert slot.views == V and slot.picture_options.views == 2
        slot.submit(images, calibs, cameras=TWO)
        slot.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        check_pictures(slot, TWO, what="ViewsSlot")
    finally:
        slot.close()


def test_no_shading_and_orthogonal_pictures(nets):
    """shade=None allocates no image; the unclipped orthogonal call goes the same way."""
    images, calibs = frames()
    slot = make_slot(nets, {"normals": None, "colors": False}, dict(views=1, res=33, shade=None), netc=False)
    try:
        assert slot.pictures_image is None and slot.picture_options.near is None
        cam = torch.eye(4)[None]
        slot.submit(images, calibs, cameras=torch.eye(4))  # [4,4]: the one camera of every frame
        pic = check_pictures(slot, cam, what="orthogonal")[0]
        assert pic.image is None and math.isfinite(float(pic.depth.sum()))
    finally:
        slot.close()
