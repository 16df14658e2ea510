"""Anti-aliased pictures in the frame pipeline on the GPU: FrameSlot / ViewsSlot(pictures={"samples": s, ...}).  The
slot runs every pass and the composite in working buffers at s times the size and resolves once, behind them, on its own
stream; its pictures are held bit for bit to recon.render_mesh_many(_in_scene)(samples=s) on the meshes the slot hands
out, its JPEG files byte for byte to recon.encode_jpeg of those pictures.  The smallest slot of the slot-picture tests:
2 frames of which one is empty, and the first again after an overflow of its mesh capacity.  Needs an MI355X."""
import numpy as np
import pytest

from test_mesh_batch_gpu import nets  # noqa: F401  (the fixture)
from test_shadow_gpu import equal_pictures, slot_scene
from test_slot_pictures_gpu import PICTURES, SIZE, TWO, check_pictures, frames, make_slot
from test_views_slot_gpu import frames as views_frames, make_slot as make_views_slot, net as views_net  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
S = 2
FINE = (S * SIZE[0], S * SIZE[1])
MESH = {"normals": "accumulate", "colors": False}


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def clay(recon):
    sh = np.random.RandomState(4).uniform(-0.3, 0.6, (9, 3)).astype(np.float32)
    return recon.Lighting(sh, direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), albedo=(0.8, 0.7, 0.6))


def wanted(recon, slot, meshes, cameras, samples=S):
    """What the render calls give for the slot's own meshes under its options."""
    po = slot.picture_options
    args = (cameras, po.res, po.shade, po.projection, po.nearest, po.background, po.near, po.perspective_correct)
    if po.scene is None:
        return recon.render_mesh_many(meshes, *args, lighting=slot.lighting, samples=samples)
    return recon.render_mesh_many_in_scene(meshes, po.scene, *args, po.composite, lighting=slot.lighting, samples=samples)


@pytest.mark.parametrize("kind", ["plain", "lit_scene"])
def test_frame_slot_with_samples(recon, nets, kind):  # noqa: F811
    images, calibs = frames()
    scene = slot_scene(recon) if kind == "lit_scene" else None
    lighting = clay(recon) if kind == "lit_scene" else None
    opts = dict(PICTURES, shade="normals", samples=S)
    if scene is not None:
        opts["scene"] = scene
    jpeg = recon.Jpeg(quality=90)
    slot = make_slot(nets, MESH, opts, netc=False, lighting=lighting)
    try:
        po = slot.picture_options
        assert po.samples == S and po.raster.samples == S and po.res == SIZE
        # the working buffers are fine, the pictures the final size
        assert tuple(slot.fine_image.shape) == (2, 2) + FINE + (3,) and tuple(slot.fine_face.shape) == (2, 2) + FINE
        assert tuple(slot.pictures_image.shape) == (2, 2) + SIZE + (3,) and tuple(slot.pictures_face.shape) == (2, 2) + SIZE
        assert tuple(slot.pictures_coverage.shape) == (2, 2) + SIZE and slot.pictures_coverage.dtype == torch.float32
        if scene is None:
            assert slot.pictures_mask is None and slot.fine_mask is None
        else:
            assert tuple(slot.pictures_mask.shape) == (2, 2) + SIZE and tuple(slot.fine_mask.shape) == (2, 2) + FINE
            assert tuple(slot.scene_image.shape) == tuple(slot.scene_lit.shape) == (2, 2) + FINE + (3,)
            assert tuple(slot.light_normal.shape) == (2, 2) + FINE + (3,)
        slot.encode_pictures(jpeg)
        assert tuple(slot.jpeg_bytes.shape) == (4, jpeg.capacity_for(*SIZE))
        slot.submit(images, calibs, cameras=TWO)
        slot.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        meshes, pics = slot.meshes(), slot.pictures()
        want = wanted(recon, slot, meshes, TWO)
        assert meshes[1] is None and isinstance(pics[0], recon.ResolvedPicture) and isinstance(want[0], recon.ResolvedPicture)
        assert equal_pictures([t for t in pics[0] if t is not None], [t for t in want[0] if t is not None])
        assert [t is None for t in pics[0]] == [t is None for t in want[0]] == [False, False, False, scene is None, False]
        assert pics[0].image.data_ptr() == slot.pictures_image[0].data_ptr()  # views of the slot's buffers
        assert pics[0].coverage.data_ptr() == slot.pictures_coverage[0].data_ptr()
        cov = pics[0].coverage
        assert int(((cov > 0) & (cov < 1)).sum()) > 20 and int((cov == 1).sum()) > 60
        if scene is None:
            assert pics[1] is None and want[1] is None and not slot.pictures_coverage[1].any()
        else:  # the empty frame: the bare scene
            assert equal_pictures(pics[1], want[1]) and int(pics[1].mask.max()) == 1 and not pics[1].coverage.any()
            assert int((pics[0].mask == 1).sum()) > 20 and int((pics[0].mask == 2).sum()) > 20
        # the files: the resolved image, encoded behind the resolve
        files = slot.jpegs()
        assert files[0] == recon.encode_jpeg(want[0], jpeg) and len(files[0]) == 2 and files[0][0][:2] == b"\xff\xd8"
        assert files[1] == (None if scene is None else recon.encode_jpeg(want[1], jpeg))
        # a second submission gives the same bits
        first = [None if t is None else t.clone() for t in pics[0]]
        slot.submit(images, calibs, cameras=TWO)
        slot.wait()
        again = slot.pictures()[0]
        assert equal_pictures([t for t in again if t is not None], [t for t in first if t is not None])
        assert slot.jpegs() == files
        # a frame whose mesh overflowed the slot's capacities: every fine pass, the composite and the resolve again, from
        # the re-run mesh, into fresh tensors -- the bits of the full-capacity submission
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
            slot._render_pictures(2)
            slot._encode_pictures(2)
        slot._busy = True
        rerun = slot.pictures()
        assert slot._reran == [0] and isinstance(rerun[0], recon.ResolvedPicture)
        assert equal_pictures([t for t in rerun[0] if t is not None], [t for t in first if t is not None])
        assert rerun[0].image.data_ptr() != slot.pictures_image[0].data_ptr()
        assert not torch.equal(slot.pictures_face[0], first[2])  # the slot's own buffers: 200 faces of the body
        assert slot.jpegs() == files
    finally:
        slot.close()


def test_slots_without_samples_are_as_before(recon, nets):  # noqa: F811
    images, calibs = frames()
    opts = dict(PICTURES, shade="normals")
    absent = make_slot(nets, MESH, opts, netc=False)
    one = make_slot(nets, MESH, dict(opts, samples=1), netc=False)
    try:
        for slot in (absent, one):
            assert slot.picture_options.samples == 1 and slot.pictures_coverage is None
            assert not any(hasattr(slot, k) for k in ("fine_image", "fine_depth", "fine_face", "fine_mask"))
            slot.submit(images, calibs, cameras=TWO)
        # the parent's construction: render_mesh without the keyword, on MeshRenders
        a = check_pictures(absent, TWO, what="no samples")
        b = check_pictures(one, TWO, what="samples=1")
        want = wanted(recon, absent, absent.meshes(), TWO, samples=1)
        assert isinstance(a[0], recon.MeshRender) and equal_pictures(a[0], b[0]) and equal_pictures(a[0], want[0])
    finally:
        absent.close()
        one.close()


def test_option_refusals(nets):  # noqa: F811
    for samples in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="samples must be"):
            make_slot(nets, MESH, dict(PICTURES, shade="normals", samples=samples), netc=False)
    with pytest.raises(ValueError, match="outside 1..4096"):
        make_slot(nets, MESH, dict(PICTURES, shade="normals", res=(1025, 8), samples=4), netc=False)


def test_views_slot_with_samples(recon, views_net):  # noqa: F811
    images, calibs = views_frames()
    slot = make_views_slot(views_net, mesh={"normals": "accumulate"}, pictures=dict(PICTURES, shade="normals", samples=S))
    try:
        assert slot.picture_options.samples == S and tuple(slot.pictures_coverage.shape) == (2, 2) + SIZE
        slot.submit(images, calibs, cameras=TWO)
        slot.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        meshes, pics = slot.meshes(), slot.pictures()
        want = wanted(recon, slot, meshes, TWO)
        assert pics[1] is None and isinstance(pics[0], recon.ResolvedPicture) and pics[0].mask is None
        assert equal_pictures([t for t in pics[0] if t is not None], [t for t in want[0] if t is not None])
        assert int(((pics[0].coverage > 0) & (pics[0].coverage < 1)).sum()) > 20
    finally:
        slot.close()
