"""FrameSlot.encode_pictures / jpegs and recon.encode_jpeg / picture_u8 on the GPU: the files a slot encodes behind its
pictures on its own stream equal recon.encode_jpeg of slot.pictures() byte for byte, and both equal the numpy
restatement (tests/jpeg_ref.py) on the pictures' floats -- without a scene, with one, with lighting, after an overflow
of the files' capacity and after a re-run mesh.  The smallest slot of the slot-picture tests: the synthetic body at 33^3,
pictures of 40 x 56 under 2 cameras, 3 frames of which one is empty.  Needs an MI355X."""
import numpy as np
import pytest

import jpeg_ref as ref
from test_mesh_batch_gpu import BMAX, BMIN, DEV, _body_hook, nets  # noqa: F401  (nets: the fixture)
from test_render_netc_gpu import RES, slot_frames
from test_shadow_gpu import slot_scene
from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, TWO
from test_views_slot_gpu import frames as views_frames, make_slot as make_views_slot, net as views_net  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
SIZE = (40, 56)
MESH = {"normals": "accumulate", "colors": False}


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def clay(recon):
    sh = np.random.RandomState(4).uniform(-0.3, 0.6, (9, 3)).astype(np.float32)
    return recon.Lighting(sh, direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), albedo=(0.8, 0.7, 0.6))


def make_slot(nets, scene=None, lighting=None):  # noqa: F811
    from monoport_amd.pipeline import FrameSlot
    pictures = dict(SLOT_PICTURES, res=SIZE, shade="normals")
    if scene is not None:
        pictures["scene"] = scene
    return FrameSlot(nets[0], torch.device(DEV), batch=3, resolutions=RES, b_min=BMIN, b_max=BMAX,
                     feature_hook=_body_hook(), mesh=MESH, pictures=pictures, lighting=lighting)


def restated(image, jpeg):
    """The files of an image tensor [views,H,W,3] by the numpy restatement."""
    x = image.cpu().numpy()
    return [ref.encode(x[v], jpeg.quality, jpeg.subsampling, jpeg.restart)[0] for v in range(x.shape[0])]


def check_jpegs(recon, slot, jpeg, live, scene):
    files, pics = slot.jpegs(), slot.pictures()
    assert len(files) == len(pics) == slot.n_active == len(live)
    for b, (f, pic) in enumerate(zip(files, pics)):
        if not live[b] and not scene:
            assert f is None and pic is None
            continue
        assert isinstance(f, list) and len(f) == 2 and all(isinstance(x, bytes) for x in f)
        assert f == recon.encode_jpeg(pic, jpeg) == restated(pic.image, jpeg), b
        assert f[0][:2] == b"\xff\xd8" and f[0][-2:] == b"\xff\xd9"
    return files


@pytest.mark.parametrize("kind", ["plain", "lit", "scene", "lit_scene"])
def test_slot_jpegs(recon, nets, kind):  # noqa: F811
    images, calibs = slot_frames()
    scene = slot_scene(recon) if "scene" in kind else None
    lighting = clay(recon) if "lit" in kind else None
    jpeg = recon.Jpeg(quality=90, subsampling="420" if kind != "lit" else "444")
    slot, bare = make_slot(nets, scene, lighting), make_slot(nets, scene, lighting)
    try:
        assert slot.jpeg is None and not hasattr(slot, "jpeg_bytes")
        slot.encode_pictures(jpeg)
        cap = jpeg.capacity_for(*SIZE)
        assert slot.jpeg is jpeg and tuple(slot.jpeg_bytes.shape) == (6, cap) and slot.jpeg_bytes.dtype == torch.uint8
        assert tuple(slot.jpeg_info.shape) == (6, 2) and slot.jpeg_info.dtype == torch.int32
        for s in (slot, bare):
            s.submit(images, calibs, cameras=TWO)
            s.wait()
        assert slot.status[:, 0].tolist() == [1, 0, 1]
        with pytest.raises(RuntimeError, match="before the first"):
            slot.encode_pictures(jpeg)
        files = check_jpegs(recon, slot, jpeg, (True, False, True), scene is not None)
        assert not slot.jpeg_info[:, 1].any()
        if scene is not None:  # the empty frame: the bare scene's file
            assert files[1] == recon.encode_jpeg(recon.render_scene(
                scene, TWO, SIZE, **{k: SLOT_PICTURES[k] for k in ("projection", "nearest", "near", "perspective_correct",
                                                                   "background")}), jpeg)
        # the slot on which encode_pictures was never called: nothing of it exists, the pictures are the same bits
        assert bare.jpeg is None and not hasattr(bare, "jpeg_bytes") and not hasattr(bare, "jpeg_info")
        with pytest.raises(RuntimeError, match="encode_pictures"):
            bare.jpegs()
        for p, q in zip(slot.pictures(), bare.pictures()):
            assert (p is None) == (q is None)
            assert p is None or torch.equal(p.image.view(torch.int32), q.image.view(torch.int32))
        # a short batch behind it
        slot.submit(images[:1], calibs[:1], cameras=TWO)
        short = check_jpegs(recon, slot, jpeg, (True,), scene is not None)
        assert short[0] == files[0]
    finally:
        slot.close()
        bare.close()


def test_a_capacity_too_small_encodes_again(recon, nets):  # noqa: F811
    images, calibs = slot_frames()
    scene = slot_scene(recon)
    roomy, tight = recon.Jpeg(quality=100, subsampling="444", restart=3), None
    slot, small = make_slot(nets, scene), make_slot(nets, scene)
    try:
        slot.encode_pictures(roomy)
        slot.submit(images, calibs, cameras=TWO)
        files = check_jpegs(recon, slot, roomy, (True, False, True), True)
        sizes = sorted(len(x) for f in files for x in f)
        assert sizes[0] < sizes[-1]
        # a capacity between the smallest and the largest file: some frames fit, some are encoded again
        tight = recon.Jpeg(quality=100, subsampling="444", restart=3, capacity=(sizes[0] + sizes[-1]) // 2)
        small.encode_pictures(tight)
        small.submit(images, calibs, cameras=TWO)
        small.wait()
        info = small.jpeg_info.cpu().numpy()
        assert 0 < info[:, 1].sum() < 6 and sorted(info[:, 0]) == sizes
        assert small.jpegs() == files
        # and with every file too large
        assert recon.encode_jpeg(slot.pictures()[0], recon.Jpeg(quality=100, subsampling="444", restart=3,
                                                               capacity=ref.HEADER_BYTES)) == files[0]
    finally:
        slot.close()
        small.close()


def test_a_rerun_frame_is_encoded_from_its_new_picture(recon, nets):  # noqa: F811
    """The mesh capacity cut behind a good submission, as the slot-picture tests do: ``jpegs()`` then encodes the picture
    ``pictures()`` renders from the re-run mesh, not the slot's own picture of the truncated one."""
    images, calibs = slot_frames()
    jpeg = recon.Jpeg(quality=75)
    slot = make_slot(nets)
    try:
        slot.encode_pictures(jpeg)
        slot.submit(images, calibs, cameras=TWO)
        first = check_jpegs(recon, slot, jpeg, (True, False, True), False)
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(3)
            slot._render_pictures(3)
            slot._encode_pictures(3)
        slot._busy = True
        again = slot.jpegs()
        assert slot._reran == [0, 2] and again == first
        own = slot.jpeg_info.cpu().numpy()
        assert slot.jpeg_bytes[0, :own[0, 0]].cpu().numpy().tobytes() != first[0][0]  # the truncated mesh's picture
    finally:
        slot.close()


def test_views_slot_jpegs(recon, views_net):  # noqa: F811
    images, calibs = views_frames()
    jpeg = recon.Jpeg(quality=50, restart=1)
    slot = make_views_slot(views_net, mesh={"normals": "accumulate"}, pictures=dict(SLOT_PICTURES, shade="normals"))
    try:
        slot.encode_pictures(jpeg)
        slot.submit(images, calibs, cameras=TWO)
        slot.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        files, pics = slot.jpegs(), slot.pictures()
        assert files[1] is None and files[0] == recon.encode_jpeg(pics[0], jpeg) == restated(pics[0].image, jpeg)
    finally:
        slot.close()


def test_encode_jpeg_and_picture_u8(recon):
    x = np.random.RandomState(3).uniform(-0.2, 1.2, (3, 17, 23, 3)).astype(np.float32)
    t = torch.from_numpy(x).to(DEV)
    jpeg = recon.Jpeg(quality=100, subsampling="444", restart=2, capacity=1024)  # the noise overflows 1 KB
    want = [ref.encode(x[i], 100, "444", 2)[0] for i in range(3)]
    assert min(len(w) for w in want) > 1024
    assert recon.encode_jpeg(t, jpeg) == want and recon.encode_jpeg(t) == [ref.encode(x[i])[0] for i in range(3)]
    one = recon.encode_jpeg(t[1], jpeg)
    assert isinstance(one, bytes) and one == want[1]
    assert recon.encode_jpeg(recon.MeshRender(t[0], None, None), jpeg) == want[0]
    assert recon.encode_jpeg(t[:, :, ::2][0], jpeg) == ref.encode(x[0, :, ::2], 100, "444", 2)[0]  # not contiguous
    u8 = recon.picture_u8(t)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), ref.to_u8(x))
