"""FrameSlot.encode_pictures(recon.Png) / pngs and recon.encode_png on the GPU: the files a slot encodes behind its
pictures on its own stream equal recon.encode_png of slot.pictures() byte for byte, and both equal the numpy restatement
(tests/png_ref.py) on the pictures' floats -- RGB, RGBA from the subject's mask and from the coverage of anti-aliased
pictures (unmatted), 16-bit depth; with a scene, a Jpeg beside the Png, an empty frame, a capacity too small and a re-run
mesh; in FrameSlot, ViewsSlot and ColorViewsSlot.  The slots of the JPEG and anti-aliasing slot tests.  Needs an MI355X."""
import io

import numpy as np
import pytest
from PIL import Image

import png_ref as ref
from test_color_views_slot_gpu import colour_slot, netc  # noqa: F401  (netc: the fixture)
from test_jpeg_slot_gpu import SIZE, clay, make_slot
from test_mesh_batch_gpu import DEV, nets  # noqa: F401  (nets: the fixture)
from test_render_netc_gpu import slot_frames
from test_shadow_gpu import slot_scene
from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE as SMALL, TWO, frames as two_frames
from test_slot_pictures_gpu import make_slot as make_small_slot
from test_views_slot_gpu import frames as views_frames, make_slot as make_views_slot, net  # noqa: F401
from test_views_slot_gpu import net as views_net  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
MESH = {"normals": "accumulate", "colors": False}


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def restated(pic, png):
    """The files of a picture of the slot ([views, ...] tensors) by the numpy restatement."""
    if png.plane == "depth":
        d = pic.depth.cpu().numpy()
        return [ref.encode(d[v], "gray16", png.filter, lo=png.lo, scale=png.scale)[0] for v in range(d.shape[0])]
    x = pic.image.cpu().numpy()
    alpha = None
    if png.alpha == "coverage":
        alpha = pic.coverage.cpu().numpy()
    elif png.alpha == "subject":
        mask = getattr(pic, "mask", None)
        alpha = ((pic.face >= 0) if mask is None else (mask == 2)).cpu().numpy().astype(np.float32)
    return [ref.encode(x[v], png.format, png.filter, None if alpha is None else alpha[v], png.unmatte)[0]
            for v in range(x.shape[0])]


def check_pngs(recon, slot, png, live, scene=False):
    files, pics = slot.pngs(), slot.pictures()
    assert len(files) == len(pics) == slot.n_active == len(live)
    for b, (f, pic) in enumerate(zip(files, pics)):
        if not live[b] and not scene:
            assert f is None and pic is None
            continue
        assert isinstance(f, list) and len(f) == slot.picture_options.views and all(isinstance(x, bytes) for x in f)
        assert f == recon.encode_png(pic, png) == restated(pic, png), b
        assert f[0][:8] == ref.SIGNATURE and f[0][-8:-4] == b"IEND"
    return files


@pytest.mark.parametrize("kind", ["plain", "lit_scene"])
def test_slot_pngs_beside_jpegs(recon, nets, kind):  # noqa: F811
    """RGB without a scene, RGBA from the composite's mask with one; the slot has a Jpeg too, whose files are those of a
    slot with the Jpeg alone."""
    images, calibs = slot_frames()
    scene = slot_scene(recon) if kind == "lit_scene" else None
    lighting = clay(recon) if kind == "lit_scene" else None
    png = recon.Png(alpha="subject", filter="paeth") if scene is not None else recon.Png()
    jpeg = recon.Jpeg(quality=90)
    slot, only = make_slot(nets, scene, lighting), make_slot(nets, scene, lighting)
    try:
        assert slot.png is None and not hasattr(slot, "png_bytes")
        slot.encode_pictures(jpeg)
        slot.encode_pictures(png)
        only.encode_pictures(jpeg)
        cap = png.capacity_for(*SIZE)
        assert slot.png is png and slot.jpeg is jpeg and tuple(slot.png_bytes.shape) == (6, cap)
        assert slot.png_bytes.dtype == torch.uint8 and tuple(slot.png_info.shape) == (6, 2)
        assert hasattr(slot, "png_alpha") == (scene is not None)
        assert only.png is None and not hasattr(only, "png_bytes") and not hasattr(only, "png_info")
        for s in (slot, only):
            s.submit(images, calibs, cameras=TWO)
            s.wait()
        assert slot.status[:, 0].tolist() == [1, 0, 1]
        with pytest.raises(RuntimeError, match="before the first"):
            slot.encode_pictures(png)
        with pytest.raises(RuntimeError, match="encode_pictures"):
            only.pngs()
        files = check_pngs(recon, slot, png, (True, False, True), scene is not None)
        assert not slot.png_info[:, 1].any()
        assert slot.jpegs() == only.jpegs()
        if scene is not None:  # the subject shows somewhere, and not everywhere
            a = np.asarray(Image.open(io.BytesIO(files[0][0])))[..., 3]
            assert set(np.unique(a)) == {0, 255}
        # a short batch behind it
        slot.submit(images[:1], calibs[:1], cameras=TWO)
        assert check_pngs(recon, slot, png, (True,), scene is not None)[0] == files[0]
    finally:
        slot.close()
        only.close()


def test_coverage_alpha_unmatted_composites_like_a_render(recon, nets):  # noqa: F811
    """Anti-aliased pictures over background 0.25 as RGBA with the coverage, unmatted; a frame with an empty mesh; a
    frame whose mesh is made again.  Decoded and put over 0.8, a file is the picture rendered over 0.8 within 1 / 255
    plus the 8-bit rounding of alpha, 0.5 / 255 (the colour byte is off by at most 0.5 / 255 times alpha, the alpha byte
    by at most 0.5 / 255 times |colour - 0.8|; the f32 rounding of the unmatte is far below)."""
    images, calibs = two_frames()
    opts = dict(SLOT_PICTURES, shade="normals", samples=2)
    png = recon.Png(alpha="coverage", unmatte=SLOT_PICTURES["background"])
    slot = make_small_slot(nets, MESH, opts, netc=False)
    over = make_small_slot(nets, MESH, dict(opts, background=0.8), netc=False)
    try:
        slot.encode_pictures(png)
        for s in (slot, over):
            s.submit(images, calibs, cameras=TWO)
            s.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        files = check_pngs(recon, slot, png, (True, False))
        want = over.pictures()[0].image.cpu().numpy()
        cov = slot.pictures()[0].coverage.cpu().numpy()
        assert int(((cov > 0) & (cov < 1)).sum()) > 20
        for v in range(2):
            rgba = np.asarray(Image.open(io.BytesIO(files[0][v]))).astype(np.float64) / 255.0
            assert rgba.shape == SMALL + (4,)
            put = rgba[..., 3:] * rgba[..., :3] + (1.0 - rgba[..., 3:]) * 0.8
            err = np.abs(put - want[v]).max()
            print("composite over 0.8 against the render over 0.8, view %d: max error %.6f" % (v, err))
            assert err <= 1.0 / 255 + 0.5 / 255
        # the mesh capacity cut behind the good submission: pngs() encodes the picture of the re-run mesh
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
            slot._render_pictures(2)
            slot._encode_png(2)
        slot._busy = True
        again = slot.pngs()
        assert slot._reran == [0] and again == files
        own = slot.png_info.cpu().numpy()
        assert slot.png_bytes[0, :own[0, 0]].cpu().numpy().tobytes() != files[0][0]  # the truncated mesh's picture
    finally:
        slot.close()
        over.close()


def test_a_capacity_too_small_encodes_again(recon, nets):  # noqa: F811
    images, calibs = slot_frames()
    scene = slot_scene(recon)
    roomy = recon.Png(filter="sub")
    slot, small = make_slot(nets, scene), make_slot(nets, scene)
    try:
        slot.encode_pictures(roomy)
        slot.submit(images, calibs, cameras=TWO)
        files = check_pngs(recon, slot, roomy, (True, False, True), True)
        sizes = sorted(len(x) for f in files for x in f)
        assert sizes[0] < sizes[-1]
        tight = recon.Png(filter="sub", capacity=(sizes[0] + sizes[-1]) // 2)
        small.encode_pictures(tight)
        small.submit(images, calibs, cameras=TWO)
        small.wait()
        info = small.png_info.cpu().numpy()
        assert 0 < info[:, 1].sum() < 6 and sorted(info[:, 0]) == sizes
        assert small.pngs() == files
        # and with every file too large
        assert recon.encode_png(slot.pictures()[0], recon.Png(filter="sub", capacity=ref.MIN_BYTES)) == files[0]
    finally:
        slot.close()
        small.close()


def test_views_slot_depth_pngs(recon, views_net):  # noqa: F811
    """The depth picture as 16-bit grey, from a slot without a shade."""
    images, calibs = views_frames()
    png = recon.Png(plane="depth", depth_range=(1.0, 5.0))
    slot = make_views_slot(views_net, mesh={"normals": "accumulate"}, pictures=dict(SLOT_PICTURES, shade=None))
    try:
        slot.encode_pictures(png)
        with pytest.raises(ValueError, match="shade=None"):
            slot.encode_pictures(recon.Png())
        slot.submit(images, calibs, cameras=TWO)
        slot.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        files = check_pngs(recon, slot, png, (True, False))
        d = np.asarray(Image.open(io.BytesIO(files[0][0])))
        assert d.dtype == np.uint16 and np.array_equal(d, ref.to_u16(slot.pictures()[0].depth[0].cpu().numpy(), png.lo,
                                                                     png.scale))
        assert len(np.unique(d)) > 50
    finally:
        slot.close()


def test_color_views_slot_pngs(recon, net, netc):  # noqa: F811
    images, calibs = views_frames()
    png = recon.Png(alpha="subject", unmatte=1.0)
    slot = colour_slot(net, netc, pictures={"views": 1, "res": 33, "shade": "colors"})
    try:
        slot.encode_pictures(png)
        slot.submit(images, calibs, cameras=torch.eye(4)[None])
        slot.wait()
        files = check_pngs(recon, slot, png, (True, False))
        assert len(files[0]) == 1
    finally:
        slot.close()


def test_encode_png_and_the_samples(recon):
    x = np.random.RandomState(3).uniform(-0.2, 1.2, (3, 17, 23, 3)).astype(np.float32)
    a = np.random.RandomState(4).uniform(-0.2, 1.2, (3, 17, 23)).astype(np.float32)
    t, ta = torch.from_numpy(x).to(DEV), torch.from_numpy(a).to(DEV)
    png = recon.Png(filter="none", capacity=256)  # the noise overflows 256 bytes
    want = [ref.encode(x[i], "rgb8", "none")[0] for i in range(3)]
    assert min(len(w) for w in want) > 256
    assert recon.encode_png(t, png) == want and recon.encode_png(t) == [ref.encode(x[i])[0] for i in range(3)]
    one = recon.encode_png(t[1], png)
    assert isinstance(one, bytes) and one == want[1]
    assert recon.encode_png(recon.MeshRender(t[0], None, None), png) == want[0]
    assert recon.encode_png(t[:, :, ::2][0], png) == ref.encode(x[0, :, ::2], "rgb8", "none")[0]  # not contiguous
    rgba = recon.Png(alpha="coverage", unmatte=0.5)
    assert recon.encode_png(t, rgba, alpha=ta) == [ref.encode(x[i], "rgba8", "adaptive", a[i], 0.5)[0] for i in range(3)]
    assert recon.encode_png(t[2], rgba, alpha=ta[2]) == ref.encode(x[2], "rgba8", "adaptive", a[2], 0.5)[0]
    depth = recon.Png(plane="depth", depth_range=(0.25, 0.75))
    assert recon.encode_png(ta, depth) == [ref.encode(a[i], "gray16", lo=0.25, scale=2.0)[0] for i in range(3)]
    picture = recon.MeshRender(t[0], ta[0], (ta[0] > 0.5).int() - 1)
    assert recon.encode_png(picture, depth) == ref.encode(a[0], "gray16", lo=0.25, scale=2.0)[0]
    assert recon.encode_png(picture, recon.Png(alpha="subject")) == ref.encode(
        x[0], "rgba8", alpha=(a[0] > 0.5).astype(np.float32))[0]
    u16 = recon.picture_u16(ta, 0.25, 0.75)
    assert u16.dtype == torch.uint16 and np.array_equal(u16.cpu().numpy(), ref.to_u16(a, 0.25, 2.0))
    u8 = recon.picture_rgba8(t, ta, unmatte=0.5)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), ref.to_rgba8(x, a, 0.5))
