"""The scene behind the subject on the GPU: mp_texture_mips, mp_picture_texture(_batch), mp_picture_composite(_batch)
(csrc/scene.hip), ops.texture_mips / picture_texture_batch / picture_composite_batch / render_scene_batch, recon.Scene,
render_scene, composite, render_mesh_many_in_scene, and FrameSlot(pictures={"scene": ...}).  Every comparison is
array_equal on the bits against the numpy restatement of the definitions (tests/scene_ref.py); the UV pictures come from
the real rasteriser.  Needs an MI355X."""
import ctypes
import math
import os

import numpy as np
import pytest

import scene_ref as ref
from monoport_amd import synthetic as syn
from test_mesh_batch_gpu import nets  # noqa: F401  (the fixture)
from test_mesh_render_gpu import ARG, DEV, OK, bits, host

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
SIZES = [(1, 1), (2, 2), (5, 3), (64, 64), (8, 1)]
PICTURES = [(33, 20), (20, 48)]
TEXTURES = [(5, 3), (64, 64)]
WRAPS = {"repeat": ref.WRAP_REPEAT, "clamp": ref.WRAP_CLAMP}
NEAR = 1.5
BG = 0.25


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def procedural(ht, wt):
    """A checker plus a ramp, float32 [ht,wt,3] in [0.05, 1]."""
    i, j = np.meshgrid(np.arange(ht), np.arange(wt), indexing="ij")
    tex = np.empty((ht, wt, 3), F)
    tex[..., 0] = 0.2 + 0.8 * (((i // 2) + (j // 2)) % 2)
    tex[..., 1] = 0.05 + 0.95 * (j + 1) / wt
    tex[..., 2] = 0.05 + 0.95 * (i + 1) / ht
    return tex


def tilted(angle, focal=2.0, t=(0.0, 0.0, 2.5), orthogonal=False):
    """A camera turned about x by ``angle``: [4,4] float32, the rows of [R|t] under diag(focal, focal, 1)."""
    c, s = math.cos(angle), math.sin(angle)
    m = np.eye(4, dtype=np.float64)
    m[:3, :3] = np.diag([focal, focal, 1.0]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    m[:3, 3] = t
    if orthogonal:  # keep z inside a friendly range
        m[2] *= 0.3
    return torch.from_numpy(m.astype(F))


def floor_mesh(y=-0.1, nan_uv=True):
    """A floor of two triangles over x in [-1.5, 0], a packed copy (vertices of its own) over x in [0, 1.5] whose uv do
    not continue the first one's -- a uv seam along x = 0 --, uv over [-1.5, 2.5], and a triangle on the cameras' side of the
    far edge (they look up at the floor from below) with one NaN uv.  -> verts [V,3], faces [F,3], uv [V,2]"""
    quad = lambda x0, x1: [[x0, y, -1.5], [x1, y, -1.5], [x1, y, 1.5], [x0, y, 1.5]]  # noqa: E731
    verts = quad(-1.5, 0.0)
    uv = [[-1.5, -1.5], [0.5, -1.5], [0.5, 2.5], [-1.5, 2.5]]
    faces = [[0, 1, 2], [0, 2, 3]]
    a = quad(0.0, 1.5)
    b = [[1.0, -0.5], [2.5, -0.5], [2.5, 1.75], [1.0, 1.75]]
    for tri in ([0, 1, 2], [0, 2, 3]):  # packed: three rows per face
        faces.append([len(verts) + k for k in range(3)])
        verts += [a[k] for k in tri]
        uv += [b[k] for k in tri]
    if nan_uv:
        faces.append([len(verts) + k for k in range(3)])
        verts += [[-0.4, y - 0.2, 1.4], [0.4, y - 0.2, 1.4], [0.0, y - 0.8, 1.4]]
        uv += [[0.0, 0.0], [1.0, 0.0], [math.nan, 1.0]]
    return np.array(verts, F), np.array(faces, np.int32), np.array(uv, F)


CAMS = torch.stack([tilted(0.5), tilted(0.9, focal=1.6, t=(0.1, -0.2, 2.2))])


@pytest.fixture(scope="module")
def floor(ops):
    verts, faces, uv = floor_mesh()
    attr = np.zeros((len(verts), 3), F)
    attr[:, :2] = uv
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return dict(verts=dev(verts), faces=dev(faces), attr=dev(attr), uv=uv,
                counts=torch.tensor([len(verts), len(faces)], dtype=torch.int32, device=DEV), pictures={}, pyramids={})


def uv_picture(ops, floor, size, cams=CAMS):
    """(uv [2,H,W,3], depth, face [2,H,W]) of the floor by the real rasteriser: clipped, perspective-correct."""
    key = (size, cams.shape[0])
    if key not in floor["pictures"]:
        floor["pictures"][key] = ops.mesh_render_raw(floor["verts"], floor["faces"], floor["counts"], floor["attr"], cams,
                                                     size, "perspective", "min", near=NEAR, perspective_correct=True)
    return floor["pictures"][key]


def pyramids(ops, floor, ht, wt):
    """(the device's pyramid, levels, the restatement's) of the procedural ht x wt texture, made once."""
    if (ht, wt) not in floor["pyramids"]:
        tex = procedural(ht, wt)
        pyr, levels = ops.texture_mips(torch.from_numpy(tex).to(DEV))
        floor["pyramids"][(ht, wt)] = (pyr, levels, ref.pyramid(tex))
    return floor["pyramids"][(ht, wt)]


def same(got, want):
    got = host(got) if torch.is_tensor(got) else got
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(
        bits(got) if got.dtype == np.float32 else got, bits(want) if want.dtype == np.float32 else want)


@pytest.mark.parametrize("ht,wt", SIZES)
def test_texture_mips(ops, ht, wt):
    tex = np.random.RandomState(ht * 100 + wt).standard_normal((ht, wt, 3)).astype(F)
    dev = torch.from_numpy(tex).to(DEV)
    full = ref.max_levels(ht, wt)
    pyr, levels = ops.texture_mips(dev)
    assert levels == full and same(pyr, ref.pyramid(tex))
    assert same(pyr[:3 * ht * wt], tex.reshape(-1))
    for fewer in range(1, full):
        out = torch.full((ref.pyramid_floats(ht, wt, fewer) + 5,), -7.0, device=DEV)
        got, n = ops.texture_mips(dev, fewer, out=out[:-5])
        assert n == fewer and same(got, ref.pyramid(tex, fewer)) and (out[-5:] == -7).all()


@pytest.mark.parametrize("wrap", ["repeat", "clamp"])
@pytest.mark.parametrize("ht,wt", TEXTURES, ids=lambda v: str(v))
@pytest.mark.parametrize("size", PICTURES, ids=lambda s: "%dx%d" % s)
def test_picture_texture_against_the_restatement(ops, floor, size, ht, wt, wrap):
    uv, _, face = uv_picture(ops, floor, size)
    pyr, levels, pyr_ref = pyramids(ops, floor, ht, wt)
    huv, hface = host(uv), host(face)
    want, level = ref.texture(huv, hface, pyr_ref, ht, wt, levels, WRAPS[wrap], background=BG, return_level=True)
    cov = ref.covered(huv, hface)
    # the pictures show what they are meant to: both views covered, the NaN triangle inside, the uv range, the levels
    assert all(cov[v].sum() > 60 for v in range(2)) and ((hface >= 0) & ~cov).sum() >= 3
    assert huv[cov][:, :2].min() < -1.0 and huv[cov][:, :2].max() > 2.0
    assert len(np.unique(level[cov])) >= (3 if (ht, wt) == (64, 64) else 2)
    got = ops.picture_texture_batch([uv], [face], pyr, (ht, wt), levels, wrap, background=BG)[0]
    assert tuple(got.shape) == (2,) + size + (3,) and same(got, want)
    # the paint, and a caller's buffer
    out = torch.full((1, 2) + size + (3,), -9.0, device=DEV)
    got = ops.picture_texture_batch([uv], [face], pyr, (ht, wt), levels, wrap, 2.0, -0.5, 0.0, 1.0, BG, out=out)[0]
    assert got.data_ptr() == out.data_ptr()
    assert same(got, ref.texture(huv, hface, pyr_ref, ht, wt, levels, WRAPS[wrap], 2.0, -0.5, 0.0, 1.0, BG))


def test_the_seam_keeps_the_fine_level(ops, floor):
    """Across x = 0 the uv jump by half a texture width: a step of 32 texels would choose level 5 (32^2 > 2^9).  The
    pixels on either side of the seam take the level of their continuous side, and the device agrees."""
    size = (64, 64)
    uv, _, face = uv_picture(ops, floor, size, CAMS[:1])
    huv, hface = host(uv), host(face)
    _, level = ref.select_level(huv, hface, 64, 64, 7)
    first, second = (hface[0] == 0) | (hface[0] == 1), (hface[0] == 2) | (hface[0] == 3)
    edge = (first[:-1] & second[1:]) | (second[:-1] & first[1:])  # (i, j) and (i + 1, j) lie across the seam
    assert edge.sum() > 10
    s, t = huv[0, :, :, 0] * F(64), huv[0, :, :, 1] * F(64)
    across = (s[1:] - s[:-1]) ** 2 + (t[1:] - t[:-1]) ** 2
    assert (across[edge] > 2 ** 9).all()
    assert level[0][:-1][edge].max() < 5 and level[0][1:][edge].max() < 5
    pyr, levels, pyr_ref = pyramids(ops, floor, 64, 64)
    got = ops.picture_texture_batch([uv], [face], pyr, (64, 64), levels, "repeat", background=BG)[0]
    assert same(got, ref.texture(huv, hface, pyr_ref, 64, 64, levels, background=BG))


def test_batched_equals_per_frame(ops, floor):
    size, (ht, wt) = PICTURES[0], TEXTURES[1]
    pyr, levels, _ = pyramids(ops, floor, ht, wt)
    cams = [CAMS, CAMS.flip(0).clone(), torch.stack([tilted(0.3), tilted(1.2, t=(0, 0.3, 2.0))])]
    raws = ops.mesh_render_raw_batch([floor["verts"]] * 3, [floor["faces"]] * 3, [floor["counts"]] * 3,
                                     [floor["attr"]] * 3, cams, size, "perspective", "min", near=NEAR,
                                     perspective_correct=True)
    uvs, faces = [r[0] for r in raws], [r[2] for r in raws]
    batch = ops.picture_texture_batch(uvs, faces, pyr, (ht, wt), levels, "repeat", background=BG)
    assert not torch.equal(batch[0], batch[2])
    ctx = ops.get_context(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    for f in range(3):
        one = ops.picture_texture_batch([uvs[f]], [faces[f]], pyr, (ht, wt), levels, "repeat", background=BG)[0]
        assert same(one, host(batch[f]))
        direct = torch.empty_like(one)  # the per-frame entry point itself
        rc = ctx.lib.mp_picture_texture(ctx.handle, uvs[f].data_ptr(), faces[f].data_ptr(), 2, size[0], size[1],
                                        pyr.data_ptr(), ht, wt, levels, 0, 1.0, 0.0, -math.inf, math.inf, BG,
                                        direct.data_ptr(), stream)
        assert rc == OK and same(direct, host(batch[f]))
    # the composite, batched against per frame, in place
    fronts = [(batch[f], raws[f][1], faces[f]) for f in range(3)]
    backs = [fronts[1], fronts[2], fronts[0]]
    many = ops.picture_composite_batch(fronts, backs, "depth", "min", BG)
    for f in range(3):
        one = ops.picture_composite_batch([fronts[f]], [backs[f]], "depth", "min", BG)[0]
        want = ref.composite([host(t) for t in fronts[f]], [host(t) for t in backs[f]], ref.DEPTH, ref.MIN_Z, BG)
        for a, b, c in zip(many[f], one, want):
            assert same(a, host(b)) and same(a, c)
        image, depth = torch.empty_like(batch[f]), torch.empty_like(raws[f][1])
        mask = torch.empty(faces[f].shape, dtype=torch.uint8, device=DEV)
        rc = ctx.lib.mp_picture_composite(ctx.handle, *[t.data_ptr() for t in fronts[f] + backs[f]], faces[f].numel(),
                                          1, 1, BG, image.data_ptr(), depth.data_ptr(), mask.data_ptr(), stream)
        assert rc == OK and all(same(a, c) for a, c in zip((image, depth, mask), want))


@pytest.fixture(scope="module")
def sphere(recon):
    return recon.reconstruct_mesh(torch.from_numpy(syn.sphere_volume(17)).to(DEV), normals="accumulate")


def scene_of(recon, y=-0.1, tex=(64, 64), **kw):
    verts, faces, uv = floor_mesh(y, nan_uv=False)
    return recon.Scene(verts, faces, uv, procedural(*tex), device=DEV, **kw)


def test_scene_uploads_what_it_is_given(recon, ops):
    tex8 = (procedural(5, 3) * 255).astype(np.uint8)
    a = scene_of(recon)
    b = recon.Scene(a.verts, a.faces, floor_mesh(nan_uv=False)[2], torch.from_numpy(tex8), wrap="clamp", flip_v=False,
                    levels=2, device=DEV)
    assert same(a.texture, procedural(64, 64)[::-1]) and same(b.texture, tex8.astype(F) / F(255))
    assert a.levels == 7 and same(a.pyramid, ref.pyramid(procedural(64, 64)[::-1]))
    assert b.levels == 2 and b.wrap == "clamp" and b.pyramid.numel() == ref.pyramid_floats(5, 3, 2)
    assert a.counts.tolist() == [10, 4] and a.attr.shape == (10, 3) and (a.attr[:, 2] == 0).all()


def test_composite_of_a_sphere_standing_in_a_floor(recon, ops, sphere):
    size = (40, 33)
    scene = scene_of(recon)
    kw = dict(projection="perspective", nearest="min", near=NEAR, perspective_correct=True, background=BG)
    front = recon.render_mesh(sphere, CAMS, size, "normals", **kw)
    back = recon.render_scene(scene, CAMS, size, **kw)
    assert isinstance(back, recon.MeshRender) and tuple(back.image.shape) == (2,) + size + (3,)
    # the scene's picture is the restatement's of its UV picture
    uv = ops.mesh_render_raw(scene.verts, scene.faces, scene.counts, scene.attr, CAMS, size, "perspective", "min",
                             near=NEAR, perspective_correct=True)
    assert same(back.image, ref.texture(host(uv[0]), host(uv[2]), host(scene.pyramid), 64, 64, 7, background=BG))
    assert same(back.depth, host(uv[1])) and same(back.face, host(uv[2]))
    hf, hb = [host(t) for t in front], [host(t) for t in back]
    got = {}
    for mode, code in (("depth", ref.DEPTH), ("over", ref.OVER)):
        pic = recon.composite(front, back, mode, "min", BG)
        want = ref.composite(hf, hb, code, ref.MIN_Z, BG)
        assert isinstance(pic, recon.ScenePicture) and pic.face is front.face
        assert same(pic.image, want[0]) and same(pic.depth, want[1]) and same(pic.mask, want[2])
        assert np.bincount(host(pic.mask).reshape(-1), minlength=3).tolist() == np.bincount(
            want[2].reshape(-1), minlength=3).tolist()
        assert all((want[2] == k).sum() > 20 for k in range(3))
        got[mode] = pic
        # in place: the outputs are the front's own buffers
        own = [t.clone() for t in front]
        mask = torch.empty(size=own[2].shape, dtype=torch.uint8, device=DEV)
        ops.picture_composite_batch([tuple(own)], [tuple(back)], mode, "min", BG, out=([own[0]], [own[1]], [mask]))
        assert same(own[0], want[0]) and same(own[1], want[1]) and same(mask, want[2]) and same(own[2], hf[2])
    # the floor in front of the sphere's lower half hides it by depth and not by coverage
    assert not torch.equal(got["depth"].mask, got["over"].mask)
    assert not torch.equal(got["depth"].image, got["over"].image)
    hidden = (got["over"].mask == 2) & (got["depth"].mask == 1)
    assert hidden.sum() > 20 and (got["over"].mask[got["depth"].mask == 2] == 2).all()
    # image and depth alone (no mask), and the one-camera form
    only = ops.picture_composite_batch([tuple(front)], [tuple(back)], "depth", "min", BG,
                                       out=([torch.empty_like(front.image)], None, None))[0]
    assert only[1] is None and only[2] is None and torch.equal(only[0], got["depth"].image)
    single = recon.render_mesh_many_in_scene([sphere, None], scene, CAMS[1], size, "normals", composite="depth", **kw)
    assert tuple(single[0].mask.shape) == size and torch.equal(single[0].image, got["depth"].image[1])
    assert single[1].mask.max() == 1 and torch.equal(single[1].image, back.image[1]) and (single[1].face == -1).all()


def test_both_nearest_conventions_with_an_orthogonal_camera(recon, sphere):
    """The viewer at +z ("max") and the same scene with z negated, depth a distance ("min"): one picture."""
    size = (33, 40)
    scene = scene_of(recon)
    cam = tilted(0.6, focal=0.6, t=(0.0, 0.0, 0.0), orthogonal=True)
    flipped = cam.clone()
    flipped[2] = -flipped[2]
    pics = {}
    for nearest, code, c in (("max", ref.MAX_Z, flipped), ("min", ref.MIN_Z, cam)):
        front = recon.render_mesh(sphere, c, size, "normals", "orthogonal", nearest, BG)
        back = recon.render_scene(scene, c, size, "orthogonal", nearest, background=BG)
        assert tuple(back.image.shape) == size + (3,)
        want = ref.composite([host(t) for t in front], [host(t) for t in back], ref.DEPTH, code, BG)
        pic = recon.composite(front, back, "depth", nearest, BG)
        assert same(pic.image, want[0]) and same(pic.depth, want[1]) and same(pic.mask, want[2])
        assert all((want[2] == k).sum() > 20 for k in (1, 2))
        over = recon.composite(front, back, "over", nearest, BG)
        assert not torch.equal(over.mask, pic.mask)
        pics[nearest] = pic
    assert torch.equal(pics["max"].mask, pics["min"].mask) and torch.equal(pics["max"].image, pics["min"].image)
    assert torch.equal(pics["max"].depth, -pics["min"].depth)


def carpet():
    """vert_data [3F,3], uv_data [3F,2] of tests/golden/scene_carpet.obj, laid out and placed as the reference's floor
    loader does: y and z exchanged, 150 units -> 3 m, centred, the floor at y = -0.9."""
    v, vt, fv, ft = [], [], [], []
    for line in open(os.path.join(os.path.dirname(__file__), "golden", "scene_carpet.obj")):
        word = line.split()
        if not word:
            continue
        if word[0] == "v":
            v.append([float(x) for x in word[1:4]])
        elif word[0] == "vt":
            vt.append([float(x) for x in word[1:3]])
        elif word[0] == "f":
            corners = [w.split("/") for w in word[1:4]]
            fv.append([int(c[0]) - 1 for c in corners])
            ft.append([int(c[1]) - 1 for c in corners])
    v, vt = np.array(v, np.float64)[:, [0, 2, 1]], np.array(vt, np.float64)
    v = v / 150 * 3.0
    v = v - v.mean(0) + np.array([0, -0.9, 0])
    return v[np.array(fv).reshape(-1)].astype(F), vt[np.array(ft).reshape(-1)].astype(F)


def test_from_packed_on_the_carpet_floor(recon, ops):
    vert_data, uv_data = carpet()
    assert vert_data.shape == (34 * 3, 3) and uv_data.shape == (34 * 3, 2)
    tex = procedural(64, 64)
    scene = recon.Scene.from_packed(vert_data, uv_data, tex, device=DEV)
    assert scene.faces.cpu().tolist() == np.arange(102).reshape(34, 3).tolist() and scene.counts.tolist() == [102, 34]
    cam = tilted(-0.7, focal=4.5, t=(0.0, 3.1, 3.0))  # the carpet is 1.04 m wide: it fills the middle of the picture
    size = (48, 40)
    pic = recon.render_scene(scene, cam, size, "perspective", "min", near=0.5, perspective_correct=True, background=-1.0)
    uv = ops.mesh_render_raw(scene.verts, scene.faces, scene.counts, scene.attr, cam, size, "perspective", "min",
                             near=0.5, perspective_correct=True)
    huv, hface = host(uv[0]), host(uv[2])
    want = ref.texture(huv, hface, ref.pyramid(tex[::-1]), 64, 64, 7, background=-1.0)
    assert same(pic.image, want[0]) and same(pic.face, hface[0])
    cov = hface[0] >= 0
    assert cov.sum() > 200 and np.array_equal(ref.covered(huv, hface)[0], cov)
    assert (host(pic.image)[cov] >= 0.05).all() and (host(pic.image)[~cov] == -1.0).all()


def test_frame_slot_with_a_scene(recon, nets):  # noqa: F811
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, check_pictures, frames, make_slot
    images, calibs = frames()
    scene = scene_of(recon, y=-0.4)
    opts = dict(SLOT_PICTURES, shade="normals")
    mesh = {"normals": "accumulate", "colors": False}
    slot = make_slot(nets, mesh, dict(opts, scene=scene), netc=False)
    plain = make_slot(nets, mesh, opts, netc=False)
    try:
        assert slot.picture_options.scene is scene and slot.picture_options.composite == "depth"
        assert tuple(slot.pictures_mask.shape) == (2, 2) + SIZE and slot.pictures_mask.dtype == torch.uint8
        assert plain.pictures_mask is None and not hasattr(plain, "scene_uv")
        slot.submit(images, calibs, cameras=TWO)
        slot.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        meshes, pics = slot.meshes(), slot.pictures()
        assert meshes[1] is None and all(isinstance(p, recon.ScenePicture) for p in pics)
        po = slot.picture_options
        want = recon.render_mesh_many_in_scene(meshes, scene, TWO, SIZE, "normals", po.projection, po.nearest,
                                               po.background, po.near, po.perspective_correct, "depth")
        for b in range(2):
            for a, c in zip(pics[b], want[b]):
                assert a.dtype == c.dtype and torch.equal(a.view(torch.uint8), c.contiguous().view(torch.uint8)), b
        assert pics[0].image.data_ptr() == slot.pictures_image[0].data_ptr()
        counts = torch.bincount(pics[0].mask.reshape(-1).long(), minlength=3).tolist()
        assert all(c > 20 for c in counts), counts
        # the empty frame: the bare scene
        bare = recon.render_scene(scene, TWO, SIZE, po.projection, po.nearest, po.near, po.perspective_correct,
                                  po.background)
        assert int(pics[1].mask.max()) == 1 and (pics[1].face == -1).all()
        assert torch.equal(pics[1].image, bare.image) and torch.equal(pics[1].depth, bare.depth)
        assert torch.equal(pics[1].mask.bool(), bare.face >= 0)
        # "over" in a second slot option set differs where the floor hides the body
        over = recon.render_mesh_many_in_scene(meshes[:1], scene, TWO, SIZE, "normals", po.projection, po.nearest,
                                               po.background, po.near, po.perspective_correct, "over")[0]
        assert not torch.equal(over.mask, pics[0].mask)
        # without a scene: MeshRenders, the bits of recon.render_mesh as before
        plain.submit(images, calibs, cameras=TWO)
        before = check_pictures(plain, TWO, what="no scene")
        assert isinstance(before[0], recon.MeshRender) and before[1] is None
        assert torch.equal(before[0].face, pics[0].face)
        # a frame whose mesh overflowed the slot's capacities: the re-run mesh, rendered again and composited over the
        # slot's own picture of the scene, into fresh tensors -- the bits of the full-capacity submission
        first = [t.clone() for t in pics[0]]
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
            slot._render_pictures(2)
        slot._busy = True
        again = slot.pictures()
        assert slot._reran == [0] and int(again[1].mask.max()) == 1
        for a, c, own in zip(again[0], first, (slot.pictures_image, slot.pictures_depth, slot.pictures_face,
                                               slot.pictures_mask)):
            assert torch.equal(a.view(torch.uint8), c.view(torch.uint8)) and a.data_ptr() != own[0].data_ptr()
        assert not torch.equal(slot.pictures_mask[0], first[3])  # the slot's own buffers: 200 faces of the body
    finally:
        slot.close()
        plain.close()


def test_frame_slot_scene_behind_netc_pictures(recon, nets):  # noqa: F811
    """shade="netC" is untouched by the scene: the composite (here "over") runs behind its paint, so the slot's picture
    is the composite of the scene-less slot's picture with the scene's."""
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, frames, make_slot
    images, calibs = frames()
    scene = scene_of(recon, y=-0.4, wrap="clamp")
    opts = dict(SLOT_PICTURES, shade="netC")
    mesh = {"normals": None, "colors": False}
    slot = make_slot(nets, mesh, dict(opts, scene=scene, composite="over"))
    plain = make_slot(nets, mesh, opts)
    try:
        for s in (slot, plain):
            s.submit(images, calibs, cameras=TWO)
        pics, base = slot.pictures(), plain.pictures()
        po = slot.picture_options
        assert po.composite == "over" and base[1] is None and isinstance(base[0], recon.MeshRender)
        back = recon.render_scene(scene, TWO, SIZE, po.projection, po.nearest, po.near, po.perspective_correct,
                                  po.background)
        want = recon.composite(base[0], back, "over", po.nearest, po.background)
        for a, c in zip(pics[0], want):
            assert torch.equal(a.view(torch.uint8), c.contiguous().view(torch.uint8))
        assert torch.equal(pics[0].mask == 2, base[0].face >= 0)  # "over": the subject wherever it is covered
        assert torch.equal(pics[1].image, back.image) and int(pics[1].mask.max()) == 1
    finally:
        slot.close()
        plain.close()


class Env:
    """Well-formed calls of the new entry points on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
        self.nv, self.h, self.w, self.ht, self.wt, self.levels = 2, 3, 4, 5, 3, 3
        n = self.nv * self.h * self.w
        self.tex, self.pyr = z(5, 3, 3), z(ref.pyramid_floats(5, 3, 3))
        self.uv, self.image, self.back = z(n, 3), z(n, 3), z(n, 3)
        self.depth, self.back_depth = z(n), z(n)
        self.face, self.back_face = z(n, dtype=torch.int32), z(n, dtype=torch.int32)
        self.mask = z(n, dtype=torch.uint8)
        self.n = n
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def done(self, rc):
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()

    def mips(self, **k):
        a = dict(tex=self.tex.data_ptr(), ht=self.ht, wt=self.wt, levels=self.levels, pyr=self.pyr.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_texture_mips(self.ctx.handle, a["tex"], a["ht"], a["wt"], a["levels"], a["pyr"],
                                                  self.stream))

    def texture(self, **k):
        a = dict(uv=self.uv.data_ptr(), face=self.face.data_ptr(), nv=self.nv, h=self.h, w=self.w,
                 pyr=self.pyr.data_ptr(), ht=self.ht, wt=self.wt, levels=self.levels, wrap=0, image=self.image.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_texture(
            self.ctx.handle, a["uv"], a["face"], a["nv"], a["h"], a["w"], a["pyr"], a["ht"], a["wt"], a["levels"],
            a["wrap"], 1.0, 0.0, -math.inf, math.inf, 1.0, a["image"], self.stream))

    def composite(self, **k):
        a = dict(fi=self.uv.data_ptr(), fd=self.depth.data_ptr(), ff=self.face.data_ptr(), bi=self.back.data_ptr(),
                 bd=self.back_depth.data_ptr(), bf=self.back_face.data_ptr(), n=self.n, mode=1, nearest=0,
                 image=self.image.data_ptr(), depth=self.depth.data_ptr(), mask=self.mask.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_composite(
            self.ctx.handle, a["fi"], a["fd"], a["ff"], a["bi"], a["bd"], a["bf"], a["n"], a["mode"], a["nearest"], 1.0,
            a["image"], a["depth"], a["mask"], self.stream))


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    for call in (env.mips, env.texture, env.composite):
        assert call()[0] == OK
    assert env.composite(depth=None, mask=None)[0] == OK and env.composite(mode=0, nearest=1)[0] == OK
    torch.cuda.synchronize()
    assert (env.image == 0).all() and (env.mask == 2).all()  # face ids 0: all covered, uv 0 of a zero texture
    refused = [
        (env.texture, "mp_picture_texture", dict(image=env.uv.data_ptr()), "aliases"),
        (env.texture, "mp_picture_texture", dict(levels=4), "levels"),
        (env.texture, "mp_picture_texture", dict(levels=0), "levels"),
        (env.texture, "mp_picture_texture", dict(ht=0), "texture size"),
        (env.texture, "mp_picture_texture", dict(wt=8193), "texture size"),
        (env.texture, "mp_picture_texture", dict(wrap=2), "wrap"),
        (env.texture, "mp_picture_texture", dict(wrap=-1), "wrap"),
        (env.texture, "mp_picture_texture", dict(h=0), "image size"),
        (env.texture, "mp_picture_texture", dict(nv=0), "n_views"),
        (env.texture, "mp_picture_texture", dict(uv=None), "null"),
        (env.texture, "mp_picture_texture", dict(image=env.image.data_ptr() + 1), "misaligned"),
        (env.texture, "mp_picture_texture", dict(pyr=None), "bad argument"),
        (env.mips, "mp_texture_mips", dict(levels=4), "levels"),
        (env.mips, "mp_texture_mips", dict(ht=0), "texture size"),
        (env.mips, "mp_texture_mips", dict(tex=None), "bad argument"),
        (env.mips, "mp_texture_mips", dict(pyr=env.tex.data_ptr()), "aliases"),
        (env.composite, "mp_picture_composite", dict(mode=2), "mode"),
        (env.composite, "mp_picture_composite", dict(nearest=2), "nearest"),
        (env.composite, "mp_picture_composite", dict(fi=None), "null"),
        (env.composite, "mp_picture_composite", dict(image=None), "null"),
        (env.composite, "mp_picture_composite", dict(n=0), "n_pixels"),
        (env.composite, "mp_picture_composite", dict(fd=env.depth.data_ptr() + 2), "misaligned"),
        (env.composite, "mp_picture_composite", dict(image=env.uv.data_ptr() + 12), "aliases"),
        (env.composite, "mp_picture_composite", dict(depth=env.back_face.data_ptr()), "aliases"),
    ]
    env.image.fill_(5.0)
    for call, name, changed, word in refused:
        rc, msg = call(**changed)
        assert rc == ARG and msg.startswith(name + ":") and word in msg, (name, changed, msg)
    torch.cuda.synchronize()
    assert (env.image == 5.0).all()  # a refused call launches nothing
    # the batched forms carry their own names and refuse a frame count out of range
    ptr = (ctypes.c_void_p * 1)(env.uv.data_ptr())
    rc = env.lib.mp_picture_texture_batch(env.ctx.handle, 33, ptr, ptr, 2, 3, 4, env.pyr.data_ptr(), 5, 3, 3, 0, 1.0,
                                          0.0, 0.0, 1.0, 1.0, ptr, env.stream)
    assert env.done(rc)[0] == ARG and env.done(rc)[1].startswith("mp_picture_texture_batch:")
    rc = env.lib.mp_picture_composite_batch(env.ctx.handle, 0, ptr, ptr, ptr, ptr, ptr, ptr, 24, 1, 0, 1.0, ptr, ptr,
                                            ptr, env.stream)
    assert env.done(rc)[0] == ARG and env.done(rc)[1].startswith("mp_picture_composite_batch:")
