"""mp_picture_shadow / mp_picture_shadow_batch (csrc/scene.hip), ops.picture_shadow_batch, recon.Light / shadow_map /
shade_shadow, the lit Scene in render_scene / render_mesh_many_in_scene and in a FrameSlot, on the GPU: every comparison
is array_equal on the bits against the numpy restatement (tests/shadow_ref.py, with tests/scene_ref.py for the texture
and the composite).  The rasteriser's pictures that the restatements start from are the device's own: it has its
bit-for-bit tests in test_mesh_render_gpu.py / test_mesh_render_clip_gpu.py.  Needs an MI355X."""
import ctypes
import math

import numpy as np
import pytest

import scene_ref
import shadow_cases as cases
import shadow_ref as ref
from test_mesh_batch_gpu import nets  # noqa: F401  (the fixture)
from test_mesh_render_gpu import ARG, DEV, OK, UNSUPPORTED, bits, host
from test_scene_gpu import procedural

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
BG = 0.25
PICTURES = [(33, 20), (20, 48)]
MAPS = [(1, 1), (2, 2), (5, 3), (64, 64)]
NEAREST = {"min": ref.MIN_Z, "max": ref.MAX_Z}
PROJECTION = {"orthogonal": ref.ORTHOGONAL, "perspective": ref.PERSPECTIVE}
LIGHT = np.array([[0.9, 0.1, 0.0, 0.05], [-0.1, 0.9, 0.05, 0.0], [0.0, 0.05, 1.0, 0.2]], F)


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want):
    got = host(got) if torch.is_tensor(got) else got
    want = host(want) if torch.is_tensor(want) else want
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return np.array_equal(bits(got), bits(want)) if got.dtype == F else np.array_equal(got, want)


def synthetic(size, map_size, seed=0):
    """Two views of a position picture with uncovered spans longer than a wavefront, NaN / inf positions, points beside
    the map and behind a perspective light; a map with holes, a NaN and ties."""
    rng = np.random.RandomState(seed)
    h, w = size
    position = rng.uniform(-1.3, 1.3, (2, h, w, 3)).astype(F)
    position[..., 2] = rng.uniform(0.3, 1.6, (2, h, w))
    flat = position.reshape(-1, 3)
    flat[5] = [np.nan, 0.0, 1.0]
    flat[6] = [0.0, np.inf, 1.0]
    flat[7] = [0.0, 0.0, -np.inf]
    flat[8] = [3e7, 0.0, 1.0]
    flat[9:40, 2] = -flat[9:40, 2]   # behind a perspective light
    flat[40] = [0.0, 0.0, -0.2]      # z == 0 under LIGHT: in the light's plane
    face = rng.randint(0, 50, (2, h, w)).astype(np.int32)
    face.reshape(-1)[100:300] = -1
    face.reshape(-1)[h * w + 17:h * w + 17 + 130] = -1
    face[rng.rand(2, h, w) < 0.1] = -1
    image = rng.standard_normal((2, h, w, 3)).astype(F)
    image.reshape(-1, 3)[3] = [np.nan, -0.0, np.inf]
    hs, ws = map_size
    map_depth = rng.uniform(0.3, 1.6, (hs, ws)).astype(F)
    map_face = np.where(rng.rand(hs, ws) < 0.7, 4, -1).astype(np.int32)
    map_face[0, 0] = 4  # a 1 x 1 map is covered
    if hs * ws > 4:
        map_depth[hs // 2, ws // 2] = np.nan
        map_depth[0, :] = F(0.9)
    position.reshape(-1, 3)[41:60, 2] = F(0.9) - F(0.2) - position.reshape(-1, 3)[41:60, 1] * F(0.05)  # near ties
    return image, position, face, map_depth, map_face


@pytest.mark.parametrize("map_size", MAPS, ids=lambda s: "map%dx%d" % s)
@pytest.mark.parametrize("size", PICTURES, ids=lambda s: "%dx%d" % s)
def test_kernel_against_the_restatement(ops, size, map_size):
    image, position, face, map_depth, map_face = synthetic(size, map_size)
    d = [dev(a) for a in (image, position, face, map_depth, map_face)]
    shaded = 0
    for radius in range(4):
        for nearest in ("min", "max"):
            for projection in ("orthogonal", "perspective"):
                for bias in (0.0, 0.125):
                    kw = dict(projection=projection, nearest=nearest, bias=bias, radius=radius, strength=0.6)
                    want_image, want_shade = ref.shadow(image, position, face, map_depth, map_face, LIGHT,
                                                        PROJECTION[projection], NEAREST[nearest], bias, radius, 0.6)
                    shaded += int((want_shade > 0).sum())
                    what = (radius, nearest, projection, bias)
                    got = ops.picture_shadow_batch([d[0]], [d[1]], [d[2]], [d[3]], [d[4]], LIGHT, with_shade=True, **kw)[0]
                    assert same(got[0], want_image) and same(got[1], want_shade), what
                    if bias:
                        continue
                    own = d[0].clone()  # in place
                    got = ops.picture_shadow_batch([own], [d[1]], [d[2]], [d[3]], [d[4]], LIGHT, out=([own], None), **kw)[0]
                    assert got[0] is own and got[1] is None and same(own, want_image), what
                    got = ops.picture_shadow_batch(None, [d[1]], [d[2]], [d[3]], [d[4]], LIGHT, **kw)[0]  # the shade alone
                    assert got[0] is None and same(got[1], want_shade), what
                    got = ops.picture_shadow_batch([d[0]], [d[1]], [d[2]], [d[3]], [d[4]], LIGHT, **kw)[0]  # the image alone
                    assert got[1] is None and same(got[0], want_image), what
    assert shaded > 0
    assert same(d[0], image)  # out of place: the input is not written


def test_strength_zero_and_an_uncovered_map_leave_the_bits(ops):
    image, position, face, map_depth, map_face = synthetic((33, 20), (5, 3))
    d = [dev(a) for a in (image, position, face, map_depth, map_face)]
    got = ops.picture_shadow_batch([d[0]], [d[1]], [d[2]], [d[3]], [d[4]], LIGHT, strength=0.0, with_shade=True)[0]
    assert same(got[0], image) and (got[1] > 0).any()
    none = torch.full_like(d[4], -1)
    got = ops.picture_shadow_batch([d[0]], [d[1]], [d[2]], [d[3]], [none], LIGHT, with_shade=True)[0]
    assert same(got[0], image) and same(got[1], np.zeros(face.shape, F))


def test_batched_equals_per_frame(ops):
    """Three frames, one with an all-uncovered map, in one launch against mp_picture_shadow on each."""
    size, map_size = (20, 48), (5, 3)
    frames = [synthetic(size, map_size, seed) for seed in (1, 2, 3)]
    frames[1] = frames[1][:4] + (np.full(map_size, -1, np.int32),)
    cals = [LIGHT, LIGHT * F(0.8), LIGHT[[1, 0, 2]].copy()]
    d = [[dev(a) for a in fr] for fr in frames]
    kw = dict(projection="perspective", nearest="min", bias=0.0, radius=2, strength=0.5)
    got = ops.picture_shadow_batch([f[0] for f in d], [f[1] for f in d], [f[2] for f in d], [f[3] for f in d],
                                   [f[4] for f in d], cals, with_shade=True, **kw)
    ctx = ops.get_context(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    n = frames[0][2].size
    for f in range(3):
        want = ref.shadow(*frames[f], cals[f], ref.PERSPECTIVE, ref.MIN_Z, 0.0, 2, 0.5)
        assert same(got[f][0], want[0]) and same(got[f][1], want[1]), f
        image, shade = torch.empty_like(d[f][0]), torch.empty(frames[f][2].shape, device=DEV)
        cal = np.ascontiguousarray(cals[f], F)
        rc = ctx.lib.mp_picture_shadow(ctx.handle, d[f][0].data_ptr(), d[f][1].data_ptr(), d[f][2].data_ptr(), n,
                                       d[f][3].data_ptr(), d[f][4].data_ptr(), map_size[0], map_size[1],
                                       cal.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1, 1, 0.0, 2, 0.5,
                                       image.data_ptr(), shade.data_ptr(), stream)
        assert rc == OK and same(image, got[f][0]) and same(shade, got[f][1]), f
    assert same(got[1][0], frames[1][0]) and not (got[1][1] != 0).any()
    assert (got[0][1] > 0).any() and (got[2][1] > 0).any()


# ---- the whole path with the real rasteriser: the geometry test's sphere over a floor ----------------------------------
NEAR = 3.4  # cuts the sphere's near cap: the subject's picture is the clipped one


def camera():
    """A perspective camera above the floor, tilted down at it: [4,4] float32."""
    a = -0.6
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    m[:3, :3] = np.diag([1.2, 1.2, 1.0]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    m[:3, 3] = [-0.3, 0.0, 4.0]
    return torch.from_numpy(m.astype(F))


@pytest.fixture(scope="module")
def world(recon):
    verts, faces = cases.sphere_mesh()
    mesh = recon.Mesh(dev(verts), dev(faces), None, dev((verts * F(0.4) + F(0.5)).astype(F)))
    fv, ff, uv = cases.plank(x=(-2.0, 3.0), z=(-1.5, 1.5))
    light = cases.light(recon, radius=1, strength=0.6)
    return dict(mesh=mesh, light=light,
                lit=recon.Scene(fv, ff, uv, procedural(64, 64), device=DEV, light=light),
                dark=recon.Scene(fv, ff, uv, procedural(64, 64), device=DEV))


@pytest.mark.parametrize("size", [(33, 20), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_lit_scene_against_the_composition_of_the_restatements(ops, recon, world, size):
    mesh, light, lit, dark = world["mesh"], world["light"], world["lit"], world["dark"]
    cam = camera()
    kw = dict(projection="perspective", nearest="min", near=NEAR, perspective_correct=True, background=BG)
    raster = dict(projection="perspective", nearest="min", near=NEAR, perspective_correct=True)
    got = recon.render_mesh_many_in_scene([mesh, None], lit, cam, size, "colors", **kw)
    plain = recon.render_mesh_many_in_scene([mesh, None], dark, cam, size, "colors", **kw)
    # the pieces: the subject, the scene's UV and position pictures, the shadow map
    front = recon.render_mesh(mesh, cam, size, "colors", **kw)
    uv = ops.mesh_render_raw(lit.verts, lit.faces, lit.counts, lit.attr, cam, size, background=BG, **raster)
    pos = ops.mesh_render_raw(lit.verts, lit.faces, lit.counts, lit.verts, cam, size, background=BG, **raster)
    assert torch.equal(uv[2], pos[2]) and same(uv[1], pos[1])  # the position pass sees the faces of the UV pass
    counts = torch.tensor([mesh.verts.shape[0], mesh.faces.shape[0]], dtype=torch.int32, device=DEV)
    smap = ops.mesh_render_raw(mesh.verts, mesh.faces, counts, None, light.calib, light.res, "orthogonal", "min")
    maps = recon.shadow_map([mesh, None], light)
    assert same(maps[0][0], host(smap[1])[0]) and same(maps[0][1], host(smap[2])[0])
    assert tuple(maps[1][0].shape) == light.res and not maps[1][0].any() and (maps[1][1] == -1).all()
    tex = scene_ref.texture(host(uv[0]), host(uv[2]), host(lit.pyramid), 64, 64, lit.levels, background=BG)
    want_lit, want_shade = ref.shadow(tex, host(pos[0]), host(uv[2]), host(smap[1])[0], host(smap[2])[0], light.calib,
                                      ref.ORTHOGONAL, ref.MIN_Z, light.bias, light.radius, light.strength)
    want = scene_ref.composite([host(t)[None] for t in front], (want_lit, host(uv[1]), host(uv[2])), scene_ref.DEPTH,
                               scene_ref.MIN_Z, BG)
    assert same(got[0].image, want[0][0]) and same(got[0].depth, want[1][0]) and same(got[0].mask, want[2][0])
    assert torch.equal(got[0].face, front.face)
    # the shadow: some floor pixel is darker, no pixel of the subject differs, nothing else changes
    floor, subject = host(got[0].mask) == 1, host(got[0].mask) == 2
    darker = (host(got[0].image) < host(plain[0].image)).any(-1)
    assert (darker & floor).sum() >= 5 and (want_shade[0][floor] == 1.0).any()
    assert not (bits(host(got[0].image)) != bits(host(plain[0].image)))[subject].any() and subject.sum() > 20
    assert torch.equal(got[0].mask, plain[0].mask) and torch.equal(got[0].depth, plain[0].depth)
    # no mesh: the bare scene, the bits of the light-less call
    for a, c in zip(got[1], plain[1]):
        assert torch.equal(a.view(torch.uint8), c.view(torch.uint8))
    assert same(got[1].image, tex[0])
    # the pieces through the public calls
    back = recon.render_scene(lit, cam, size, casters=mesh, **kw)
    assert same(back.image, want_lit[0]) and same(back.face, host(uv[2])[0])
    assert same(recon.render_scene(lit, cam, size, **kw).image, tex[0])
    bare = recon.render_scene(dark, cam, size, **kw)
    image, shade = recon.shade_shadow(bare, pos[0][0], maps[0], light)
    assert same(image, want_lit[0]) and same(shade, want_shade[0])
    # a second run gives the same bits
    again = recon.render_mesh_many_in_scene([mesh, None], lit, cam, size, "colors", **kw)
    for a, c in zip(again[0], got[0]):
        assert torch.equal(a.view(torch.uint8), c.view(torch.uint8))


# ---- the slot -------------------------------------------------------------------------------------------------------
def slot_scene(recon, light=True, **kw):
    from test_scene_gpu import floor_mesh
    verts, faces, uv = floor_mesh(-0.4, nan_uv=False)
    sun = recon.Light.directional((0.3, -1.0, 0.2), (-1.5, -1.0, -1.5), (1.5, 1.0, 1.5), res=(64, 48)) if light else None
    return recon.Scene(verts, faces, uv, procedural(64, 64), device=DEV, light=sun, **kw)


def equal_pictures(a, b):
    return all(x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
               for x, y in zip(a, b))


def test_frame_slot_with_a_lit_scene(recon, nets):  # noqa: F811
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, frames, make_slot
    images, calibs = frames()
    scene, unlit = slot_scene(recon), slot_scene(recon, light=False)
    opts = dict(SLOT_PICTURES, shade="normals")
    mesh = {"normals": "accumulate", "colors": False}
    slot = make_slot(nets, mesh, dict(opts, scene=scene), netc=False)
    plain = make_slot(nets, mesh, dict(opts, scene=unlit), netc=False)
    try:
        assert tuple(slot.shadow_depth.shape) == (2, 64, 48) and slot.shadow_face.dtype == torch.int32
        assert tuple(slot.scene_pos.shape) == tuple(slot.scene_lit.shape) == (2, 2) + SIZE + (3,)
        assert not any(hasattr(plain, k) for k in ("shadow_depth", "shadow_face", "scene_pos", "scene_lit"))
        for s in (slot, plain):
            s.submit(images, calibs, cameras=TWO)
            s.wait()
        meshes, pics = slot.meshes(), slot.pictures()
        assert meshes[1] is None and all(isinstance(p, recon.ScenePicture) for p in pics)
        po = slot.picture_options
        args = (TWO, SIZE, "normals", po.projection, po.nearest, po.background, po.near, po.perspective_correct, "depth")
        want = recon.render_mesh_many_in_scene(meshes, scene, *args)
        assert equal_pictures(pics[0], want[0]) and equal_pictures(pics[1], want[1])
        assert pics[0].image.data_ptr() == slot.pictures_image[0].data_ptr()
        # the shadow is there, on the floor only; scene_image stays unshadowed
        before = recon.render_mesh_many_in_scene(meshes, unlit, *args)
        changed = (pics[0].image != before[0].image).any(-1)
        assert changed.sum() >= 5 and (pics[0].mask[changed] == 1).all()
        assert (pics[0].image[changed] <= before[0].image[changed]).all()
        bare = recon.render_scene(unlit, TWO, SIZE, po.projection, po.nearest, po.near, po.perspective_correct,
                                  po.background)
        assert torch.equal(slot.scene_image[0], bare.image) and not torch.equal(slot.scene_lit[0], bare.image)
        # the empty frame: an uncovered map, the unshadowed bare scene
        assert (slot.shadow_face[1] == -1).all() and (slot.shadow_face[0] >= 0).any()
        assert torch.equal(pics[1].image, bare.image) and int(pics[1].mask.max()) == 1 and (pics[1].face == -1).all()
        # the same slot without a light: today's bits
        assert equal_pictures(plain.pictures()[0], before[0]) and equal_pictures(plain.pictures()[1], before[1])
        # a frame whose mesh overflowed the slot's capacities: rendered, shadowed and composited again, the same bits
        first = [t.clone() for t in pics[0]]
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
            slot._render_pictures(2)
        slot._busy = True
        again = slot.pictures()
        assert slot._reran == [0] and int(again[1].mask.max()) == 1
        assert equal_pictures(again[0], first) and again[0].image.data_ptr() != slot.pictures_image[0].data_ptr()
        assert not torch.equal(slot.pictures_image[0], first[0])  # the slot's own buffers: 200 faces of the body
    finally:
        slot.close()
        plain.close()


def test_frame_slot_lit_scene_behind_netc_pictures(recon, nets):  # noqa: F811
    """shade="netC": the slot's picture is the composite of the scene-less slot's picture over the lit scene."""
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, frames, make_slot
    images, calibs = frames()
    scene = slot_scene(recon, wrap="clamp")
    opts = dict(SLOT_PICTURES, shade="netC")
    mesh = {"normals": None, "colors": False}
    slot = make_slot(nets, mesh, dict(opts, scene=scene, composite="over"))
    plain = make_slot(nets, mesh, opts)
    try:
        for s in (slot, plain):
            s.submit(images, calibs, cameras=TWO)
        pics, base = slot.pictures(), plain.pictures()
        po = slot.picture_options
        kw = dict(projection=po.projection, nearest=po.nearest, near=po.near, perspective_correct=po.perspective_correct,
                  background=po.background)
        back = recon.render_scene(scene, TWO, SIZE, casters=slot.meshes()[0], **kw)
        bare = recon.render_scene(scene, TWO, SIZE, **kw)
        assert not torch.equal(back.image, bare.image)
        want = recon.composite(base[0], back, "over", po.nearest, po.background)
        assert equal_pictures(pics[0], want)
        assert torch.equal(pics[1].image, bare.image) and int(pics[1].mask.max()) == 1
    finally:
        slot.close()
        plain.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
class Env:
    """A well-formed call of mp_picture_shadow on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
        self.n, self.hs, self.ws = 24, 5, 3
        self.image, self.out, self.position, self.shade = z(24, 3), z(24, 3), z(24, 3), z(24)
        self.face, self.map_face = z(24, dtype=torch.int32), z(5, 3, dtype=torch.int32)
        self.map_depth = torch.full((5, 3), -1.0, device=DEV)
        self.cal = np.ascontiguousarray(np.eye(4, dtype=F)[:3])
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def done(self, rc):
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()

    def shadow(self, **k):
        a = dict(image=self.image.data_ptr(), position=self.position.data_ptr(), face=self.face.data_ptr(), n=self.n,
                 map_depth=self.map_depth.data_ptr(), map_face=self.map_face.data_ptr(), hs=self.hs, ws=self.ws,
                 cal=self.cal.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), projection=0, nearest=1, bias=0.0, radius=1,
                 strength=0.5, out=self.out.data_ptr(), shade=self.shade.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_shadow(
            self.ctx.handle, a["image"], a["position"], a["face"], a["n"], a["map_depth"], a["map_face"], a["hs"], a["ws"],
            a["cal"], a["projection"], a["nearest"], a["bias"], a["radius"], a["strength"], a["out"], a["shade"],
            self.stream))


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    env.image.fill_(2.0)
    assert env.shadow()[0] == OK
    assert env.shadow(out=env.image.data_ptr(), shade=None)[0] == OK  # in place
    assert env.shadow(image=None, out=None)[0] == OK                   # the shade alone
    torch.cuda.synchronize()
    assert (env.shade == 1.0).all() and (env.out == 1.0).all() and (env.image == 1.0).all()
    null_cal = ctypes.POINTER(ctypes.c_float)()
    refused = [
        (dict(n=0), ARG, "n_pixels"),
        (dict(n=0x7fffffff // 3 + 1), UNSUPPORTED, "2^31 / 3"),
        (dict(hs=0), ARG, "shadow map size"),
        (dict(ws=4097), ARG, "shadow map size"),
        (dict(projection=2), ARG, "projection"),
        (dict(nearest=-1), ARG, "nearest"),
        (dict(bias=-0.5), ARG, "bias"),
        (dict(bias=math.nan), ARG, "bias"),
        (dict(bias=math.inf), ARG, "bias"),
        (dict(radius=-1), ARG, "radius"),
        (dict(radius=4), ARG, "radius"),
        (dict(strength=-0.1), ARG, "strength"),
        (dict(strength=1.5), ARG, "strength"),
        (dict(strength=math.nan), ARG, "strength"),
        (dict(out=None, shade=None), ARG, "no output"),
        (dict(out=None), ARG, "go together"),
        (dict(image=None), ARG, "go together"),
        (dict(position=None), ARG, "null"),
        (dict(face=None), ARG, "null"),
        (dict(map_depth=None), ARG, "null"),
        (dict(map_face=None), ARG, "null"),
        (dict(cal=null_cal), ARG, "bad argument"),
        (dict(position=env.position.data_ptr() + 2), ARG, "misaligned"),
        (dict(shade=env.shade.data_ptr() + 1), ARG, "misaligned"),
        (dict(out=env.image.data_ptr() + 12), ARG, "aliases"),          # the image shifted by a pixel
        (dict(out=env.position.data_ptr()), ARG, "aliases"),
        (dict(shade=env.face.data_ptr()), ARG, "aliases"),
        (dict(shade=env.map_depth.data_ptr(), n=15), ARG, "aliases"),
        (dict(shade=env.image.data_ptr()), ARG, "aliases"),
        (dict(out=env.map_face.data_ptr(), n=5), ARG, "aliases"),
    ]
    for t in (env.out, env.shade, env.image):
        t.fill_(5.0)
    for changed, code, word in refused:
        rc, msg = env.shadow(**changed)
        assert rc == code and msg.startswith("mp_picture_shadow:") and word in msg, (changed, rc, msg)
    torch.cuda.synchronize()
    assert (env.out == 5.0).all() and (env.shade == 5.0).all() and (env.image == 5.0).all()  # nothing was launched
    # the batched form carries its own name and refuses a frame count out of range
    ptr = (ctypes.c_void_p * 1)(env.position.data_ptr())
    for n_frames in (0, 33):
        rc = env.lib.mp_picture_shadow_batch(env.ctx.handle, n_frames, ptr, ptr, ptr, 24, ptr, ptr, 5, 3,
                                             env.cal.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 0, 1, 0.0, 1, 0.5,
                                             ptr, ptr, env.stream)
        assert env.done(rc)[0] == ARG and env.done(rc)[1].startswith("mp_picture_shadow_batch:")


def test_the_python_layers_refuse_before_they_enqueue(ops, recon):
    image, position, face, map_depth, map_face = [dev(a) for a in synthetic((33, 20), (5, 3))]
    call = lambda **k: ops.picture_shadow_batch([image], [position], [face], [map_depth], [map_face], LIGHT, **k)  # noqa: E731
    for kw in (dict(radius=4), dict(bias=-1.0), dict(strength=2.0), dict(projection="fisheye"), dict(nearest="far"),
               dict(out=(None, None)), dict(out=([position], None))):
        with pytest.raises((ValueError, RuntimeError)):
            call(**kw)
    with pytest.raises(ValueError):
        ops.picture_shadow_batch([image], [position], [face], [map_depth], [map_face.float()], LIGHT)
    with pytest.raises(ValueError):
        recon.shadow_map([None], "sun")
