"""Anti-aliased pictures from the render calls on the GPU: recon.render_mesh / render_mesh_many / render_scene /
render_mesh_many_in_scene(samples=s) against the numpy restatement's resolve (tests/resolve_ref.py) of the same call at
s times the size -- every pass and the composite run there under the same record, and the resolve runs once at the end.
Every comparison is on the bits.  Needs an MI355X."""
import math

import numpy as np
import pytest

import resolve_ref as rr
from monoport_amd import synthetic as syn
from test_mesh_render_gpu import DEV, host
from test_render_netc_gpu import heads, mesh33, picture_cameras  # noqa: F401  (heads, mesh33: the fixtures)
from test_scene_gpu import carpet, procedural, tilted

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
RES = (24, 40)
BG = 0.25
NAMES = ("image", "depth", "face", "mask", "coverage")


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


@pytest.fixture(scope="module")
def mesh(recon):
    """The 33^3 sphere with normals, and colours that vary over it."""
    m = recon.reconstruct_mesh(torch.from_numpy(syn.sphere_volume(33)).to(DEV), normals="accumulate")
    assert m.normals is not None and m.verts.shape[0] > 500
    return m._replace(colors=(m.verts * 0.4 + 0.5).contiguous())


def turned():
    c = torch.eye(4)
    a = math.radians(35.0)
    c[0, 0], c[0, 2], c[2, 0], c[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    c[:3] *= 0.9
    c[0, 3] = 0.2
    return c


# two orthogonal cameras in one call; one perspective camera whose near plane cuts the sphere (z = 2.4 .. 3.6)
CAMERAS = {"orthogonal": dict(calibs=torch.stack([torch.eye(4), turned()]), projection="orthogonal", nearest="max"),
           "perspective": dict(calibs=torch.tensor([[2.0, 0, 0, 0.1], [0, 2.0, 0, 0], [0, 0, 1.0, 3.0], [0, 0, 0, 1.0]]),
                               projection="perspective", nearest="min", near=2.6, perspective_correct=True)}


def fine_res(s):
    return (RES[0] * s, RES[1] * s)


def same(got, want, what):
    """A ResolvedPicture against the restatement's five outputs."""
    for name, g, w in zip(NAMES, got, want):
        assert rr.same_bits(host(g), w), (what, name)


def resolved(picture, s, nearest):
    """The restatement's resolve of a MeshRender / ScenePicture rendered at s times the size."""
    image, depth, face = (host(t) for t in picture[:3])
    return rr.resolve(image, depth, face, host(picture[3]) if len(picture) > 3 else None, s, nearest)


def lighting_of(recon, **kw):
    rng = np.random.default_rng(3)
    sh = (rng.standard_normal((9, 3)) * 0.2).astype(F)
    sh[0] = 0.8
    return recon.Lighting(sh, direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), **kw)


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("camera", ["orthogonal", "perspective"])
def test_render_mesh(recon, mesh, camera, s):
    cam = CAMERAS[camera]
    nearest = cam["nearest"]
    cases = [("colors", None), ("normals", None), (None, None), ("colors", lighting_of(recon)),
             ("normals", lighting_of(recon, frame="camera", albedo=(0.8, 0.7, 0.6)))]
    for shade, lighting in cases:
        what = (camera, s, shade, lighting is not None)
        got = recon.render_mesh(mesh, res=RES, shade=shade, background=BG, lighting=lighting, samples=s, **cam)
        fine = recon.render_mesh(mesh, res=fine_res(s), shade=shade, background=BG, lighting=lighting, **cam)
        assert isinstance(got, recon.ResolvedPicture) and isinstance(fine, recon.MeshRender), what
        want = resolved(fine, s, nearest)
        same(got, want, what)
        assert got.mask is None and (got.image is None) == (shade is None), what
        lead = cam["calibs"].shape[:-2]
        assert tuple(got.coverage.shape) == tuple(lead) + RES and got.coverage.dtype == torch.float32, what
        cov = host(got.coverage)
        assert ((cov > 0) & (cov < 1)).sum() > 20 and (cov == 1).sum() > 50 and (cov == 0).sum() > 50, what
        # the generic call on the fine picture, and a list with a None mesh
        same(recon.resolve_picture(fine, s, nearest), want, what + ("resolve_picture",))
        many = recon.render_mesh_many([mesh, None], res=RES, shade=shade, background=BG, lighting=lighting, samples=s,
                                      **cam)
        assert many[1] is None
        same(many[0], want, what + ("many",))
    # a flat colour stays that colour inside the silhouette and blends with the background along it
    flat = mesh._replace(colors=torch.full_like(mesh.verts, 0.75))
    got = recon.render_mesh(flat, res=RES, shade="colors", background=BG, samples=2, **cam)
    image, cov = host(got.image), host(got.coverage)
    assert (image[cov == 0] == F(BG)).all() and np.abs(image[cov == 1] - F(0.75)).max() < 1e-6
    edge = (cov > 0) & (cov < 1)
    assert (image[edge] > BG).all() and (image[edge] < 0.75).all()
    assert np.abs(image[edge][:, 0] - (cov[edge] * F(0.75) + (1 - cov[edge]) * F(BG))).max() < 1e-6


def scene_of(recon, light=True):
    """The carpet floor, 2.5 times as wide and raised to y = -0.3: it stands in the sphere and hides its lower cap."""
    vert_data, uv_data = carpet()
    vert_data = vert_data.copy()
    vert_data[:, [0, 2]] *= F(2.5)
    vert_data[:, 1] += F(0.6)
    sun = recon.Light.directional((0.3, -1.0, 0.2), (-1.5, -1.0, -1.5), (1.5, 1.0, 1.5), res=(64, 48)) if light else None
    return recon.Scene.from_packed(vert_data, uv_data, procedural(64, 64), device=DEV, light=sun)


ABOVE = dict(calibs=tilted(-0.7, focal=2.2, t=(0.0, 0.3, 3.0)), projection="perspective", nearest="min", near=0.5,
             perspective_correct=True)


@pytest.mark.parametrize("s", [2, 3])
def test_render_scene(recon, mesh, s):
    scene = scene_of(recon)
    for casters in (None, mesh):
        got = recon.render_scene(scene, res=RES, background=BG, casters=casters, samples=s, **ABOVE)
        fine = recon.render_scene(scene, res=fine_res(s), background=BG, casters=casters, **ABOVE)
        assert isinstance(got, recon.ResolvedPicture) and got.mask is None
        same(got, resolved(fine, s, "min"), (s, casters is not None))
        cov = host(got.coverage)
        assert ((cov > 0) & (cov < 1)).sum() > 10 and (cov == 1).sum() > 30


@pytest.mark.parametrize("composite", ["depth", "over"])
@pytest.mark.parametrize("s", [2, 3])
def test_render_mesh_many_in_scene(recon, mesh, s, composite):
    scene = scene_of(recon)
    lighting = lighting_of(recon, self_shadow=0.05)
    kw = dict(shade="colors", background=BG, composite=composite, lighting=lighting, **ABOVE)
    got = recon.render_mesh_many_in_scene([mesh, None], scene, res=RES, samples=s, **kw)
    fine = recon.render_mesh_many_in_scene([mesh, None], scene, res=fine_res(s), **kw)
    for b in range(2):
        assert isinstance(got[b], recon.ResolvedPicture) and isinstance(fine[b], recon.ScenePicture)
        same(got[b], resolved(fine[b], s, "min"), (s, composite, b))
    mask, cov = host(got[0].mask), host(got[0].coverage)
    counts = np.bincount(mask.reshape(-1), minlength=3)
    print("masks 0/1/2: %s, partly covered: %d" % (counts.tolist(), int(((cov > 0) & (cov < 1)).sum())))
    assert counts[1] > 20 and counts[2] > 20 and ((cov > 0) & (cov < 1)).sum() > 10
    # mask and coverage come from the composite's mask: the subject's samples are those where it shows
    want = (host(fine[0].mask) == 2).reshape(RES[0], s, RES[1], s).sum(axis=(1, 3)).astype(F) / F(s * s)
    assert np.array_equal(cov, want) and np.array_equal(mask > 1, cov > 0)
    # no mesh: the bare scene, no subject anywhere
    assert int(host(got[1].mask).max()) == 1 and not host(got[1].coverage).any() and (host(got[1].face) == -1).all()
    bare = recon.render_scene(scene, res=RES, background=BG, samples=s, **ABOVE)
    assert rr.same_bits(host(got[1].image), host(bare.image)) and rr.same_bits(host(got[1].depth), host(bare.depth))


def test_render_mesh_netc(recon, mesh33, heads):  # noqa: F811
    """shade="netC" queries every covered fine sample: the same construction."""
    s = 2
    net, calib, feat = heads["nets"]["orthogonal"], heads["calibs"]["orthogonal"], heads["maps"]["64x64"]
    cam = dict(picture_cameras()["orthogonal"], res=RES)
    kw = dict(shade="netC", background=BG, netC=net, feat_tensor_C=feat, calib_tensor=calib)
    got = recon.render_mesh(mesh33, samples=s, **kw, **cam)
    fine = recon.render_mesh(mesh33, **kw, **dict(cam, res=fine_res(s)))
    same(got, resolved(fine, s, "max"), "netC")
    cov = host(got.coverage)
    assert ((cov > 0) & (cov < 1)).sum() > 20 and float(host(got.image)[cov == 1].std()) > 0.01


def test_samples_1_is_the_call_without_the_keyword(recon, mesh):
    scene = scene_of(recon)
    cam = CAMERAS["perspective"]
    pairs = [(recon.render_mesh(mesh, res=RES, background=BG, samples=1, **cam),
              recon.render_mesh(mesh, res=RES, background=BG, **cam), recon.MeshRender),
             (recon.render_mesh_many([mesh], res=RES, shade=None, samples=1, **cam)[0],
              recon.render_mesh_many([mesh], res=RES, shade=None, **cam)[0], recon.MeshRender),
             (recon.render_scene(scene, res=RES, samples=1, **ABOVE), recon.render_scene(scene, res=RES, **ABOVE),
              recon.MeshRender),
             (recon.render_mesh_many_in_scene([mesh], scene, res=RES, samples=1, **ABOVE)[0],
              recon.render_mesh_many_in_scene([mesh], scene, res=RES, **ABOVE)[0], recon.ScenePicture)]
    for got, want, kind in pairs:
        assert type(got) is kind and type(want) is kind
        for a, b in zip(got, want):
            assert rr.same_bits(host(a), host(b))


def test_refusals_before_anything_is_enqueued(recon, mesh):
    scene = scene_of(recon, light=False)
    eye = torch.eye(4)
    for samples in (0, 5, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="samples must be"):
            recon.render_mesh(mesh, eye, RES, samples=samples)
        with pytest.raises(ValueError, match="samples must be"):
            recon.render_mesh(None, eye, RES, samples=samples)
        with pytest.raises(ValueError, match="samples must be"):
            recon.render_mesh_many([mesh], eye, RES, samples=samples)
        with pytest.raises(ValueError, match="samples must be"):
            recon.render_scene(scene, eye, RES, samples=samples)
        with pytest.raises(ValueError, match="samples must be"):
            recon.render_mesh_many_in_scene([mesh], scene, eye, RES, samples=samples)
    for res, samples in (((2049, 8), 2), ((8, 1366), 3), (1025, 4)):
        for call in (lambda: recon.render_mesh(mesh, eye, res, samples=samples),
                     lambda: recon.render_mesh_many([mesh], eye, res, samples=samples),
                     lambda: recon.render_scene(scene, eye, res, samples=samples),
                     lambda: recon.render_mesh_many_in_scene([mesh], scene, eye, res, samples=samples)):
            with pytest.raises(ValueError, match="outside 1..4096"):
                call()
    with pytest.raises(ValueError, match="samples must be"):
        recon.resolve_picture(recon.render_mesh(mesh, eye, RES), 1)
    with pytest.raises(ValueError, match="MeshRender"):
        recon.resolve_picture((None, None, None), 2)
