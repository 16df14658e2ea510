"""mp_mesh_render / mp_mesh_render_batch (csrc/raster.hip), ops.mesh_render_raw(_batch) and recon.render_mesh(_many) on
the GPU, bit for bit against the numpy restatement of the definition (tests/mesh_render_ref.py).  The restatement is fed
the coordinates the existing ops.orthogonal / ops.perspective return for the same vertices (step 1 of the definition
has its own parity tests); depth, face ids and image are compared with array_equal on the bits.  Needs an MI355X."""
import ctypes
import math

import numpy as np
import pytest

import mesh_render_ref as ref
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, -1, -3  # MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED (include/monoport_hip.h)
INF = math.inf
NORMALS = dict(scale=0.5, bias=0.5, lo=0.0, hi=1.0)   # main.py:220-225
PREDS = dict(scale=0.5, bias=0.5, lo=-INF, hi=INF)    # raw netC predictions
SIZES = [(33, 33), (66, 66), (28, 28), (40, 24)]


def _cameras():
    from monoport_amd import recon
    persp = np.eye(4, dtype=np.float32)
    persp[0, 0] = persp[1, 1] = 2.5
    persp[:3, 3] = [0.2, -0.1, 3.0]  # the body at z = 2.3 .. 3.6, in front of the camera
    return {"identity": (torch.eye(4), "orthogonal"),
            "scene": (recon.pifu_calib(*syn.scene_camera(step=3), device="cpu")[0], "orthogonal"),
            "perspective": (torch.from_numpy(persp), "perspective")}


CAMERAS = ["identity", "scene", "perspective"]


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


@pytest.fixture(scope="module")
def cameras():
    return _cameras()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(t):
    return None if t is None else t.cpu().numpy()


def projected(ops, verts, calib, projection):
    """[N,3] numpy: what the existing projection calls give for these vertices."""
    if verts.shape[0] == 0:
        return np.zeros((0, 3), np.float32)
    fn = ops.orthogonal if projection == "orthogonal" else ops.perspective
    return fn(verts.t().contiguous()[None], calib[None].to(verts.device))[0].t().cpu().numpy()


def assert_same(got, want, what=""):
    """(image, depth, face) of the device against a ``ref.Rendered``, bit for bit."""
    image, depth, face = got
    if face is not None:
        assert np.array_equal(host(face), want.face), what
    if depth is not None:
        assert np.array_equal(bits(host(depth)), bits(want.depth)), what
    if image is not None:
        assert np.array_equal(bits(host(image)), bits(want.image)), what


@pytest.fixture(scope="module")
def body33(ops):
    """The device's own marching cubes of blob_volume(33, 5), its normals, and seeded channel-major values."""
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    verts, faces, counts = ops.marching_cubes_raw(vol)
    normals = ops.mesh_normals_raw(verts, faces, counts, out=torch.zeros_like(verts))
    nv, nf = counts.cpu().tolist()
    assert 0 < nv <= verts.shape[0] and 0 < nf <= faces.shape[0]
    seeded = torch.from_numpy(np.random.RandomState(3).standard_normal((3, verts.shape[0])).astype(np.float32)).to(DEV)
    return dict(vol=vol, verts=verts, faces=faces, counts=counts, nv=nv, nf=nf, normals=normals, seeded=seeded,
                xyz={})


def body_reference(ops, body33, cameras, cam, size, nearest):
    """The restatement's two pictures (normals row-major, seeded values channel-major) of body33."""
    calib, projection = cameras[cam]
    if cam not in body33["xyz"]:
        body33["xyz"][cam] = projected(ops, body33["verts"][:body33["nv"]], calib, projection)
    xyz, faces = body33["xyz"][cam], host(body33["faces"][:body33["nf"]])
    return (ref.render(xyz, faces, *size, attr=host(body33["normals"][:body33["nv"]]), nearest=nearest, **NORMALS),
            ref.render(xyz, faces, *size, attr=host(body33["seeded"][:, :body33["nv"]]), channel_major=True,
                       nearest=nearest, background=0.25, **PREDS))


@pytest.mark.parametrize("nearest", ["max", "min"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cam", CAMERAS)
def test_bit_for_bit_against_the_restatement(ops, body33, cameras, cam, size, nearest):
    calib, projection = cameras[cam]
    want_n, want_s = body_reference(ops, body33, cameras, cam, size, nearest)
    assert (want_n.face >= 0).sum() > 60
    b = body33
    got = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], b["normals"], calib, size, projection, nearest,
                              **NORMALS)
    assert tuple(got[0].shape) == (1,) + size + (3,) and tuple(got[1].shape) == tuple(got[2].shape) == (1,) + size
    assert_same([t[0] for t in got], want_n, "normals")
    got = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], b["seeded"], calib, size, projection, nearest,
                              channel_major=True, background=0.25, **PREDS)
    assert_same([t[0] for t in got], want_s, "seeded")


@pytest.mark.parametrize("cam,size,nearest", [("identity", (33, 33), "max"), ("perspective", (40, 24), "min")])
def test_each_output_alone(ops, body33, cameras, cam, size, nearest):
    calib, projection = cameras[cam]
    want = body_reference(ops, body33, cameras, cam, size, nearest)[0]
    b = body33
    image = torch.full((1,) + size + (3,), -5.0, device=DEV)
    depth = torch.full((1,) + size, -5.0, device=DEV)
    face = torch.full((1,) + size, -5, dtype=torch.int32, device=DEV)
    for pick in ((0,), (1,), (2,), (0, 1, 2)):
        out = [t.clone() if k in pick else None for k, t in enumerate((image, depth, face))]
        got = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], b["normals"], calib, size, projection, nearest,
                                  out=tuple(out), **NORMALS)
        for k in range(3):
            assert (got[k] is None) == (k not in pick)
            assert got[k] is None or got[k].data_ptr() == out[k].data_ptr()
        assert_same([None if t is None else t[0] for t in got], want, str(pick))
    # without attributes: depth and face ids only
    got = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], None, calib, size, projection, nearest)
    assert got[0] is None
    assert_same([None, got[1][0], got[2][0]], want)


def soup():
    """Both face paths on a 64 x 64 image: two triangles that span the whole image and reach beyond it, some dozens of 1
    to 20 pixels in front of and behind them, the normals soup (huge and tiny coordinates, a 200-face fan, degenerate
    faces) and faces the definition skips.  (verts [N,3] in projected coordinates, faces, attr [N,3])."""
    rng = np.random.RandomState(23)
    size = 64
    pix = [[-10.0, -12.0, 0.1], [90.0, -9.0, -0.2], [-11.0, 85.0, 0.3], [88.0, 91.0, -0.1]]
    faces = [[0, 1, 2], [3, 2, 1]]
    for k in range(96):
        c = rng.uniform(2, 62, 2)
        ext = rng.choice([1.0, 2.0, 3.0, 5.0, 8.0, 9.0, 20.0])
        tri = c + rng.uniform(-ext / 2, ext / 2, (3, 2))
        z = rng.uniform(-0.6, 0.6) + rng.uniform(-0.1, 0.1, 3)
        base = len(pix)
        pix += [[tri[i, 0], tri[i, 1], z[i]] for i in range(3)]
        faces.append([base, base + 1, base + 2] if k % 2 else [base, base + 2, base + 1])
    # boxes of exactly 8 x 8 = 64 and 8 x 9 = 72 pixel centres: either side of any threshold near 64
    for (x0, y0, nx, ny) in ((10.25, 20.25, 8, 8), (30.25, 40.25, 8, 9), (40.25, 5.25, 9, 8)):
        base = len(pix)
        pix += [[x0, y0, 0.5], [x0 + nx, y0, 0.55], [x0, y0 + ny, 0.6]]
        faces.append([base, base + 1, base + 2])
    xyz = ref.to_ndc(np.array(pix), size, size)
    sv, sf, _ = syn.normals_soup_mesh()
    sv[:500] *= np.array([0.3, 0.003, 300.0], np.float32)  # the soup's wide axis (sigma 100) within the image, mostly
    sv[500:, :2] *= 0.8                                      # the collinear points, the lonely ones and the fan
    n0 = len(xyz)
    xyz = np.concatenate([xyz, sv.astype(np.float32)])
    faces = np.concatenate([np.array(faces), sf.astype(np.int64) + n0])
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, 0.0, np.inf], [3.0e6, 0.0, 0.0]], np.float32)
    n1 = len(xyz)
    xyz = np.concatenate([xyz, bad])
    skipped = [[0, 1, n1], [2, n1 + 1, 3], [0, n1 + 2, 2], [0, 1, n1 + 3], [-1, 2, 3], [5, 5, 6], [7, 7, 7]]
    faces = np.concatenate([faces, np.array(skipped)]).astype(np.int32)
    attr = np.random.RandomState(29).standard_normal((len(xyz), 3)).astype(np.float32)
    return xyz.astype(np.float32), faces, attr, size


@pytest.mark.parametrize("nearest", ["max", "min"])
def test_both_face_paths(ops, nearest):
    xyz, faces, attr, size = soup()
    verts = torch.from_numpy(xyz).to(DEV)
    calib = torch.eye(4)
    want = ref.render(projected(ops, verts, calib, "orthogonal"), faces, size, size, attr=attr, nearest=nearest, **PREDS)
    assert want.cover.min() >= 1 and (want.cover > 2).sum() > 500  # the two spanning triangles, and much in front
    assert (want.face <= 1).sum() > 100 and len(np.unique(want.face)) > 100
    counts = torch.tensor([len(xyz), len(faces)], dtype=torch.int32, device=DEV)
    got = ops.mesh_render_raw(verts, torch.from_numpy(faces).to(DEV), counts, torch.from_numpy(attr).to(DEV), calib,
                              size, nearest=nearest, **PREDS)
    assert_same([t[0] for t in got], want)


def test_contention(ops):
    """2 000 faces of identical geometry and depth over the same four pixels."""
    size = 8
    xyz = ref.to_ndc(np.array([[3.5625, 2.8125, 0.3], [2.3125, 4.5625, -0.4], [5.0625, 5.0625, 0.7]]), size, size)
    faces = np.tile(np.array([[0, 1, 2]], np.int32), (2000, 1))
    verts = torch.from_numpy(xyz).to(DEV)
    calib = torch.eye(4)
    want = ref.render(projected(ops, verts, calib, "orthogonal"), faces, size, size)
    assert (want.cover == 2000).sum() == 4 and (want.cover > 0).sum() == 4
    counts = torch.tensor([3, 2000], dtype=torch.int32, device=DEV)
    runs = [ops.mesh_render_raw(verts, torch.from_numpy(faces).to(DEV), counts, None, calib, size) for _ in range(2)]
    for _, depth, face in runs:
        assert set(face.unique().tolist()) == {-1, 0}
        assert_same([None, depth[0], face[0]], want)
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    assert torch.equal(runs[0][2], runs[1][2])


@pytest.fixture(scope="module")
def vols33():
    """Unequal vertex / face counts, and one empty mesh."""
    return [torch.from_numpy(v).to(DEV) for v in (syn.blob_volume(33, 5), syn.sphere_volume(33), syn.blob_volume(33, 7),
                                                  np.zeros((33, 33, 33), np.float32))]


def two_views(cameras):
    return torch.stack([cameras["identity"][0], cameras["scene"][0]])


def equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("caps", [None, (30, 10), (300, 100)], ids=["roomy", "truncated", "truncated300"])
def test_batch_equals_per_mesh(ops, vols33, cameras, caps):
    kw = {} if caps is None else dict(max_verts=caps[0], max_faces=caps[1])
    raws = ops.marching_cubes_raw_batch(vols33, **kw)
    verts, faces, counts = ([r[k] for r in raws] for k in range(3))
    need = torch.stack(counts).cpu().tolist()
    assert need[3] == [0, 0] and len({tuple(c) for c in need}) == 4
    if caps is not None:
        assert all(c[0] > caps[0] and c[1] > caps[1] for c in need[:3])
    attrs = [torch.from_numpy(np.random.RandomState(40 + k).standard_normal(tuple(v.shape)).astype(np.float32)).to(DEV)
             for k, v in enumerate(verts)]
    views = two_views(cameras)
    batch = ops.mesh_render_raw_batch(verts, faces, counts, attrs, [views] * 4, (40, 24), background=0.5, **NORMALS)
    for f in range(4):
        single = ops.mesh_render_raw(verts[f], faces[f], counts[f], attrs[f], views, (40, 24), background=0.5, **NORMALS)
        for v in range(2):
            one = ops.mesh_render_raw(verts[f], faces[f], counts[f], attrs[f], views[v], (40, 24), background=0.5,
                                      **NORMALS)
            for k in range(3):
                assert equal_bits(batch[f][k], single[k]), (f, k)
                assert equal_bits(batch[f][k][v], one[k][0]), (f, v, k)
    assert (batch[3][0] == 0.5).all() and (batch[3][1] == 0).all() and (batch[3][2] == -1).all()  # counts {0, 0}
    # ... and against the definition on the rows a truncated mesh keeps
    nv, nf = (min(need[0][0], verts[0].shape[0]), min(need[0][1], faces[0].shape[0]))
    want = ref.render(projected(ops, verts[0][:nv], views[1], "orthogonal"), host(faces[0][:nf]), 40, 24,
                      attr=host(attrs[0][:nv]), background=0.5, **NORMALS)
    # (at 30 / 10 six faces of mesh 0 keep all their vertices and none covers a centre under this camera)
    assert caps == (30, 10) or (want.face >= 0).sum() > 20
    assert_same([t[1] for t in batch[0]], want)


def test_33_image_slots_cross_the_chunking(ops, vols33, cameras):
    assert ops.MAX_FRAMES == 32
    raws = ops.marching_cubes_raw_batch([vols33[k % 4] for k in range(11)])
    verts, faces, counts = ([r[k] for r in raws] for k in range(3))
    views = torch.stack([cameras["identity"][0], cameras["scene"][0], cameras["identity"][0].flip(0)[[2, 1, 0, 3]]])
    cams = [views.roll(k, 0) for k in range(11)]  # every mesh its own order of the three cameras
    batch = ops.mesh_render_raw_batch(verts, faces, counts, None, cams, 28)
    assert all(b[0] is None for b in batch)
    for f in range(11):
        single = ops.mesh_render_raw(verts[f], faces[f], counts[f], None, cams[f], 28)
        assert equal_bits(batch[f][1], single[1]) and equal_bits(batch[f][2], single[2]), f
    assert not equal_bits(batch[0][1], batch[4][1])  # same mesh, rolled cameras


def test_render_mesh_many_shared_and_per_mesh_cameras(recon, vols33, cameras):
    sdfs = [vols33[0], None, vols33[1], vols33[2]]
    meshes = recon.reconstruct_mesh_many(sdfs)
    assert meshes[1] is None and len({m.verts.shape[0] for m in meshes if m is not None}) == 3
    views = two_views(cameras)
    shared = recon.render_mesh_many(meshes, views, res=(40, 24), shade="normals")
    per_mesh = recon.render_mesh_many(meshes, [views, None, views, views], res=(40, 24), shade="normals")
    assert shared[1] is None and per_mesh[1] is None
    for i in (0, 2, 3):
        alone = recon.render_mesh(meshes[i], views, res=(40, 24), shade="normals")
        assert tuple(alone.image.shape) == (2, 40, 24, 3)
        first = recon.render_mesh(meshes[i], views[0], res=(40, 24), shade="normals")
        assert tuple(first.image.shape) == (40, 24, 3)
        for k in range(3):
            assert equal_bits(shared[i][k], alone[k]) and equal_bits(per_mesh[i][k], alone[k]), (i, k)
            assert equal_bits(first[k], alone[k][0]), (i, k)
        assert (alone.face >= 0).sum() > 100
    swapped = recon.render_mesh_many(meshes, [views.flip(0), None, views, views], res=(40, 24), shade=None)
    assert swapped[0].image is None
    assert equal_bits(swapped[0].depth[0], shared[0].depth[1]) and equal_bits(swapped[2].depth, shared[2].depth)


@pytest.mark.parametrize("r,seed", [(33, 5), (17, 3)])
def test_end_to_end_silhouette_is_the_visible_surface(recon, r, seed):
    vol = torch.from_numpy(syn.blob_volume(r, seed)).to(DEV)[None, None]
    mesh = recon.reconstruct_mesh(vol)
    out = recon.render_mesh(mesh, torch.eye(4), res=r, shade="normals")
    x, y, _, _ = recon.forward_vertices(vol, "front")
    want = torch.zeros((r, r), dtype=torch.bool, device=DEV)
    want[x, y] = True
    assert want.sum() > 40
    assert torch.equal(out.face >= 0, want)
    assert torch.equal((out.image != 1.0).any(-1), want)  # a painted normal is never pure white
    assert ((out.image >= 0) & (out.image <= 1)).all()
    norm, tex, mask = recon.visulization(out.image, None, render_size=64)
    assert norm.shape == (64, 64, 3) and tex is None and mask.shape == (64, 64, 1) and 0 < mask.sum() < 64 * 64
    assert recon.render_mesh(None, torch.eye(4)) is None


# ---- refusals ---------------------------------------------------------------------------------------------------------

class Env:
    """A well-formed call of both entry points on real buffers; every test changes one argument."""
    ORDER = {
        "mp_mesh_render": "verts max_v faces max_f counts attr ch_major calib proj nearest h w scale bias lo hi bg image "
                          "depth face stream",
        "mp_mesh_render_batch": "n verts max_v faces max_f counts attr ch_major n_views calib proj nearest h w scale "
                                "bias lo hi bg image depth face stream",
    }

    def __init__(self):
        from monoport_amd import ops
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        self.n, self.nv, self.h, self.w = 2, 2, 6, 5
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
        self.verts, self.attr = z(self.n, 9, 3), z(self.n, 9, 3)
        self.faces, self.counts = z(self.n, 4, 3, dtype=torch.int32), z(self.n, 2, dtype=torch.int32)
        self.image, self.depth = z(self.n, self.nv, self.h, self.w, 3), z(self.n, self.nv, self.h, self.w)
        self.face = z(self.n, self.nv, self.h, self.w, dtype=torch.int32)
        self.odd = z(64)[1:].view(torch.uint8)[1:]  # an address that is not 4-byte aligned
        assert self.odd.data_ptr() % 4 == 1
        self.calib = (ctypes.c_float * (12 * self.n * self.nv))(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] * (self.n * self.nv)))
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def args(self, name):
        batch = name.endswith("_batch")
        one = (lambda t: ctypes.c_void_p(t[0].data_ptr()))
        many = (lambda t: (ctypes.c_void_p * self.n)(*[r.data_ptr() for r in t]))
        p = many if batch else one
        a = dict(verts=p(self.verts), max_v=9, faces=p(self.faces), max_f=4, counts=p(self.counts), attr=p(self.attr),
                 ch_major=0, calib=self.calib, proj=0, nearest=0, h=self.h, w=self.w, scale=1.0, bias=0.0, lo=-INF,
                 hi=INF, bg=1.0, image=p(self.image), depth=p(self.depth), face=p(self.face), stream=self.stream)
        if batch:
            a.update(n=self.n, n_views=self.nv)
        return a

    def call(self, name, **changed):
        a = self.args(name)
        a.update(changed)
        rc = getattr(self.lib, name)(self.ctx.handle, *[a[k] for k in self.ORDER[name].split()])
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()


@pytest.fixture(scope="module")
def env():
    return Env()


ENTRIES = ["mp_mesh_render", "mp_mesh_render_batch"]
REFUSED = [
    ("h", dict(h=0), ARG), ("h", dict(h=4097), ARG), ("w", dict(w=0), ARG), ("w", dict(w=4097), ARG),
    ("projection", dict(proj=2), ARG), ("projection", dict(proj=-1), ARG),
    ("nearest", dict(nearest=2), ARG), ("nearest", dict(nearest=-1), ARG),
    ("no output", dict(image=None, depth=None, face=None), ARG),
    ("image without attr", dict(attr=None), ARG),
    ("capacity", dict(max_v=2 ** 31 // 3 + 1), UNSUPPORTED), ("capacity", dict(max_f=2 ** 31 // 3 + 1), UNSUPPORTED),
]


@pytest.mark.parametrize("name", ENTRIES)
def test_a_well_formed_call_is_accepted(env, name):
    rc, _ = env.call(name)
    assert rc == OK
    rc, _ = env.call(name, attr=None, image=None)
    assert rc == OK
    rc, _ = env.call(name, depth=None, face=None)
    assert rc == OK
    torch.cuda.synchronize()
    written = env.image[0, 0] if name == "mp_mesh_render" else env.image
    assert (written == 1.0).all()  # counts {0, 0}: pure background


@pytest.mark.parametrize("what,changed,code", REFUSED, ids=[r[0] + str(i) for i, r in enumerate(REFUSED)])
@pytest.mark.parametrize("name", ENTRIES)
def test_refusals(env, name, what, changed, code):
    rc, msg = env.call(name, **changed)
    assert rc == code, (what, msg)
    assert msg.startswith(name + ":"), msg


@pytest.mark.parametrize("buffer", ["verts", "faces", "counts", "attr", "image", "depth", "face"])
@pytest.mark.parametrize("name", ENTRIES)
def test_null_and_misaligned_buffers(env, name, buffer):
    tensor = dict(verts=env.verts, faces=env.faces, counts=env.counts, attr=env.attr, image=env.image, depth=env.depth,
                  face=env.face)[buffer]
    for address, word in ((env.odd.data_ptr(), "misaligned"), (None, "null")):
        if name.endswith("_batch"):
            rows = [r.data_ptr() for r in tensor]
            arg = (ctypes.c_void_p * env.n)(*(rows[:-1] + [address]))
        else:
            if address is None and buffer in ("attr", "image", "depth", "face"):
                continue  # a NULL here is "not requested" in the per-mesh form
            arg = ctypes.c_void_p(address)
        rc, msg = env.call(name, **{buffer: arg})
        assert rc == ARG and msg.startswith(name + ":") and word in msg, (buffer, word, msg)


def test_image_slots_per_call(env):
    for n, n_views in ((0, 1), (1, 0), (33, 1), (1, 33), (2, 17), (-1, 1)):
        many = (lambda t: (ctypes.c_void_p * max(n, 1))(*([t[0].data_ptr()] * max(n, 1))))  # noqa: E731
        rc, msg = env.call("mp_mesh_render_batch", n=n, n_views=n_views, verts=many(env.verts), faces=many(env.faces),
                           counts=many(env.counts), attr=many(env.attr), image=many(env.image), depth=many(env.depth),
                           face=many(env.face))
        assert rc == ARG and msg.startswith("mp_mesh_render_batch:"), (n, n_views, msg)


def test_python_layer_refusals(ops, recon, body33, cameras):
    b = body33
    eye = torch.eye(4)
    good = (b["verts"], b["faces"], b["counts"], b["normals"], eye, 16)
    with pytest.raises(ValueError, match="projection"):
        ops.mesh_render_raw(*good, projection="fisheye")
    with pytest.raises(ValueError, match="nearest"):
        ops.mesh_render_raw(*good, nearest="closest")
    for res in (0, 4097, (16, 0), (5000, 16)):
        with pytest.raises(ValueError, match="image size"):
            ops.mesh_render_raw(*good[:5], res)
    with pytest.raises(ValueError, match="calibs"):
        ops.mesh_render_raw(*good[:4], torch.eye(3), 16)
    with pytest.raises(ValueError, match="attr"):
        ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], b["seeded"], eye, 16)  # [3,V] given as row-major
    with pytest.raises(ValueError, match="attr"):
        ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], None, eye, 16,
                            out=(torch.zeros(1, 16, 16, 3, device=DEV), None, None))
    with pytest.raises(ValueError, match="out"):
        ops.mesh_render_raw(*good, out=(None, None, None))
    with pytest.raises(ValueError, match="depth"):
        ops.mesh_render_raw(*good, out=(None, torch.zeros(1, 16, 15, device=DEV), None))
    with pytest.raises(ValueError, match="faces"):
        ops.mesh_render_raw(b["verts"], b["faces"].long(), b["counts"], None, eye, 16)
    with pytest.raises(ValueError, match="capacity"):
        ops.mesh_render_raw_batch([b["verts"], b["verts"][:-1]], [b["faces"]] * 2, [b["counts"]] * 2, None, [eye] * 2,
                                  16)
    with pytest.raises(ValueError, match="calibrations"):
        ops.mesh_render_raw_batch([b["verts"]] * 2, [b["faces"]] * 2, [b["counts"]] * 2, None, [eye], 16)
    with pytest.raises(ValueError, match="views"):
        ops.mesh_render_raw_batch([b["verts"]] * 2, [b["faces"]] * 2, [b["counts"]] * 2, None,
                                  [eye, torch.stack([eye, eye])], 16)
    mesh = recon.Mesh(b["verts"][:b["nv"]], b["faces"][:b["nf"]], b["normals"][:b["nv"]], None)
    with pytest.raises(ValueError, match="colors"):
        recon.render_mesh(mesh, eye, res=16)  # shade="colors" on a mesh without colours
    with pytest.raises(ValueError, match="normals"):
        recon.render_mesh(mesh._replace(normals=None), eye, res=16, shade="normals")
    with pytest.raises(ValueError, match="shade"):
        recon.render_mesh(mesh, eye, res=16, shade="depth")
    with pytest.raises(ValueError, match="camera sets"):
        recon.render_mesh_many([mesh, mesh], [eye], res=16, shade=None)
    assert recon.render_mesh(mesh, eye, res=16, shade="normals").image.shape == (16, 16, 3)
