"""mp_mesh_render_clip / mp_mesh_render_clip_batch (csrc/raster.hip: raster_*_clip), the ``near`` / ``perspective_correct``
keywords of ops.mesh_render_raw(_batch) and recon.render_mesh(_many) on the GPU, bit for bit against the numpy
restatement of the definition (tests/mesh_render_clip_ref.py).  The restatement is fed the camera-space coordinates
ops.orthogonal returns for the camera's [R|t]; depth, face ids and image are compared with array_equal on the bits.
Needs an MI355X."""
import ctypes
import math

import numpy as np
import pytest

import mesh_render_clip_ref as clip
import scratch_cases as cases
from monoport_amd import synthetic as syn
from test_mesh_render_gpu import ARG, DEV, NORMALS, OK, PREDS, UNSUPPORTED, Env, assert_same, equal_bits, host

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
INF = math.inf
SIZES = [(33, 33), (66, 66), (40, 24)]


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def _cameras():
    """Two perspective cameras on the body of blob_volume(33, 5) (inside [-1, 1]^3)."""
    a = np.eye(4, dtype=np.float32)
    a[0, 0] = a[1, 1] = 2.5
    a[:3, 3] = [0.2, -0.1, 3.0]
    cy, sy, cx, sx = math.cos(0.7), math.sin(0.7), math.cos(-0.35), math.sin(-0.35)
    rot = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    b = np.eye(4, dtype=np.float32)
    b[:3, :3] = np.diag([2.0, 2.0, 1.0]) @ rot
    b[:3, 3] = [-0.15, 0.1, 2.6]
    return {"front": torch.from_numpy(a), "turned": torch.from_numpy(b.astype(np.float32))}


CAMERAS = _cameras()


def camera_space(ops, verts, calib):
    """[N,3] numpy: the rows of [R|t] p, as the existing orthogonal projection call returns them."""
    if verts.shape[0] == 0:
        return np.zeros((0, 3), np.float32)
    return ops.orthogonal(verts.t().contiguous()[None], calib[None].to(verts.device))[0].t().cpu().numpy()


@pytest.fixture(scope="module")
def body33(ops):
    """The device's own marching cubes of blob_volume(33, 5), its normals, seeded channel-major values; per camera the
    camera-space vertices and the plane through the median depth, which is sure to cut the body."""
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    verts, faces, counts = ops.marching_cubes_raw(vol)
    normals = ops.mesh_normals_raw(verts, faces, counts, out=torch.zeros_like(verts))
    nv, nf = counts.cpu().tolist()
    assert 0 < nv <= verts.shape[0] and 0 < nf <= faces.shape[0]
    seeded = torch.from_numpy(np.random.RandomState(3).standard_normal((3, verts.shape[0])).astype(np.float32)).to(DEV)
    cam = {k: camera_space(ops, verts[:nv], c) for k, c in CAMERAS.items()}
    near = {k: float(np.median(c[:, 2])) for k, c in cam.items()}
    return dict(vol=vol, verts=verts, faces=faces, counts=counts, nv=nv, nf=nf, normals=normals, seeded=seeded, cam=cam,
                near=near, want={})


def body_reference(b, cam, size, nearest, pc):
    """The restatement's two pictures (normals row-major, seeded values channel-major) of body33, made once."""
    key = (cam, size, nearest, pc)
    if key not in b["want"]:
        faces = host(b["faces"][:b["nf"]])
        kw = dict(near=b["near"][cam], perspective_correct=pc, nearest=nearest)
        b["want"][key] = (
            clip.render(b["cam"][cam], faces, *size, attr=host(b["normals"][:b["nv"]]), **kw, **NORMALS),
            clip.render(b["cam"][cam], faces, *size, attr=host(b["seeded"][:, :b["nv"]]), channel_major=True,
                        background=0.25, **kw, **PREDS))
    return b["want"][key]


@pytest.mark.parametrize("pc", [False, True], ids=["affine", "correct"])
@pytest.mark.parametrize("nearest", ["max", "min"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_bit_for_bit_against_the_restatement(ops, body33, cam, size, nearest, pc):
    b = body33
    want_n, want_s = body_reference(b, cam, size, nearest, pc)
    for kind in range(4):  # a test that clips nothing shows nothing
        assert (want_n.kind == kind).sum() >= 10, (kind, np.bincount(want_n.kind))
    assert (want_n.face >= 0).sum() > 60
    kw = dict(projection="perspective", nearest=nearest, near=b["near"][cam], perspective_correct=pc)
    got = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], b["normals"], CAMERAS[cam], size, **kw, **NORMALS)
    assert tuple(got[0].shape) == (1,) + size + (3,) and tuple(got[1].shape) == tuple(got[2].shape) == (1,) + size
    assert_same([t[0] for t in got], want_n, "normals")
    got = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], b["seeded"], CAMERAS[cam], size, channel_major=True,
                              background=0.25, **kw, **PREDS)
    assert_same([t[0] for t in got], want_s, "seeded")


@pytest.mark.parametrize("cam,size,nearest,pc", [("front", (33, 33), "max", False), ("turned", (40, 24), "min", True)])
def test_each_output_alone(ops, body33, cam, size, nearest, pc):
    b = body33
    want = body_reference(b, cam, size, nearest, pc)[0]
    kw = dict(projection="perspective", nearest=nearest, near=b["near"][cam], perspective_correct=pc)
    image = torch.full((1,) + size + (3,), -5.0, device=DEV)
    depth = torch.full((1,) + size, -5.0, device=DEV)
    face = torch.full((1,) + size, -5, dtype=torch.int32, device=DEV)
    for pick in ((0,), (1,), (2,), (0, 1, 2)):
        out = [t.clone() if k in pick else None for k, t in enumerate((image, depth, face))]
        got = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], b["normals"], CAMERAS[cam], size, out=tuple(out),
                                  **kw, **NORMALS)
        for k in range(3):
            assert (got[k] is None) == (k not in pick)
            assert got[k] is None or got[k].data_ptr() == out[k].data_ptr()
        assert_same([None if t is None else t[0] for t in got], want, str(pick))
    got = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], None, CAMERAS[cam], size, **kw)
    assert got[0] is None
    assert_same([None, got[1][0], got[2][0]], want)


NEAR = 1.0


def soup():
    """Camera-space faces of all four kinds on a 64 x 64 image under the plane zc = 1: two that span its left half behind
    everything, some dozens of small ones astride the plane, vertices exactly on it, cut faces whose sub-triangles are
    too large for one thread, a cut vertex beyond the snap guard and faces the definition skips.  Returns (cam [N,3],
    faces, attr [N,3], size, the face ids by name)."""
    rng = np.random.RandomState(31)
    size = 64

    def at(px, py, z):  # the camera-space point that projects to pixel coordinates (px, py) at depth z
        return [(px * 2.0 / size - 1.0) * z, (py * 2.0 / size - 1.0) * z, z]

    pts = [at(-10, -12, 3.0), at(30, -9, 3.5), at(-11, 85, 2.5), at(28, 91, 3.0)]
    faces = [[0, 1, 2], [3, 2, 1]]
    for k in range(120):
        c = rng.uniform(4, 60, 2)
        ext = rng.choice([1.0, 2.0, 3.0, 5.0, 8.0, 9.0, 14.0])
        tri = c + rng.uniform(-ext / 2, ext / 2, (3, 2))
        z = rng.uniform(0.6, 1.5) + rng.uniform(-0.4, 0.4, 3)
        if k % 10 == 0:
            z[k // 10 % 3] = NEAR  # exactly on the plane: inside
        base = len(pts)
        pts += [at(tri[i, 0], tri[i, 1], z[i]) for i in range(3)]
        faces.append([base, base + 1, base + 2] if k % 2 else [base, base + 2, base + 1])
    named = {}
    base = len(pts)  # large and cut: one vertex behind the camera, then two
    pts += [at(5, 6, 2.0), at(50, 10, 1.8), [0.3, 2.5, -0.7], at(40, 8, 1.6), [-2.0, 1.0, 0.2], [1.5, 2.0, -0.1]]
    named["large2"], named["large1"] = len(faces), len(faces) + 1
    faces += [[base, base + 1, base + 2], [base + 4, base + 3, base + 5]]
    base = len(pts)  # the cut of the second edge lies at x = 5e6: beyond the guard, the face is skipped whole
    pts += [at(30, 30, 1.5), at(34, 31, 1.4), [1.0e7, 0.0, 0.5]]
    named["guard"] = len(faces)
    faces.append([base, base + 1, base + 2])
    base = len(pts)
    pts += [[np.nan, 0.0, 2.0], [0.0, 0.0, np.inf], [0.1, 0.1, np.nan], at(20, 20, 1.2)]
    named["skipped"] = len(faces)
    faces += [[0, 1, base], [2, base + 1, 3], [base + 3, base + 2, 5], [0, 1, base + 4], [-1, 2, 3], [5, 5, 6]]
    cam = np.array(pts, np.float32)
    attr = np.random.RandomState(37).standard_normal((len(cam), 3)).astype(np.float32)
    return cam, np.array(faces, np.int32), attr, size, named


@pytest.mark.parametrize("pc", [False, True], ids=["affine", "correct"])
@pytest.mark.parametrize("nearest", ["max", "min"])
def test_soup_of_every_kind_on_both_face_paths(ops, nearest, pc):
    cam, faces, attr, size, named = soup()
    verts = torch.from_numpy(cam).to(DEV)
    calib = torch.eye(4)
    xyz = camera_space(ops, verts, calib)
    finite = np.isfinite(cam).all(1)  # the identity camera: the soup as written (a NaN or inf spreads over its row)
    assert np.array_equal(xyz[finite].view(np.uint32), cam[finite].view(np.uint32)) and (~finite).sum() == 3
    assert not np.isfinite(xyz[~finite]).all(1).any()
    want = clip.render(xyz, faces, size, size, NEAR, pc, attr=attr, nearest=nearest, **PREDS)
    kinds = np.bincount(want.kind[want.kind >= 0], minlength=4)
    assert (kinds >= 10).all() and (want.kind == -1).sum() == 5, kinds
    assert (xyz[:, 2] == NEAR).sum() == 12
    seen = set(np.unique(want.face).tolist())
    assert {0, 1, named["large1"], named["large2"]} <= seen and len(seen) > 20
    assert want.kind[named["large1"]] == 1 and want.kind[named["large2"]] == 2
    if nearest == "min":  # with "max" the far half-image faces hide most of them
        assert (want.face == named["large1"]).sum() > 64 and (want.face == named["large2"]).sum() > 64
    assert want.kind[named["guard"]] == 2 and named["guard"] not in seen
    assert not seen & set(range(named["skipped"], len(faces)))
    counts = torch.tensor([len(cam), len(faces)], dtype=torch.int32, device=DEV)
    got = ops.mesh_render_raw(verts, torch.from_numpy(faces).to(DEV), counts, torch.from_numpy(attr).to(DEV), calib,
                              size, "perspective", nearest, near=NEAR, perspective_correct=pc, **PREDS)
    assert_same([t[0] for t in got], want)


@pytest.mark.parametrize("size", [(66, 66), (40, 24)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("nearest", ["max", "min"])
def test_a_mesh_wholly_in_front_is_the_unclipped_call(ops, body33, size, nearest):
    b = body33
    assert b["cam"]["front"][:, 2].min() > 2.0
    args = (b["verts"], b["faces"], b["counts"], b["normals"], CAMERAS["front"], size, "perspective", nearest)
    old = ops.mesh_render_raw(*args, **NORMALS)
    for near in (1.0, 2.0):
        new = ops.mesh_render_raw(*args, near=near, **NORMALS)
        for k in range(3):
            assert equal_bits(new[k], old[k]), (near, k)
    assert (old[2] >= 0).sum() > 60
    correct = ops.mesh_render_raw(*args, near=1.0, perspective_correct=True, **NORMALS)
    assert torch.equal(correct[2] >= 0, old[2] >= 0) and not equal_bits(correct[1], old[1])


@pytest.fixture(scope="module")
def meshes33(ops):
    """Unequal vertex / face counts, and one empty mesh."""
    vols = [torch.from_numpy(v).to(DEV) for v in (syn.blob_volume(33, 5), syn.sphere_volume(33), syn.blob_volume(33, 7),
                                                  np.zeros((33, 33, 33), np.float32))]
    raws = ops.marching_cubes_raw_batch(vols)
    need = torch.stack([r[2] for r in raws]).cpu().tolist()
    assert need[3] == [0, 0] and len({tuple(c) for c in need}) == 4
    return vols, raws


VIEWS = torch.stack([CAMERAS["front"], CAMERAS["turned"]])
CLIP = dict(projection="perspective", nearest="min", near=2.7, perspective_correct=True)


def test_batch_equals_per_mesh(ops, meshes33):
    verts, faces, counts = ([r[k] for r in meshes33[1]] for k in range(3))
    attrs = [torch.from_numpy(np.random.RandomState(40 + k).standard_normal(tuple(v.shape)).astype(np.float32)).to(DEV)
             for k, v in enumerate(verts)]
    batch = ops.mesh_render_raw_batch(verts, faces, counts, attrs, [VIEWS] * 4, (40, 24), background=0.5, **CLIP, **NORMALS)
    for f in range(4):
        single = ops.mesh_render_raw(verts[f], faces[f], counts[f], attrs[f], VIEWS, (40, 24), background=0.5, **CLIP,
                                     **NORMALS)
        for v in range(2):
            one = ops.mesh_render_raw(verts[f], faces[f], counts[f], attrs[f], VIEWS[v], (40, 24), background=0.5,
                                      **CLIP, **NORMALS)
            for k in range(3):
                assert equal_bits(batch[f][k], single[k]), (f, k)
                assert equal_bits(batch[f][k][v], one[k][0]), (f, v, k)
    assert (batch[3][0] == 0.5).all() and (batch[3][1] == 0).all() and (batch[3][2] == -1).all()  # counts {0, 0}
    nv, nf = counts[0].cpu().tolist()
    want = clip.render(camera_space(ops, verts[0][:nv], VIEWS[1]), host(faces[0][:nf]), 40, 24, CLIP["near"], True,
                       attr=host(attrs[0][:nv]), nearest="min", background=0.5, **NORMALS)
    assert all((want.kind == k).sum() >= 10 for k in range(4)) and (want.face >= 0).sum() > 20
    assert_same([t[1] for t in batch[0]], want)


def test_33_image_slots_cross_the_chunking(ops, meshes33):
    assert ops.MAX_FRAMES == 32
    raws = ops.marching_cubes_raw_batch([meshes33[0][k % 4] for k in range(11)])
    verts, faces, counts = ([r[k] for r in raws] for k in range(3))
    third = CAMERAS["front"].clone()
    third[0, 3] = -0.4
    views = torch.stack([CAMERAS["front"], CAMERAS["turned"], third])
    cams = [views.roll(k, 0) for k in range(11)]  # every mesh its own order of the three cameras
    batch = ops.mesh_render_raw_batch(verts, faces, counts, None, cams, 28, **CLIP)
    assert all(b[0] is None for b in batch)
    for f in range(11):
        single = ops.mesh_render_raw(verts[f], faces[f], counts[f], None, cams[f], 28, **CLIP)
        assert equal_bits(batch[f][1], single[1]) and equal_bits(batch[f][2], single[2]), f
    assert not equal_bits(batch[0][1], batch[4][1])  # same mesh, rolled cameras
    unclipped = ops.mesh_render_raw(verts[0], faces[0], counts[0], None, cams[0], 28, "perspective", "min")
    assert not equal_bits(batch[0][2], unclipped[2])  # the plane does cut


def test_render_mesh_many_shared_and_per_mesh_cameras(recon, meshes33):
    vols = meshes33[0]
    meshes = recon.reconstruct_mesh_many([vols[0], None, vols[1], vols[2]])
    assert meshes[1] is None and len({m.verts.shape[0] for m in meshes if m is not None}) == 3
    kw = dict(res=(40, 24), shade="normals", **CLIP)
    shared = recon.render_mesh_many(meshes, VIEWS, **kw)
    per_mesh = recon.render_mesh_many(meshes, [VIEWS, None, VIEWS, VIEWS], **kw)
    assert shared[1] is None and per_mesh[1] is None
    for i in (0, 2, 3):
        alone = recon.render_mesh(meshes[i], VIEWS, **kw)
        assert tuple(alone.image.shape) == (2, 40, 24, 3)
        first = recon.render_mesh(meshes[i], VIEWS[0], **kw)
        assert tuple(first.image.shape) == (40, 24, 3)
        for k in range(3):
            assert equal_bits(shared[i][k], alone[k]) and equal_bits(per_mesh[i][k], alone[k]), (i, k)
            assert equal_bits(first[k], alone[k][0]), (i, k)
        assert (alone.face >= 0).sum() > 100
        unclipped = recon.render_mesh(meshes[i], VIEWS, res=(40, 24), shade="normals", projection="perspective",
                                      nearest="min")
        assert not equal_bits(unclipped.face, alone.face)


def on_dirty_arena(ops, byte, op):
    """``op()`` on a private stream whose scratch arena is one block of cases.ARENA_BYTES or more, every byte of it
    ``byte`` (test_scratch_residue_gpu's helper), asserting that ``op`` worked inside that block.  The block is filled
    with zeros before it goes back to the driver, so that no later test finds 0xFF (a NaN) in fresh memory."""
    dev = torch.device(DEV)
    torch.cuda.synchronize(dev)  # the inputs were made on the default stream
    stream = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(stream):
            block = ops.scratch_fill(dev, cases.ARENA_BYTES, byte)
            before = ops.memory_stats(dev)
            out = op()
            after = ops.memory_stats(dev)
            assert ops.scratch_fill(dev, 0, 0x00) == block
        stream.synchronize()
    finally:
        ops.stream_release(stream)
    assert block >= cases.ARENA_BYTES, block
    assert (after["arena_bytes"], after["arenas"]) == (before["arena_bytes"], before["arenas"]), \
        "the stage left the filled block: %s -> %s" % (before, after)
    return out


@pytest.mark.parametrize("byte", [0xFF, 0x5A], ids=["0xFF", "0x5A"])
def test_dirty_arena(ops, body33, byte):
    """The same picture whatever the scratch arena held: the camera-space vertices, like the snapped ones, are written
    for every vertex a face may name before a face reads them."""
    b = body33
    want = body_reference(b, "turned", (40, 24), "min", True)[1]
    pair = [b["verts"], b["verts"].clone()], [b["faces"], b["faces"]], [b["counts"], b["counts"]]
    attrs = [b["seeded"], b["seeded"]]

    def op():
        return ops.mesh_render_raw_batch(*pair, attrs, [VIEWS.flip(0)] * 2, (40, 24), "perspective", "min",
                                         channel_major=True, background=0.25, near=b["near"]["turned"],
                                         perspective_correct=True, **PREDS)

    for got in on_dirty_arena(ops, byte, op):
        assert_same([t[0] for t in got], want)


# ---- refusals ---------------------------------------------------------------------------------------------------------

class ClipEnv(Env):
    """A well-formed call of both clipped entry points on real buffers; every test changes one argument."""
    ORDER = {
        "mp_mesh_render_clip": "verts max_v faces max_f counts attr ch_major calib proj nearest h w scale bias lo hi bg "
                               "image depth face near flags stream",
        "mp_mesh_render_clip_batch": "n verts max_v faces max_f counts attr ch_major n_views calib proj nearest h w "
                                     "scale bias lo hi bg image depth face near flags stream",
    }

    def args(self, name):
        a = super().args(name)
        a.update(proj=1, near=0.5, flags=0)
        return a


@pytest.fixture(scope="module")
def env():
    return ClipEnv()


ENTRIES = ["mp_mesh_render_clip", "mp_mesh_render_clip_batch"]
REFUSED = [
    ("near", dict(near=0.0), ARG), ("near", dict(near=-1.0), ARG), ("near", dict(near=INF), ARG),
    ("near", dict(near=-INF), ARG), ("near", dict(near=math.nan), ARG),
    ("flags", dict(flags=2), ARG), ("flags", dict(flags=3), ARG), ("flags", dict(flags=-1), ARG),
    ("projection", dict(proj=0), ARG), ("projection", dict(proj=2), ARG), ("projection", dict(proj=-1), ARG),
    ("h", dict(h=0), ARG), ("h", dict(h=4097), ARG), ("w", dict(w=0), ARG), ("w", dict(w=4097), ARG),
    ("nearest", dict(nearest=2), ARG), ("nearest", dict(nearest=-1), ARG),
    ("no output", dict(image=None, depth=None, face=None), ARG),
    ("image without attr", dict(attr=None), ARG),
    ("capacity", dict(max_v=2 ** 31 // 3 + 1), UNSUPPORTED), ("capacity", dict(max_f=2 ** 31 // 3 + 1), UNSUPPORTED),
]


@pytest.mark.parametrize("name", ENTRIES)
def test_a_well_formed_call_is_accepted(env, name):
    for changed in ({}, dict(flags=1), dict(attr=None, image=None), dict(depth=None, face=None)):
        rc, msg = env.call(name, **changed)
        assert rc == OK, msg
    torch.cuda.synchronize()
    written = env.image[0, 0] if name == "mp_mesh_render_clip" else env.image
    assert (written == 1.0).all()  # counts {0, 0}: pure background


@pytest.mark.parametrize("what,changed,code", REFUSED, ids=[r[0] + str(i) for i, r in enumerate(REFUSED)])
@pytest.mark.parametrize("name", ENTRIES)
def test_refusals(env, name, what, changed, code):
    env.image.fill_(7.0)
    rc, msg = env.call(name, **changed)
    assert rc == code, (what, msg)
    assert msg.startswith(name + ":"), msg
    torch.cuda.synchronize()
    assert (env.image == 7.0).all()  # nothing was launched
    rc, msg = env.call(name)  # and the context is as usable as before
    assert rc == OK, msg
    torch.cuda.synchronize()
    assert (env.image[0, 0] == 1.0).all()


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
    assert env.call(name)[0] == OK


def test_image_slots_per_call(env):
    for n, n_views in ((0, 1), (1, 0), (33, 1), (1, 33), (2, 17), (-1, 1)):
        many = (lambda t: (ctypes.c_void_p * max(n, 1))(*([t[0].data_ptr()] * max(n, 1))))  # noqa: E731
        rc, msg = env.call("mp_mesh_render_clip_batch", n=n, n_views=n_views, verts=many(env.verts),
                           faces=many(env.faces), counts=many(env.counts), attr=many(env.attr), image=many(env.image),
                           depth=many(env.depth), face=many(env.face))
        assert rc == ARG and msg.startswith("mp_mesh_render_clip_batch:"), (n, n_views, msg)


def test_python_layer_refusals(ops, recon, body33):
    b = body33
    eye = torch.eye(4)
    good = (b["verts"], b["faces"], b["counts"], b["normals"], eye, 16)
    with pytest.raises(ValueError, match="perspective_correct needs near"):
        ops.mesh_render_raw(*good, projection="perspective", perspective_correct=True)
    with pytest.raises(ValueError, match="perspective cameras only"):
        ops.mesh_render_raw(*good, near=0.5)
    with pytest.raises(ValueError, match="perspective cameras only"):
        ops.mesh_render_raw_batch([b["verts"]], [b["faces"]], [b["counts"]], None, [eye], 16, "orthogonal", near=0.5)
    for near in (0.0, -1.0, INF, math.nan):
        with pytest.raises(ValueError, match="near must be"):
            ops.mesh_render_raw(*good, projection="perspective", near=near)
    mesh = recon.Mesh(b["verts"][:b["nv"]], b["faces"][:b["nf"]], b["normals"][:b["nv"]], None)
    with pytest.raises(ValueError, match="perspective_correct needs near"):
        recon.render_mesh(mesh, eye, res=16, shade="normals", projection="perspective", perspective_correct=True)
    with pytest.raises(ValueError, match="perspective cameras only"):
        recon.render_mesh(mesh, eye, res=16, shade="normals", near=0.5)
    with pytest.raises(ValueError, match="perspective cameras only"):
        recon.render_mesh_many([None, None], eye, res=16, shade="normals", near=0.5)
    out = recon.render_mesh(mesh, CAMERAS["front"], res=16, shade="normals", projection="perspective", nearest="min",
                            near=b["near"]["front"], perspective_correct=True)
    assert out.image.shape == (16, 16, 3) and (out.face >= 0).any()
