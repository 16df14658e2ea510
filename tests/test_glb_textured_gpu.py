"""mp_mesh_glb_textured / _batch (csrc/glb.hip), recon.bake_texture and recon.encode_glb(Glb(texture=...)) on the GPU.
The device's file equals the numpy restatement (tests/glb_texture_ref.py) BYTE FOR BYTE -- with and without normals, at
the exact capacity and one byte short, with code 2 for an atlas too small and for an overflowed image, in aligned and
odd rows, with an image whose length is no multiple of 4, for empty meshes, over a dirty ``out`` --; and, independently
of every restatement, a file baked from an affine colour field reads back by the glTF specification and Pillow to that
field at random surface points, to half an 8-bit step.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import atlas_cases as cases
import atlas_ref
import glb_cases
import glb_ref
import glb_texture_ref as ref
import png_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, -1, -3
F = np.float32
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def on_device(c):
    return t(c.verts), t(c.faces), torch.tensor(c.counts, dtype=torch.int32).to(DEV), t(c.normals)


_PNG = {}


def png_of(case):
    """The restatement's PNG of a picture of the case's atlas: the affine colour at covered texels, 0.5 elsewhere."""
    if case.name not in _PNG:
        face_id, position, _ = cases.restated(case)
        with np.errstate(all="ignore"):
            image = np.where((face_id >= 0)[..., None], cases.affine_colour(position) * 0.5 + 0.5, 0.5).astype(F)
        _PNG[case.name] = png_ref.encode(image, "rgb8")[0]
    return _PNG[case.name]


def png_buffers(files, capacity=None, overflowed=()):
    """(png [n,capacity] uint8, png_info [n,2] int32) on the device, as mp_picture_png leaves them."""
    capacity = capacity or max(len(f) for f in files) + 5
    rows = np.full((len(files), capacity), 0xEE, np.uint8)
    info = np.zeros((len(files), 2), np.int32)
    for i, f in enumerate(files):
        if i in overflowed:
            info[i] = (len(f), 1)
        else:
            rows[i, :len(f)] = np.frombuffer(f, np.uint8)
            info[i] = (len(f), 0)
    return t(rows), t(info)


def same(got, want, what):
    if got != want:
        first = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
        raise AssertionError("%s: byte %d of %d (got %d) differs" % (what, first, len(want), len(got)))


def device_file(ops, c, normals, png, **kw):
    v, f, n, nrm = on_device(c)
    rows, info = png_buffers([png])
    out, got = ops.mesh_glb_textured_raw(v, f, n, c.size, c.cell, rows, info, nrm if normals else None, None, c.b_min,
                                         c.b_max, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), got.cpu().numpy()


FILE_CASES = [c for c in cases.cases() if c.name != "sphere17_64_4" and not c.name.startswith("full+1")]


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("case", FILE_CASES, ids=lambda c: c.name)
def test_files_equal_the_restatement(ops, case, normals):
    png = png_of(case)
    want, info = ref.encode(case.verts, case.faces, case.size, case.cell, png, case.counts,
                            case.normals if normals else None, case.b_min, case.b_max)
    out, got = device_file(ops, case, normals, png)
    assert tuple(got[0]) == info == (len(want), 0), (case.name, got[0], info)
    same(out[0, :len(want)].tobytes(), want, case.name)
    nv, nf = atlas_ref.counts_of(case.verts, case.faces, case.counts)
    assert len(want) == ops.glb_textured_bytes(nf, len(png), normals) == ref.file_bytes(nf, len(png), normals)
    assert len(want) <= ops.glb_textured_max_bytes(len(case.faces), case.size, normals) \
        == ref.max_bytes(len(case.faces), case.size, normals)


def test_image_lengths_of_every_remainder(ops):
    """An image of 4 k, 4 k + 1, 4 k + 2 and 4 k + 3 bytes: the padding of the BIN chunk."""
    seen = set()
    for case in FILE_CASES:
        png = png_of(case)
        seen.add(len(png) % 4)
    assert seen == {0, 1, 2, 3}, seen


def batch_of_three():
    frames = [cases._from_glb(glb_cases.random_mesh("tex_batch_%d" % k, 90, 61, 60 + k, glb_cases.SKEW, counts=n), 64, 8)
              for k, n in enumerate(((90, 61), (0, 0), (40, 22)))]
    return frames, [png_of(c) for c in frames]


def device_batch(ops, frames, pngs, overflowed=(), size=64, cell=8, **kw):
    parts = [on_device(c) for c in frames]
    rows, info = png_buffers(pngs, overflowed=overflowed)
    out, got = ops.mesh_glb_textured_raw_batch(*[[p[k] for p in parts] for k in range(3)], size, cell, rows, info,
                                               [p[3] for p in parts], None, frames[0].b_min, frames[0].b_max, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), got.cpu().numpy()


def restated(frames, pngs, **kw):
    return [ref.encode(c.verts, c.faces, c.size, c.cell, p, c.counts, c.normals, c.b_min, c.b_max, **kw)
            for c, p in zip(frames, pngs)]


def test_batched_equals_per_frame_and_runs_repeat(ops):
    frames, pngs = batch_of_three()
    want = restated(frames, pngs)
    runs = [device_batch(ops, frames, pngs) for _ in range(2)]
    assert np.array_equal(runs[0][1], runs[1][1])
    for i, (c, (data, info)) in enumerate(zip(frames, want)):
        assert tuple(runs[0][1][i]) == info
        for out, _ in runs:
            same(out[i, :len(data)].tobytes(), data, "batched %d" % i)
        alone, got = device_file(ops, c, True, pngs[i])
        assert tuple(got[0]) == info and alone[0, :len(data)].tobytes() == data
    assert len(want[1][0]) == glb_ref.MIN_BYTES


def test_capacity_exact_and_one_byte_short_aligned_and_odd_rows(ops):
    frames, pngs = batch_of_three()
    want = [w[0] for w in restated(frames, pngs)]
    sizes = [len(b) for b in want]
    assert sizes[1] < sizes[2] < sizes[0]
    guard = 8192
    for cap in (sizes[2], sizes[2] - 1, sizes[0], sizes[0] - 1, sizes[0] + 3, sizes[0] + 1, glb_ref.MIN_BYTES):
        buf = torch.full((3 * cap + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
        out, info = device_batch(ops, frames, pngs, out=buf[:3 * cap].view(3, cap))
        whole = buf.cpu().numpy()
        assert (whole[3 * cap:] == SENTINEL).all()
        for i in range(3):
            fits = sizes[i] <= cap
            assert tuple(info[i]) == (sizes[i], 0 if fits else 1), (cap, i, info[i])
            if fits:
                assert out[i, :sizes[i]].tobytes() == want[i] and (out[i, sizes[i]:] == SENTINEL).all(), (cap, i)
            else:
                assert (out[i] == SENTINEL).all(), (cap, i)
    # a second call at the reported size gives the bytes a sufficient capacity gives
    out, info = device_file(ops, frames[0], True, pngs[0], capacity=sizes[0])
    assert tuple(info[0]) == (sizes[0], 0) and out[0].tobytes() == want[0]


def test_code_2(ops):
    """An atlas too small for the mesh, and an image that itself overflowed: nothing is written, the others are."""
    frames, pngs = batch_of_three()
    want = restated(frames, pngs)
    cap = len(want[0][0]) + 7
    for overflowed in ((0,), (2,), (0, 1, 2)):
        buf = torch.full((3, cap), SENTINEL, dtype=torch.uint8, device=DEV)
        out, info = device_batch(ops, frames, pngs, overflowed=overflowed, out=buf)
        for i in range(3):
            if i in overflowed and i != 1:  # the empty frame's image is not looked at
                assert tuple(info[i]) == (0, 2) and (out[i] == SENTINEL).all(), (overflowed, i, info[i])
                assert ref.encode(frames[i].verts, frames[i].faces, 64, 8, pngs[i], frames[i].counts, frames[i].normals,
                                  frames[i].b_min, frames[i].b_max, png_overflowed=True) == (None, (0, 2))
            else:
                assert tuple(info[i]) == want[i][1] and out[i, :len(want[i][0])].tobytes() == want[i][0]
    # 61 faces in an atlas of 2 * 1^2 (size 64, cell 64): frames 0 and 2 do not fit, the empty one does
    buf = torch.full((3, cap), SENTINEL, dtype=torch.uint8, device=DEV)
    out, info = device_batch(ops, frames, pngs, size=64, cell=64, out=buf)
    assert [tuple(r) for r in info] == [(0, 2), (glb_ref.MIN_BYTES, 0), (0, 2)]
    assert (out[0] == SENTINEL).all() and (out[2] == SENTINEL).all()
    # a length outside MP_PNG_MIN_BYTES..png_capacity is no image either
    v, f, n, nrm = on_device(frames[0])
    rows, pinfo = png_buffers([pngs[0]])
    for bad in (56, 0, -1, rows.shape[1] + 1):
        pinfo[0, 0] = bad
        _, got = ops.mesh_glb_textured_raw(v, f, n, 64, 8, rows, pinfo, nrm, None, frames[0].b_min, frames[0].b_max)
        assert got.cpu().tolist() == [[0, 2]], bad
    small = cases.sphere_case(17, 64, 4)
    out, got = device_file(ops, small, True, png_of(cases.hand_made(1)))
    assert tuple(got[0]) == (0, 2)


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_dirty_out_and_arena(ops, byte):
    for case in (cases.hand_made(3, 64, 5), cases.sphere_case(17, 128, 4), cases._from_glb(glb_cases.small_cases()[13], 64, 8)):
        ops.scratch_fill(DEV, 1 << 20, byte)
        png = png_of(case)
        want, info = ref.encode(case.verts, case.faces, case.size, case.cell, png, case.counts, case.normals, case.b_min,
                                case.b_max)
        out = torch.full((1, len(want) + 9), byte, dtype=torch.uint8, device=DEV)
        got, ginfo = device_file(ops, case, True, png, out=out)
        assert tuple(ginfo[0]) == info and got[0, :len(want)].tobytes() == want and (got[0, len(want):] == byte).all()


def test_refusals(ops):
    frames, pngs = batch_of_three()
    c = frames[0]
    v, f, n, nrm = on_device(c)
    rows, pinfo = png_buffers([pngs[0]])
    with pytest.raises(ValueError, match="COLOR_0"):
        ops.mesh_glb_textured_raw(v, f, n, 64, 8, rows, pinfo, nrm, t(np.zeros((90, 3), F)))
    for bad in (dict(size=100), dict(cell=3), dict(png=rows[0]), dict(png=rows.int()), dict(png=rows[:, :40].contiguous()),
                dict(png_info=pinfo.long()), dict(png_info=pinfo[0]), dict(normals=nrm[:-1]), dict(capacity=99),
                dict(out=torch.zeros((2, 4096), dtype=torch.uint8, device=DEV)),
                dict(info=torch.zeros((1, 2), dtype=torch.int64, device=DEV))):
        kw = dict(size=64, cell=8, png=rows, png_info=pinfo)
        kw.update(bad)
        with pytest.raises(ValueError, match="mesh_glb_textured_raw"):
            ops.mesh_glb_textured_raw(v, f, n, **kw)
    # through the C ABI: colours given, the atlas's sizes, the image's buffers, aliasing
    ctx = ops.get_context(DEV)
    out = torch.full((1, 16384), SENTINEL, dtype=torch.uint8, device=DEV)
    info = torch.full((1, 2), -7, dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    f3 = lambda *x: (ctypes.c_float * 3)(*x)  # noqa: E731

    def call(**k):
        a = dict(verts=v.data_ptr(), max_v=90, faces=f.data_ptr(), max_f=61, counts=n.data_ptr(), normals=nrm.data_ptr(),
                 colors=None, size=64, cell=8, png=rows.data_ptr(), png_cap=rows.shape[1], png_info=pinfo.data_ptr(),
                 b_min=f3(*c.b_min), b_max=f3(*c.b_max), out=out.data_ptr(), cap=16384, info=info.data_ptr())
        a.update(k)
        rc = ctx.lib.mp_mesh_glb_textured(ctx.handle, a["verts"], a["max_v"], a["faces"], a["max_f"], a["counts"],
                                          a["normals"], a["colors"], a["size"], a["cell"], a["png"], a["png_cap"],
                                          a["png_info"], a["b_min"], a["b_max"], a["out"], a["cap"], a["info"], stream)
        return rc, ctx.lib.mp_last_error(ctx.handle).decode()
    nan = float("nan")
    refused = [
        (dict(colors=nrm.data_ptr()), ARG, "COLOR_0"), (dict(size=96), ARG, "atlas_size"), (dict(size=8192), ARG, "atlas_size"),
        (dict(cell=3), ARG, "cell"), (dict(cell=65), ARG, "cell"),
        (dict(png=None), ARG, "bad argument"), (dict(png_info=None), ARG, "bad argument"),
        (dict(png_info=pinfo.data_ptr() + 2), ARG, "bad argument"), (dict(counts=None), ARG, "null buffer"),
        (dict(out=None), ARG, "bad argument"), (dict(info=None), ARG, "bad argument"), (dict(verts=None), ARG, "null buffer"),
        (dict(png_cap=56), ARG, "png_capacity"), (dict(png_cap=2 ** 31 + 1), ARG, "png_capacity"),
        (dict(cap=99), ARG, "capacity"), (dict(cap=2 ** 31 + 1), ARG, "capacity"),
        (dict(b_min=f3(nan, 0, 0)), ARG, "box"), (dict(b_min=f3(5, 0, 0)), ARG, "box"),
        (dict(out=rows.data_ptr() + 3), ARG, "aliases"), (dict(out=pinfo.data_ptr()), ARG, "aliases"),
        (dict(info=rows.data_ptr() + 4), ARG, "aliases"), (dict(info=pinfo.data_ptr()), ARG, "aliases"),
        (dict(out=v.data_ptr() + 1), ARG, "aliases"), (dict(info=f.data_ptr()), ARG, "aliases"),
        (dict(out=info.data_ptr()), ARG, "aliases"),
        (dict(verts=v.data_ptr() + 2), ARG, "misaligned"), (dict(normals=nrm.data_ptr() + 1), ARG, "misaligned"),
        (dict(max_f=2 ** 27), UNSUPPORTED, "2^31"), (dict(max_v=2 ** 30), UNSUPPORTED, "2^31"),
    ]
    for changed, code, word in refused:
        rc, msg = call(**changed)
        assert rc == code and msg.startswith("mp_mesh_glb_textured:") and word in msg, (changed, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((info == -7).all())  # nothing was launched
    assert call()[0] == OK
    torch.cuda.synchronize()
    want = restated(frames[:1], pngs[:1])[0]
    assert tuple(info.cpu().numpy()[0]) == want[1] and out[0, :len(want[0])].cpu().numpy().tobytes() == want[0]
    assert ops.glb_textured_bytes(0, 1234) == glb_ref.MIN_BYTES
    with pytest.raises(ValueError):
        ops.glb_textured_bytes(-1, 10)
    with pytest.raises(ValueError):
        ops.glb_textured_max_bytes(10, 100)


# ---- independently of the restatements ------------------------------------------------------------------------------
def affine_on_device(points):
    """atlas_cases.affine_colour as the ``colors=`` callable: points [3,K] f32 -> raw predictions [3,K] f32."""
    m = torch.tensor(cases.AFFINE[0], dtype=torch.float32, device=points.device)
    b = torch.tensor(cases.AFFINE[1], dtype=torch.float32, device=points.device)
    return (m @ points + b[:, None]).contiguous()


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("case", [cases.hand_made(3, 64, 4), cases.sphere_case(17, 128, 4), cases.sphere_case(17, 256, 5),
                                  cases.sphere_case(33, 256, 4), cases.hand_made(2, 128, 64), cases.sphere_case(17, 256, 8)],
                         ids=lambda c: c.name)
def test_a_viewer_sees_the_colour_field(recon, case, normals):
    """The device's file, read by the specification; its image, decoded by Pillow, looked up bilinearly at the UV of
    random surface points (edges and corners included) is the affine colour at the 3-D point.  In units of one byte
    step = 1 / 255: every texel is within half a step of the field at its own position, a bilinear lookup is a convex
    combination of texels of the face's own, and the field is affine -- so 0.5 / 255, plus 1e-5 for the f32 arithmetic
    of the bake (positions to 6e-8, the colour callable, the paint)."""
    mesh = recon.Mesh(t(case.verts), t(case.faces), t(case.normals) if normals else None, None)
    glb = recon.Glb(normals=normals, texture=recon.Atlas(case.size, case.cell))
    data = recon.encode_glb(mesh, glb, case.b_min, case.b_max, colors=affine_on_device)
    assert isinstance(data, bytes)
    got = ref.read(data)
    nf = len(case.faces)
    assert np.array_equal(got["faces"], np.arange(3 * nf).reshape(nf, 3))  # the faces, corner by corner
    corner = case.faces.reshape(-1)
    assert np.abs(got["positions"] - case.verts[corner].astype(np.float64)).max() <= 0.52 * 2.0 / 65535
    if normals:
        assert np.abs(got["normals"] - case.normals[corner]).max() <= 0.51 / 127
    face, bary, _ = atlas_ref.surface_points(nf, case.size, case.cell, 12, seed=9)
    shown, _ = ref.viewer_colours(got, face, bary)
    point = (case.verts.astype(np.float64)[case.faces[face]] * bary[:, :, None]).sum(axis=1)
    want = cases.affine_colour(point) * 0.5 + 0.5
    err = np.abs(shown - want).max() * 255
    print("%s: %d points, largest colour error %.4f byte steps" % (case.name, len(face), err))
    assert want.min() >= 0 and want.max() <= 1
    assert np.abs(shown - want).max() <= 0.5 / 255 + 1e-5
    # the same file from bake_texture + the restatement's writer: the bake is what encode_glb wrote
    image, face_id = recon.bake_texture(mesh, glb.texture, colors=affine_on_device)
    torch.cuda.synchronize()
    assert np.array_equal(face_id.cpu().numpy(), cases.restated(case)[0])
    assert np.array_equal(ref.decode_png(got["png"]), glb_ref.to_u8(image.cpu().numpy()))


def test_encode_glb_textured_lists_and_refusals(recon):
    """Meshes of different sizes in one call, one of them empty; capacities that overflow; what is refused."""
    made = [cases.hand_made(3, 64, 5), cases.sphere_case(17, 64, 5), cases._from_glb(glb_cases.small_cases()[12], 64, 5)]
    made[1] = made[1]._replace(faces=made[1].faces[:200], counts=(made[1].counts[0], 200))
    meshes = [recon.Mesh(t(c.verts), t(c.faces[:c.counts[1]]), t(c.normals), None) for c in made]
    atlas = recon.Atlas(64, 5)
    glb = recon.Glb(texture=atlas)
    files = recon.encode_glb(meshes, glb, colors=affine_on_device)
    assert len(files) == 3 and len(files[2]) == glb_ref.MIN_BYTES
    for c, data, mesh in zip(made[:2], files[:2], meshes):
        got = ref.read(data)
        image, _ = recon.bake_texture(mesh, atlas, colors=affine_on_device)
        png = png_ref.encode(image.cpu().numpy(), "rgb8")[0]
        assert got["png"] == png
        want, _ = ref.encode(c.verts, c.faces[:c.counts[1]], 64, 5, png, None, c.normals)
        same(data, want, c.name)
    tight = recon.Glb(texture=recon.Atlas(64, 5, png_capacity=200), capacity=len(files[2]) + 8)
    assert recon.encode_glb(meshes, tight, colors=affine_on_device) == files
    assert recon.encode_glb(meshes[0], glb, colors=affine_on_device) == files[0]
    images, faces = recon.bake_texture(meshes, atlas, colors=affine_on_device)
    assert tuple(images.shape) == (3, 64, 64, 3) and tuple(faces.shape) == (3, 64, 64) and int(faces[2].max()) == -1
    assert bool((images[2] == 0.5).all())
    with pytest.raises(ValueError, match="colors=True together with texture"):
        recon.Glb(colors=True, texture=atlas)
    with pytest.raises(ValueError, match="recon.Atlas"):
        recon.Glb(texture=recon.Png())
    for bad in (dict(size=100), dict(cell=3), dict(filter="best"), dict(background=np.inf), dict(png_capacity=10)):
        with pytest.raises(ValueError):
            recon.Atlas(**bad)
    assert atlas.faces == 2 * 12 * 12 and recon.Atlas().faces == 2 * 128 * 128 and recon.Atlas().filter == recon.Png().filter
    with pytest.raises(ValueError, match="holds 288"):
        recon.encode_glb(recon.Mesh(t(cases.sphere(17)[0]), t(cases.sphere(17)[1]), None, None),
                         recon.Glb(normals=False, texture=atlas), colors=affine_on_device)
    with pytest.raises(ValueError, match="one of the two"):
        recon.encode_glb(meshes[0], glb)
    with pytest.raises(ValueError, match="this Glb has none"):
        recon.encode_glb(meshes[0], recon.Glb(colors=False), colors=affine_on_device)
    with pytest.raises(ValueError, match="float32 tensor"):
        recon.bake_texture(meshes[0], atlas, colors=lambda p: p.double())
    # capacity_for accounts for the image and for the atlas's room
    g = recon.Glb(texture=recon.Atlas(128, 8))
    assert g.capacity_for(10 ** 6, 2 * 10 ** 6) == ref.file_bytes(512, recon.Png().capacity_for(128, 128), True)
    assert recon.Glb(capacity=4096, texture=atlas).capacity_for(9, 9) == 4096 and g.colors is False
