"""The texture atlas and the textured .glb on their numpy restatements alone (tests/atlas_ref.py,
tests/glb_texture_ref.py): the layout's ownership property for every cell size, exact and distinct corner UVs, the
position texture as an affine map of the surface, and the restated file read back by the glTF specification and
Pillow.  No GPU, no library."""
import json

import numpy as np
import pytest

import atlas_cases as cases
import atlas_ref as ref
import glb_ref
import glb_texture_ref as tex
import png_ref

F = np.float32
# A viewer's interpolation weights carry f32 rounding: a texel that enters a footprint with less than this weight
# (0.03 of an 8-bit step at full contrast) is not looked at.  It is not a tolerance of the layout.
WEIGHT = 1e-4
# |bilinear lookup of the f32 position texture - the float64 affine map| on the meshes below: measured 5.9e-8 (about
# one f32 step of coordinates below 1: a texel is six f32 operations, each rounded), given 4x margin.
POSITION_BOUND = 2.4e-7


@pytest.mark.parametrize("cell", list(range(4, 17)) + [64])
def test_every_bilinear_footprint_is_owned(cell):
    """For random barycentric points of every face slot, edges and corners included, every texel of the bilinear
    footprint with a weight above WEIGHT belongs to that face."""
    size = 64 if cell <= 16 else 128
    nf = ref.capacity(size, cell)
    slot = ref.texel_faces(size, cell)[0]
    face, _, uv = ref.surface_points(nf, size, cell, 64, seed=cell)
    texels, w = ref.bilinear_footprint(uv, size)
    owner = slot[texels[..., 1], texels[..., 0]]
    bad = (w > WEIGHT) & (owner != face[:, None])
    assert not bad.any(), (cell, int(bad.sum()), face[bad.any(axis=1)][:5])
    # and the cells tile: every slot owns T (T + 1) / 2 or T (T - 1) / 2 texels, the margins none
    g = ref.grid(size, cell)
    count = np.bincount(slot[slot >= 0], minlength=nf)
    assert (count[0::2] == cell * (cell + 1) // 2).all() and (count[1::2] == cell * (cell - 1) // 2).all()
    assert (slot >= 0).sum() == (g * cell) ** 2


@pytest.mark.parametrize("size,cell", [(64, 4), (64, 5), (128, 8), (256, 7), (4096, 64), (4096, 4), (128, 64)])
def test_corner_uvs_are_exact_and_distinct(size, cell):
    nf = min(ref.capacity(size, cell), 20000)
    uv = ref.corner_uvs(nf, size, cell)
    assert uv.dtype == F
    texel = ref.corner_texels(nf, size, cell)
    assert np.array_equal(uv.astype(np.float64) * size - 0.5, texel.astype(np.float64))  # exactly (k + 0.5) / A
    assert texel.min() >= 0 and texel.max() < size
    flat = texel.reshape(-1, 2)
    assert len(np.unique(flat[:, 1] * size + flat[:, 0])) == 3 * nf  # no two corners, of any faces, share a texel
    slot = ref.texel_faces(size, cell)[0]
    assert np.array_equal(slot[texel[..., 1], texel[..., 0]], np.repeat(np.arange(nf)[:, None], 3, 1))
    # a right triangle with the right angle at corner 0 and legs of T - 2 / T - 3 texels
    d1, d2 = texel[:, 1] - texel[:, 0], texel[:, 2] - texel[:, 0]
    leg = cell - 2 - (np.arange(nf) & 1)
    sign = 1 - 2 * (np.arange(nf) & 1)
    assert np.array_equal(d1, np.stack([sign * leg, 0 * leg], 1)) and np.array_equal(d2, np.stack([0 * leg, sign * leg], 1))


@pytest.mark.parametrize("case", [c for c in cases.cases() if c.name.startswith(("sphere", "hand"))],
                         ids=lambda c: c.name)
def test_position_texture_is_the_surface(case):
    """``position`` looked up bilinearly at a surface point's UV is the point: against the float64 affine map."""
    face_id, position, info = cases.restated(case)
    laid = int(info[0])
    face, bary, uv = ref.surface_points(laid, case.size, case.cell, 16, seed=3)
    got = ref.sample_bilinear(position, uv)
    tri = case.verts.astype(np.float64)[case.faces[face]]
    want = (tri * bary[:, :, None]).sum(axis=1)
    err = np.abs(got - want).max()
    print("%s: position error %.3g" % (case.name, err))
    assert err <= POSITION_BOUND
    # corner texels hold the vertices themselves, to the last bit
    texel = ref.corner_texels(laid, case.size, case.cell)
    assert np.array_equal(position[texel[..., 1], texel[..., 0]], case.verts[case.faces[:laid]])


def test_info_and_uncovered_texels():
    for case in cases.cases():
        face_id, position, info = cases.restated(case)
        nv, nf = ref.counts_of(case.verts, case.faces, case.counts)
        assert tuple(info) == (min(nf, ref.capacity(case.size, case.cell)), nf)
        off = face_id < 0
        assert (position[off] == F(0.5)).all()
        assert set(np.unique(face_id[~off])) == set(range(int(info[0])))
    too_small = cases.sphere_case(17, 64, 4)
    info = cases.restated(too_small)[2]
    assert info[1] > info[0] == 512


def _image_of(case):
    """A picture for the atlas of a case: the affine colour painted at covered texels, 0.5 elsewhere."""
    face_id, position, _ = cases.restated(case)
    image = np.where((face_id >= 0)[..., None], cases.affine_colour(position) * 0.5 + 0.5, 0.5).astype(F)
    return image


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("case", [cases.hand_made(1), cases.hand_made(3, 64, 5), cases.sphere_case(17, 128, 4)],
                         ids=lambda c: c.name)
def test_restated_file_reads_by_the_specification(case, normals):
    image = _image_of(case)
    png, size = png_ref.encode(image, "rgb8")
    data, info = tex.encode(case.verts, case.faces, case.size, case.cell, png, case.counts,
                            case.normals if normals else None, case.b_min, case.b_max)
    nf = len(case.faces)
    assert info == (len(data), 0) and len(data) == tex.file_bytes(nf, size, normals) <= tex.max_bytes(nf, case.size, normals)
    got = tex.read(data)
    doc = got["doc"]
    json.dumps(doc)
    assert "indices" not in doc["meshes"][0]["primitives"][0] and "COLOR_0" not in doc["meshes"][0]["primitives"][0]["attributes"]
    assert doc["extensionsRequired"] == ["KHR_mesh_quantization"]
    assert got["png"] == png
    assert np.array_equal(tex.decode_png(got["png"]), glb_ref.to_u8(image))  # Pillow gives the restatement's samples
    corner = case.faces.reshape(-1)
    assert np.abs(got["positions"] - case.verts[corner].astype(np.float64)).max() <= 0.52 * 2.0 / 65535
    assert np.array_equal(got["uv"].astype(F), ref.corner_uvs(nf, case.size, case.cell).reshape(-1, 2))
    if normals:
        assert np.abs(got["normals"] - case.normals[corner]).max() <= 0.51 / 127
    else:
        assert got["normals"] is None
    # what a viewer shows is the colour field at the surface point, to half an 8-bit step
    face, bary, _ = ref.surface_points(nf, case.size, case.cell, 8, seed=5)
    shown, _ = tex.viewer_colours(got, face, bary)
    tri = case.verts.astype(np.float64)[case.faces[face]]
    want = cases.affine_colour((tri * bary[:, :, None]).sum(axis=1)) * 0.5 + 0.5
    assert np.abs(shown - want).max() <= 0.5 / 255 + 1e-5


def test_restated_file_codes():
    case = cases.hand_made(3)
    png, _ = png_ref.encode(_image_of(case), "rgb8")
    args = (case.verts, case.faces, case.size, case.cell, png, case.counts, None, case.b_min, case.b_max)
    data, info = tex.encode(*args)
    assert tex.encode(*args, capacity=len(data))[0] == data
    assert tex.encode(*args, capacity=len(data) - 1) == (None, (len(data), 1))
    assert tex.encode(*args, png_overflowed=True) == (None, (0, 2))
    small = cases.sphere_case(17, 64, 4)
    assert tex.encode(small.verts, small.faces, 64, 4, png) == (None, (0, 2))
    empty, info = tex.encode(case.verts, case.faces, 64, 8, png, (0, 3))
    assert info == (glb_ref.MIN_BYTES, 0) and tex.read(empty) is None
    assert len(data) % 4 == 0
    # the JSON chunk's length is a constant per attribute set, and the BIN data starts at a multiple of 8
    g = glb_ref.Glb(data)
    assert len(g.chunks[0][2]) == tex.json_len(False) and g.chunks[1][1] % 8 == 0
