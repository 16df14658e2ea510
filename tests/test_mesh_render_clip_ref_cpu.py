"""The clipped rasteriser's definition itself (include/monoport_hip.h, mp_mesh_render_clip), pinned on its numpy
restatement tests/mesh_render_clip_ref.py: it is the unclipped definition where nothing is cut, the cut leaves no crack
and no doubly covered centre, and the perspective-correct form reproduces a field that is linear in space.  No GPU."""
import numpy as np
import pytest

import mesh_render_clip_ref as clip
import mesh_render_ref as ref

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_nothing_cut_is_the_unclipped_definition():
    rng = np.random.RandomState(11)
    n = 120
    cam = np.concatenate([rng.uniform(-1.6, 1.6, (3 * n, 2)), rng.uniform(1.0, 3.0, (3 * n, 1))], 1).astype(np.float32)
    cam[:, :2] *= cam[:, 2:3] * rng.uniform(0.05, 1.0, (3 * n, 1)).astype(np.float32)
    faces = np.arange(3 * n).reshape(n, 3)
    attr = rng.standard_normal((3 * n, 3)).astype(np.float32)
    for (h, w), nearest in (((40, 24), "min"), ((33, 33), "max")):
        got = clip.render(cam, faces, h, w, 0.5, attr=attr, nearest=nearest, scale=0.5, bias=0.5)
        want = ref.render(clip.project(cam), faces, h, w, attr=attr, nearest=nearest, scale=0.5, bias=0.5)
        assert (got.kind == 3).all() and (want.face >= 0).sum() > 100
        assert np.array_equal(got.face, want.face) and np.array_equal(got.cover, want.cover)
        assert np.array_equal(bits(got.depth), bits(want.depth)) and np.array_equal(bits(got.image), bits(want.image))
        assert not got.both.any()


def octahedron(levels):
    """The unit octahedron subdivided ``levels`` times onto the unit sphere: a closed mesh of 8 * 4^levels faces whose
    equator vertices have z == 0 exactly."""
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    verts = [np.array(v, np.float64) for v in verts]
    for _ in range(levels):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[key[0]] + verts[key[1]]
                verts.append(m / np.sqrt((m * m).sum()))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = out
    return np.array(verts), np.array(faces)


# (levels, sphere centre, radius, focal scale of x and y, near, (H, W), some covered centres are covered twice)
SPHERES = [
    (3, (0.0, 0.0, 2.0), 1.0, 1.0, 1.7, (48, 40), False),
    (4, (0.1, -0.05, 2.0), 1.0, 1.0, 2.0, (32, 32), False),   # the equator's vertices lie ON the plane: inside
    (3, (0.9, 0.3, 2.0), 1.0, 1.5, 1.6, (65, 33), True),      # the cap leaves the picture and covers part of the body
    (3, (-0.3, 0.4, 1.5), 1.2, 1.0, 0.9, (40, 24), False),
    (4, (0.0, 0.0, 2.0), 1.0, 1.0, 1.05, (66, 66), True),     # a small cap in the middle of the body
    (3, (0.2, 0.1, 2.0), 1.0, 1.0, 2.5, (50, 50), False),     # the plane behind the centre: the far bowl alone
]


@pytest.mark.parametrize("levels,centre,radius,focal,near,size,partial", SPHERES,
                         ids=["%dx%d" % s[5] for s in SPHERES])
def test_the_cut_leaves_no_crack(levels, centre, radius, focal, near, size, partial):
    """What is drawn of a closed mesh is a surface whose border is the loop of cut segments, so the centres covered an
    odd number of times are exactly those inside the even-odd fill of that loop -- evaluated in the snapped integers
    with the same top-left rule, as the parity of the fan of triangles from the snapped point (0, 0) to each segment."""
    verts, faces = octahedron(levels)
    assert len(faces) == 8 * 4 ** levels
    cam = verts * radius + np.array(centre)
    cam[:, :2] *= focal
    cam = cam.astype(np.float32)
    h, w = size
    out = clip.render(cam, faces, h, w, near)
    assert all((out.kind == k).sum() >= 8 for k in (0, 1, 2, 3))
    if near == centre[2]:
        assert (cam[:, 2] == F32(near)).sum() >= 16
    origin = clip.Vert(0, 0, F32(1), -1, -1, F32(0))
    fill = np.zeros((h, w), np.int64)
    segments = clip.cut_segments(cam, faces, h, w, near)
    assert len(segments) == ((out.kind == 1) | (out.kind == 2)).sum()
    for p, q in segments:
        fill += clip.covered(clip._tri(origin, p, q, h, w), h, w)
    odd = out.cover % 2 == 1
    assert np.array_equal(odd, fill % 2 == 1)
    assert odd.sum() > 100 and not out.both.any()
    covered = out.cover > 0
    assert np.array_equal(out.face >= 0, covered)
    assert (not odd[covered].all()) == partial  # the fill is then a proper part of what is covered


def test_quad_whose_diagonal_crosses_the_plane_is_covered_once():
    """Two faces sharing the diagonal V0-V2, which the plane cuts: the cut of the diagonal is the same bits in both, so
    every centre of the clipped quad is covered exactly once."""
    quad = np.array([[-1.9, -1.4, 3.0], [1.7, -1.6, 2.6], [0.9, 0.8, 0.7], [-2.7, 1.0, 1.1]])  # planar: V3 = V0 + V2 - V1
    near = 1.5
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    poly = []  # the quad clipped at the plane, in float64 (Sutherland-Hodgman)
    for k in range(4):
        a, b = quad[k], quad[(k + 1) % 4]
        if a[2] >= near:
            poly.append(a)
        if (a[2] >= near) != (b[2] >= near):
            poly.append(a + (near - a[2]) / (b[2] - a[2]) * (b - a))
    poly = np.array(poly)
    for h, w in ((40, 24), (64, 64)):
        out = clip.render(quad.astype(np.float32), faces, h, w, near)
        assert sorted(out.kind) == [1, 2] and out.cover.max() == 1 and not out.both.any()
        pix = (poly[:, :2] / poly[:, 2:3] + 1.0) * 0.5 * np.array([h, w])
        ci, cj = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        nxt = np.roll(pix, -1, 0)
        turn = np.sign((pix[:, 0] * nxt[:, 1] - pix[:, 1] * nxt[:, 0]).sum())  # the polygon's orientation
        dist = np.full((h, w), np.inf)  # signed distance to the convex polygon's border, in pixels (inside > 0)
        for a, b in zip(pix, nxt):
            d = b - a
            dist = np.minimum(dist, turn * (d[0] * (cj - a[1]) - d[1] * (ci - a[0])) / np.hypot(*d))
        # snapping moves a vertex by at most 1/512 pixel: 1/64 is far outside that
        assert (out.cover[dist > 1 / 64] == 1).all() and (out.cover[dist < -1 / 64] == 0).all()
        assert (out.cover == 1).sum() > 80


def test_perspective_correct_reproduces_a_linear_field():
    """A planar quad tilted in depth (z = 3 at one end, 1 at the other, the plane at 2 cuts it) that carries a field
    linear in space.  Its vertices and its cuts (all at t = 1/2) project onto the 1/256 pixel grid exactly, so the
    picture differs from the ray-plane value by f32 rounding alone."""
    A, B = np.array([-1.5, -2.25, 3.0]), np.array([1.5, -2.25, 3.0])
    d = np.array([0.5, 3.5, -2.0])
    quad = np.array([A, B, B + d, A + d])
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    lin = np.array([[0.3, -0.2, 0.25], [-0.15, 0.1, 0.4], [0.2, 0.3, -0.1]])
    offset = np.array([0.1, -0.3, 0.5])
    attr = (quad @ lin.T + offset).astype(np.float32)
    h = w = 64
    near = 2.0
    normal = np.cross(B - A, d)
    ci, cj = np.meshgrid((np.arange(h) + 0.5) * 2 / h - 1, (np.arange(w) + 0.5) * 2 / w - 1, indexing="ij")
    depth = (normal @ A) / (normal[0] * ci + normal[1] * cj + normal[2])  # the ray (x, y, 1) z meets the plane
    points = np.stack([ci * depth, cj * depth, depth], -1)
    want = points @ lin.T + offset
    out = clip.render(quad.astype(np.float32), faces, h, w, near, perspective_correct=True, attr=attr)
    hit = out.face >= 0
    assert hit.sum() > 500 and sorted(out.kind) == [1, 2] and out.cover.max() == 1
    assert (depth[hit] >= near - 1e-6).all()
    assert np.abs(out.image[hit] - want[hit]).max() < 1e-5
    assert (np.abs(out.depth[hit] - depth[hit]) / depth[hit]).max() < 1e-5
    affine = clip.render(quad.astype(np.float32), faces, h, w, near, perspective_correct=False, attr=attr)
    assert np.array_equal(affine.face, out.face)
    assert np.abs(affine.image[hit] - want[hit]).max() > 1e-2
