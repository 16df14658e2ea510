"""The definition of the mesh rasteriser itself (include/monoport_hip.h, mp_mesh_render), pinned on its numpy
restatement tests/mesh_render_ref.py: watertight coverage under the top-left rule, closed meshes covering every pixel
centre an even number of times, the silhouette of a marching-cubes mesh against the occupied columns of its volume,
depth order and ties, and the faces the definition skips.  No GPU."""
import numpy as np
import pytest

import mesh_render_ref as ref
from monoport_amd import synthetic as syn

VOLUMES = {"sphere33": lambda: syn.sphere_volume(33), "blob33": lambda: syn.blob_volume(33, 5),
           "blob17": lambda: syn.blob_volume(17, 3)}


@pytest.fixture(scope="module")
def meshes(oracle):
    """name -> (volume, verts, faces) of the oracle's marching cubes; the identity camera projects verts to
    themselves."""
    out = {}
    for name, make in VOLUMES.items():
        vol = make()
        v, f = oracle.marching_cubes(vol, 0.5)[:2]
        out[name] = (vol, np.asarray(v, np.float32), np.asarray(f, np.int32))
    return out


def polygon(n=12, centre=(12.1, 11.7), radius=9.0):
    ang = 0.3 + 2.0 * np.pi * np.arange(n) / n
    rim = np.stack([centre[0] + radius * np.cos(ang), centre[1] + radius * np.sin(ang)], 1)
    return np.concatenate([[[centre[0] + 1.3, centre[1] - 0.8]], rim])  # vertex 0: an inner point, 1..n: the rim


def test_fan_is_watertight_and_equals_the_other_triangulation():
    n, size = 12, 24
    xyz = ref.to_ndc(polygon(n), size, size)
    fan = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)])
    fan[1::2] = fan[1::2][:, [0, 2, 1]]  # mixed windings
    fan[2::3] = fan[2::3][:, [1, 2, 0]]
    from_rim = np.array([[1, 1 + k, 2 + k] for k in range(1, n - 1)])
    from_rim[::2] = from_rim[::2][:, [2, 1, 0]]
    a = ref.render(xyz, fan, size, size)
    b = ref.render(xyz, from_rim, size, size)
    assert a.cover.max() == 1 and b.cover.max() == 1  # no centre is covered twice, on shared edges included
    assert np.array_equal(a.cover, b.cover)           # ... and none on them is missed
    assert 200 < a.cover.sum() < 3.1416 * 81          # a 12-gon of radius 9: ~243 pixels


def test_square_on_pixel_centres_covers_16():
    size = 8
    corners = np.array([[2.5, 2.5], [6.5, 2.5], [6.5, 6.5], [2.5, 6.5]])  # the centres of pixels 2 and 6
    xyz = ref.to_ndc(corners, size, size)
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 2, 3]], [[1, 2, 3], [3, 0, 1]]):
        r = ref.render(xyz, np.array(faces), size, size)
        assert r.cover.max() == 1 and r.cover.sum() == 16
        # the top-left rule keeps the edges through the centres of row / column 2 and drops those of 6
        assert np.array_equal(np.argwhere(r.cover), np.argwhere(np.pad(np.ones((4, 4), int), ((2, 2), (2, 2)))))


@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_closed_mesh_covers_every_centre_an_even_number_of_times(meshes, name):
    vol, v, f = meshes[name]
    r = vol.shape[0]
    for size in (r, 2 * r, r - 5):
        cover = ref.render(v, f, size, size).cover
        assert cover.max() >= 2
        assert (cover % 2 == 0).all(), (name, size, int((cover % 2).sum()))


@pytest.mark.parametrize("name", ["blob33", "blob17"])
def test_silhouette_equals_the_occupied_columns(meshes, name):
    vol, v, f = meshes[name]
    r = vol.shape[0]
    got = ref.render(v, f, r, r)
    want = (vol > 0.5).any(axis=0).T  # [x, y]: x runs along the first image index
    assert want.sum() > 40
    assert np.array_equal(got.cover > 0, want)
    assert np.array_equal(got.face >= 0, want)


def two_triangles(z_first, z_second):
    """Two overlapping triangles on a 16 x 16 image, each at a constant depth."""
    pix = np.array([[1, 1, z_first], [14, 2, z_first], [3, 14, z_first],
                    [2, 3, z_second], [15, 6, z_second], [8, 15, z_second]], np.float64)
    return ref.to_ndc(pix, 16, 16), np.array([[0, 1, 2], [3, 4, 5]])


@pytest.mark.parametrize("z", [(0.25, -0.5), (-0.5, 0.25), (-0.0, 0.0), (3.0, 1.0)])
def test_the_nearer_fragment_wins(z):
    xyz, faces = two_triangles(*z)
    both = ref.render(xyz, faces, 16, 16).cover == 2
    assert both.sum() > 20
    for nearest, pick in (("max", max), ("min", min)):
        r = ref.render(xyz, faces, 16, 16, nearest=nearest)
        want = pick(z)
        winner = z.index(want) if z[0] != z[1] else 0
        if set(z) == {0.0} and np.signbit(z[0]) != np.signbit(z[1]):  # -0 < +0 in the key's order
            winner = [np.signbit(v) for v in z].index(nearest == "min")
        assert (r.face[both] == winner).all(), nearest
        # a constant depth is interpolated as (w0 + w1 + w2) * z with three roundings of the weights, two of the sum
        assert np.abs(r.depth[both] - np.float32(z[winner])).max() <= 4 * 2.0 ** -24 * abs(z[winner]), nearest


def test_equal_depth_goes_to_the_smaller_face_index():
    xyz, faces = two_triangles(0.0, 0.0)  # w * 0 is exactly +0 for every weight: the depths tie bit for bit
    both = ref.render(xyz, faces, 16, 16).cover == 2
    for nearest in ("max", "min"):
        assert (ref.render(xyz, faces, 16, 16, nearest=nearest).face[both] == 0).all()
        assert (ref.render(xyz, faces[::-1], 16, 16, nearest=nearest).face[both] == 0).all()
    xyz, faces = two_triangles(0.3, -0.7)  # the same face three times over: the same depth bits at any slope
    xyz[:3, 2] = [0.3, -0.2, 0.9]
    for nearest in ("max", "min"):
        r = ref.render(xyz, faces[[1, 0, 0, 0]], 16, 16, nearest=nearest)
        alone = ref.render(xyz, faces[[1, 0]], 16, 16, nearest=nearest)
        assert set(np.unique(r.face)) == {-1, 0, 1} and np.array_equal(r.face, alone.face)


def test_orderable_is_monotone():
    vals = np.array([-np.inf, -3.0e38, -1.5, -1e-30, -1e-45, -0.0, 0.0, 1e-45, 1e-30, 0.75, 2.0, 3.0e38, np.inf],
                    np.float32)
    keys = ref.orderable(vals.view(np.uint32)).astype(np.int64)
    assert (np.diff(keys) > 0).all()
    assert keys.min() > 0  # no depth collides with the cleared key
    rng = np.random.RandomState(7)
    a = (rng.standard_normal(4000) * 10.0 ** rng.randint(-30, 30, 4000)).astype(np.float32)
    order = np.argsort(ref.orderable(a.view(np.uint32)), kind="stable")
    assert (np.diff(a[order]) >= 0).all()


def base_scene():
    rng = np.random.RandomState(11)
    pix = np.concatenate([rng.uniform(-2, 22, (40, 2)), rng.uniform(-1, 1, (40, 1))], 1)
    faces = rng.randint(0, 40, (30, 3))
    attr = rng.standard_normal((40, 3)).astype(np.float32)
    return ref.to_ndc(pix, 20, 20), faces, attr


SKIPPED = {
    "zero area": (None, [[5, 5, 9], [7, 7, 7]]),
    "collinear": ([[-0.5, -0.5, 0.0], [0.0, 0.0, 0.0], [0.5, 0.5, 0.0]], [[40, 41, 42]]),
    "NaN vertex": ([[np.nan, 0.0, 0.0], [0.0, 0.0, np.nan], [0.0, np.inf, 0.0]], [[0, 1, 40], [2, 41, 3], [4, 5, 42]]),
    "beyond the guard": ([[1.0e6, 0.0, 0.0], [0.0, -1.0e6, 0.0]], [[0, 1, 40], [2, 41, 3]]),
    "index out of range": (None, [[0, 1, 40], [-1, 2, 3], [4, 2 ** 31 - 1, 5]]),
}


@pytest.mark.parametrize("what", sorted(SKIPPED))
def test_skipped_faces_change_nothing(what):
    xyz, faces, attr = base_scene()
    want = ref.render(xyz, faces, 20, 20, attr=attr, scale=0.5, bias=0.5)
    assert (want.face >= 0).sum() > 100
    more_v, more_f = SKIPPED[what]
    if more_v is not None:
        xyz = np.concatenate([xyz, np.array(more_v, np.float32)])
        attr = np.concatenate([attr, np.ones((len(more_v), 3), np.float32)])
    got = ref.render(xyz, np.concatenate([faces, np.array(more_f)]), 20, 20, attr=attr, scale=0.5, bias=0.5)
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True), what
