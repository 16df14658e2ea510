"""tests/shadow_ref.py, the numpy restatement of mp_picture_shadow (include/monoport_hip.h), held to hand-made cases and
to the geometry of a sphere's shadow on a floor, and the host logic of recon.Light / Scene(light=).  No GPU."""
import numpy as np
import pytest

import mesh_render_ref as render_ref
import shadow_cases as cases
import shadow_ref as ref
from oracle import pifu_oracle as oracle

F = np.float32
IDENTITY = np.eye(4, dtype=F)[:3]
NEAREST = {"min": ref.MIN_Z, "max": ref.MAX_Z}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def at_texel(i, j, hs, ws, z=1.0, fi=0.0, fj=0.0):
    """The point whose map coordinates under the identity light are (i + fi, j + fj): exact for power-of-two sizes."""
    return [(2.0 * (i + fi) + 1.0) / hs - 1.0, (2.0 * (j + fj) + 1.0) / ws - 1.0, z]


def one(position, map_depth, map_face, **kw):
    position = np.asarray([position], F)
    return ref.shade(position, np.zeros(1, np.int32), np.asarray(map_depth, F), np.asarray(map_face, np.int32),
                     IDENTITY, **kw)[0]


# ---- one tap --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nearest", ["min", "max"])
def test_truth_table_of_one_tap(nearest):
    mode, sign = NEAREST[nearest], (1.0 if nearest == "min" else -1.0)
    z = F(0.5)
    i = j = np.zeros(1, np.int64)

    def occ(depth, face=0, at=(0, 0), bias=0.0):
        return ref.occluded(i + at[0], j + at[1], np.full(1, z, F), np.full((2, 2), depth, F),
                            np.full((2, 2), face, np.int32), mode, bias)[0]

    nearer, farther = z - F(sign * 0.25), z + F(sign * 0.25)
    assert occ(nearer) == 1.0                      # inside, covered, strictly nearer
    assert occ(nearer, at=(2, 0)) == 0.0           # outside the map
    assert occ(nearer, at=(0, -1)) == 0.0
    assert occ(nearer, face=-1) == 0.0             # an uncovered texel
    assert occ(z) == 0.0                           # a tie
    assert occ(farther) == 0.0
    assert occ(np.nan) == 0.0
    assert occ(nearer, bias=0.2) == 1.0            # nearer by more than the bias
    assert occ(nearer, bias=0.25) == 0.0           # the bias makes it a tie: lit
    assert occ(nearer, bias=0.5) == 0.0
    next_nearer = np.nextafter(z, F(-sign * np.inf), dtype=F)
    assert occ(next_nearer) == 1.0                 # one ulp is strictly nearer


# ---- the filter -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_weights_sum_the_taps_in_the_stated_order(radius):
    """A random map of occluders: the shade is the rows' sums over dj ascending, summed over di ascending."""
    rng = np.random.RandomState(radius)
    hs, ws = 16, 8
    face = np.where(rng.rand(hs, ws) < 0.5, 0, -1).astype(np.int32)
    depth = np.zeros((hs, ws), F)
    for i, j, fi, fj in [(7, 3, 0.3, 0.7), (0, 0, 0.9, 0.1), (15, 7, 0.5, 0.25), (-1, 4, 0.6, 0.6), (3, -2, 0.2, 0.2)]:
        p = np.asarray(at_texel(i, j, hs, ws, 1.0, fi, fj), F)
        a = (p[0] + F(1)) * (F(0.5) * F(hs)) - F(0.5)
        b = (p[1] + F(1)) * (F(0.5) * F(ws)) - F(0.5)
        i0, j0 = int(np.floor(a)), int(np.floor(b))
        fa, fb = F(a - np.floor(a)), F(b - np.floor(b))
        total = F(0)
        for di in range(-radius, radius + 2):
            row = F(0)
            for dj in range(-radius, radius + 2):
                ii, jj = i0 + di, j0 + dj
                o = F(1) if (0 <= ii < hs and 0 <= jj < ws and face[ii, jj] >= 0) else F(0)
                wj = F(1) - fb if dj == -radius else (fb if dj == radius + 1 else F(1))
                row = F(row + F(wj * o))
            wi = F(1) - fa if di == -radius else (fa if di == radius + 1 else F(1))
            total = F(total + F(wi * row))
        want = min(F(total * ref.K[radius]), F(1))
        assert bits(one(p, depth, face, radius=radius)) == bits(want)


def test_the_constants_are_the_nearest_floats():
    for r in range(4):
        exact = 1.0 / (2 * r + 1) ** 2
        k = ref.K[r]
        assert k.dtype == F and abs(float(k) - exact) <= min(abs(float(np.nextafter(k, F(0))) - exact),
                                                             abs(float(np.nextafter(k, F(1))) - exact))


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_an_all_occluding_map_gives_exactly_one(radius):
    rng = np.random.RandomState(7 + radius)
    n = 4000
    position = np.ones((n, 3), F)
    position[:, :2] = rng.uniform(-0.5, 0.5, (n, 2))  # at least 16 texels from the border of a 64^2 map
    position[:8, :2] = [at_texel(20, 30, 64, 64, fi=f, fj=g)[:2] for f in (0.0, 0.5) for g in (0.0, 0.25, 0.5, 0.75)]
    s = ref.shade(position, np.zeros(n, np.int32), np.zeros((64, 64), F), np.zeros((64, 64), np.int32), IDENTITY,
                  radius=radius)
    assert np.array_equal(bits(s), bits(np.ones(n, F)))


def picture(rng, shape=(2, 9, 7)):
    image = rng.standard_normal(shape + (3,)).astype(F)
    image[0, 0, 0] = [np.nan, -0.0, np.inf]
    position = rng.uniform(-1.2, 1.2, shape + (3,)).astype(F)
    face = np.where(rng.rand(*shape) < 0.8, 3, -1).astype(np.int32)
    return image, position, face


@pytest.mark.parametrize("radius", [0, 3])
def test_an_uncovered_map_and_zero_strength_leave_the_bits(radius):
    rng = np.random.RandomState(11)
    image, position, face = picture(rng)
    out, s = ref.shadow(image, position, face, np.full((5, 3), -9.0, F), np.full((5, 3), -1, np.int32), IDENTITY,
                        radius=radius)
    assert np.array_equal(bits(s), np.zeros(s.shape, np.uint32))  # +0.0, not -0.0
    assert np.array_equal(bits(out), bits(image))
    out, s = ref.shadow(image, position, face, np.full((5, 3), -9.0, F), np.zeros((5, 3), np.int32), IDENTITY,
                        radius=radius, strength=0.0)
    assert (s > 0).any()
    assert np.array_equal(bits(out), bits(image))


def test_a_shadowed_pixel_is_multiplied_once():
    image = np.array([[0.5, 1.0, 0.3]], F)
    out, s = ref.shadow(image, [at_texel(1, 1, 4, 4)], np.zeros(1, np.int32), np.zeros((4, 4), F),
                        np.zeros((4, 4), np.int32), IDENTITY, radius=0, strength=0.6)
    assert s[0] == 1.0
    assert np.array_equal(bits(out), bits(image * (F(1) - F(0.6) * F(1))))


def test_points_that_fail_the_projection_have_no_shade():
    depth, face = np.zeros((4, 4), F), np.zeros((4, 4), np.int32)
    for p in ([np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.nan], [0, 0, -np.inf], [3e7, 0, 1], [0, -3e7, 1], [1e38, 0, 1]):
        assert bits(one(p, depth, face))[()] == 0, p
    assert one([0, 0, 1], depth, face) == 1.0
    assert one([-1.6, 0, 1], depth, face, radius=0) == 0.0  # beside the map
    # a perspective light: a point behind it, and in its plane, have none; the point in front has
    for p, want in (([0.1, 0.1, 1.0], 1.0), ([0.1, 0.1, -1.0], 0.0), ([0.1, 0.1, 0.0], 0.0), ([0.0, 0.0, 0.0], 0.0)):
        assert one(p, depth, face, projection=ref.PERSPECTIVE) == want, p
    # an uncovered pixel is not looked at
    s = ref.shade(np.array([[0, 0, 1]], F), np.array([-1], np.int32), depth, face, IDENTITY)
    assert bits(s)[0] == 0


def test_a_one_texel_map_counts_only_the_taps_on_it():
    """1 x 1 map, radius 2: of the 36 taps only the one on texel (0, 0) counts, with its weight along each axis."""
    depth, face = np.zeros((1, 1), F), np.zeros((1, 1), np.int32)
    k = ref.K[2]
    assert one([0.0, 0.0, 1.0], depth, face, radius=2) == F(F(1) * k)  # a = b = 0: di = dj = 0, weight 1
    # a = 2.25: i0 = 2, texel 0 is di = -2, weight 1 - fa = 0.75; b = -2.5: j0 = -3, texel 0 is dj = 3, weight fb = 0.5
    s = one([4.5, -5.0, 1.0], depth, face, radius=2)
    assert s == F(F(F(0.75) * F(0.5)) * k)
    assert one([7.0, 0.0, 1.0], depth, face, radius=2) == 0.0  # a = 3.5: the footprint starts at texel 1
    assert one([0.0, 0.0, 1.0], depth, np.full((1, 1), -1, np.int32), radius=2) == 0.0


# ---- geometry: the shadow of a sphere on a floor --------------------------------------------------------------------
@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def test_the_shadow_of_a_sphere_lies_where_geometry_puts_it(recon):
    """Independent of the restatement's reading of the definition: with d the float64 distance, in the light's map
    plane, between a floor pixel's point and the sphere centre's projection, R the sphere's radius there and band =
    (r+1) sqrt(2) texels + 1 voxel, d < R - band is fully shadowed and d > R + band fully lit.  Measured here: R = 30.9
    texels, band = 3.9, 864 pixels inside, 414 outside, the band holds 23 % of the pixels with d < R + band."""
    radius = 1
    light = cases.light(recon, radius=radius)
    verts, faces = cases.sphere_mesh()
    lit = oracle.orthogonal(np.ascontiguousarray(verts.T), light.calib).T
    smap = render_ref.render(lit, faces, cases.MAP, cases.MAP, nearest="min")
    fv, ff, _ = cases.plank()
    h, w = 128, 12
    seen = render_ref.render(oracle.orthogonal(np.ascontiguousarray(fv.T), cases.camera_down()).T, ff, h, w, attr=fv,
                             nearest="max")
    assert (seen.face >= 0).all()
    s = ref.shade(seen.image, seen.face, smap.depth, smap.face, light.calib, ref.ORTHOGONAL, ref.MIN_Z, 0.0, radius)
    c = light.calib.astype(np.float64)
    per_unit = np.linalg.norm(c[0, :3]) * cases.MAP / 2  # texels per world unit in the map plane
    assert abs(np.linalg.norm(c[1, :3]) * cases.MAP / 2 - per_unit) < 1e-5 and abs(c[0, :3] @ c[1, :3]) < 1e-6
    points = seen.image.reshape(-1, 3).astype(np.float64)
    d = (np.linalg.norm(points @ c[:2, :3].T, axis=1) * cases.MAP / 2).reshape(h, w)  # the centre is the origin
    big_r = cases.RADIUS * per_unit
    band = (radius + 1) * np.sqrt(2.0) + cases.VOXEL * per_unit
    inside, outside = d < big_r - band, d > big_r + band
    assert inside.sum() > 500 and outside.sum() > 200
    assert (s[inside] == 1.0).all()
    assert np.array_equal(bits(s[outside]), np.zeros(outside.sum(), np.uint32))
    assert ((d < big_r + band) & ~inside).sum() <= 0.25 * (d < big_r + band).sum()
    # the light travels towards +x: the shadow lies beyond the sphere, about where the centre's ray meets the floor
    centroid = seen.image[..., 0][s > 0].mean()
    assert abs(centroid - (-cases.FLOOR_Y) * np.tan(cases.TILT)) < 0.05 and centroid > 0.4


# ---- host logic -----------------------------------------------------------------------------------------------------
def test_light_refusals(recon):
    good = np.eye(4, dtype=F)
    light = recon.Light(good, "perspective", res=(5, 3), near=0.5, bias=0.01, radius=3, strength=1.0, nearest="max")
    assert light.res == (5, 3) and light.near == 0.5 and light.radius == 3 and light.calib.shape == (3, 4)
    assert recon.Light(good).res == (512, 512) and recon.Light(good).radius == 1 and recon.Light(good).strength == 0.6
    for kw in (dict(calib=np.eye(2)), dict(calib=np.stack([good, good])), dict(calib=good * np.nan),
               dict(projection="fisheye"), dict(projection=0), dict(res=0), dict(res=4097), dict(res=(4, 0)),
               dict(res=(4, 4, 4)), dict(res=2.5), dict(near=0.5), dict(projection="perspective", near=0.0),
               dict(projection="perspective", near=np.inf), dict(bias=-0.1), dict(bias=np.nan), dict(bias=np.inf),
               dict(radius=-1), dict(radius=4), dict(radius=1.0), dict(radius=True), dict(strength=-0.1),
               dict(strength=1.5), dict(strength=np.nan), dict(nearest="far")):
        args = dict(calib=good)
        args.update(kw)
        with pytest.raises(ValueError):
            recon.Light(**args)
    for args in (((0, 0, 0),), ((np.nan, 1, 0),), ((1, 0),), ((0, -1, 0), (1, 1, 1), (0, 0, 0))):
        with pytest.raises(ValueError):
            recon.Light.directional(*args)
    with pytest.raises(ValueError):
        recon.Light.directional((0, -1, 0), projection="perspective")
    with pytest.raises(ValueError):
        recon.Light.directional((0, -1, 0), radius=7)


def test_scene_refuses_what_is_not_a_light(recon):
    quad = np.zeros((4, 3), F)
    for bad in ("sun", 1.0, np.eye(4)):
        with pytest.raises(ValueError, match="light"):  # before anything is uploaded
            recon.Scene(quad, np.array([[0, 1, 2]]), np.zeros((4, 2), F), np.zeros((2, 2, 3), F), device="cpu", light=bad)


@pytest.mark.parametrize("direction", [(0, -1, 0), (0.5, -0.8, 0.2), (1, 1, 1), (0, 0, 3)])
def test_directional_fits_the_box(recon, direction):
    b_min, b_max = (-1.0, -0.5, 0.0), (2.0, 1.5, 0.5)
    light = recon.Light.directional(direction, b_min, b_max, res=32)
    assert light.projection == "orthogonal" and light.nearest == "min" and light.near is None and light.res == (32, 32)
    corners = np.array([[x, y, z] for x in (b_min[0], b_max[0]) for y in (b_min[1], b_max[1])
                        for z in (b_min[2], b_max[2])], F)
    xyz = oracle.orthogonal(np.ascontiguousarray(corners.T), light.calib).T
    assert np.isfinite(xyz).all() and (np.abs(xyz[:, :2]) <= 1.0).all() and (xyz[:, 2] >= 0).all()
    rot = light.calib[:, :3].astype(np.float64)
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    assert np.allclose(rot[2], d, atol=1e-6)  # depth grows along the light's travel
    assert abs(rot[0] @ rot[1]) < 1e-6 and abs(rot[0] @ rot[2]) < 1e-6 and abs(rot[1] @ rot[2]) < 1e-6
    assert np.linalg.det(rot) > 0
    assert np.isclose(np.linalg.norm(rot[0]), np.linalg.norm(rot[1]))
    assert np.abs(xyz[:, :2]).max() > 0.5  # the sphere fills the map: the box is not lost in it


def test_the_light_belongs_to_the_scene_and_the_picture_options_are_unchanged(recon):
    import inspect

    from monoport_amd import pipeline
    assert list(inspect.signature(recon.Scene.__init__).parameters)[-1] == "light"  # a new keyword at the end
    assert list(inspect.signature(recon.render_scene).parameters)[-1] == "casters"
    assert pipeline.PICTURE_KEYS[-2:] == ("scene", "composite")
    assert "light" not in pipeline.PICTURE_KEYS and "light" not in pipeline.PictureOptions._fields
    assert len(pipeline.PictureOptions._fields) == len(pipeline.PICTURE_KEYS)
