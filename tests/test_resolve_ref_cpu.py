"""tests/resolve_ref.py, the numpy restatement of mp_picture_resolve, against what the definition promises -- and, in one
test that does not rest on the restatement's own logic, the coverage it gives against the exact area of a triangle."""
import numpy as np
import pytest

import mesh_render_ref as mrr
import resolve_ref as rr


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("s", [2, 4])
def test_equal_samples_keep_their_bits(s):
    """x + x + ... (s*s terms, one f32 addition each) / (s*s) is x again.  s = 2, any x whose sum does not overflow: 2x
    is exact, fl(3x) is off by at most an ulp of x, and 4x, representable, is then the nearest value to fl(3x) + x.
    s = 4: sequential additions give that only while every partial sum k x, k <= 16, is exact, which holds for an x of
    at most 20 significant bits (the backgrounds and flat colours 0, 1, 0.5, k / 256 ...); any other x may move, by less
    than 8 ulps: each of the 15 additions errs by at most half an ulp of a sum <= 16 |x|, that is 8 ulps of x, and the
    division by 16 is exact -- 15 * 8 / 16 ulps."""
    rng = np.random.default_rng(5)
    h, w = 6, 7
    x = (rng.standard_normal((h, w, 3)) * np.exp2(rng.integers(-120, 120, (h, w, 3)))).astype(np.float32)
    x[0, 0] = (0.0, -0.0, 1.0)
    x[0, 1] = (np.float32(1e-42), np.float32(-3e-45), np.float32(2.0 ** -126))  # denormals and the smallest normal
    x[0, 2] = (np.float32(1e37), np.float32(-1e37), np.float32(0.1))
    if s == 4:
        general = rr.resolve(np.repeat(np.repeat(x, s, axis=0), s, axis=1), None, None, None, s)[0]
        assert np.abs(_bits(general).astype(np.int64) - _bits(x).astype(np.int64)).max() < 8
        x = (_bits(x) & np.uint32(0xFFFFFFF0)).view(np.float32)  # 20 significant bits (denormals: fewer still)
    fine = np.repeat(np.repeat(x, s, axis=0), s, axis=1)
    image = rr.resolve(fine, None, None, None, s)[0]
    assert np.array_equal(_bits(image), _bits(x))
    # the constant pictures the renders produce: a background and 8-bit colours
    for value in (1.0, 0.0, 0.5, 0.75, 200.0 / 256.0, 1.0 / 3.0):
        if s == 4 and value == 1.0 / 3.0:
            continue
        fine = np.full((2 * s, 3 * s, 3), value, np.float32)
        assert np.array_equal(_bits(rr.resolve(fine, None, None, None, s)[0]), _bits(np.full((2, 3, 3), value, np.float32)))


def test_the_sum_starts_from_the_first_sample_in_row_major_order():
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    # (((big + 1) + 1) + -big) = 0 in f32, while any order that adds the ones first gives 2
    fine = np.zeros((2, 2, 3), np.float32)
    fine[0, 0], fine[0, 1], fine[1, 0], fine[1, 1] = big, one, one, -big
    assert np.array_equal(rr.resolve(fine, None, None, None, 2)[0][0, 0], np.zeros(3, np.float32))
    fine[0, 0], fine[0, 1], fine[1, 0], fine[1, 1] = one, one, big, -big
    assert np.array_equal(rr.resolve(fine, None, None, None, 2)[0][0, 0], np.full(3, 0.5, np.float32))
    # from the first sample, not from +0: four samples of -0 stay -0
    fine[:] = -0.0
    assert np.array_equal(_bits(rr.resolve(fine, None, None, None, 2)[0]), _bits(np.full((1, 1, 3), -0.0, np.float32)))
    # s = 3 divides by 9: one correctly rounded f32 division of the f32 sum
    x = np.arange(1, 10, dtype=np.float32).reshape(3, 3) * np.float32(0.1)
    acc = np.float32(0.1)
    for v in x.reshape(-1)[1:]:
        acc = np.float32(acc + v)
    got = rr.resolve(np.repeat(x[:, :, None], 3, axis=2), None, None, None, 3)[0]
    assert np.array_equal(got[0, 0], np.full(3, np.float32(acc / np.float32(9.0))))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_coverage_of_empty_and_full_pictures(s):
    h, w = 3, 5
    depth = np.zeros((s * h, s * w), np.float32)
    for face, mask, want in ((np.full((s * h, s * w), -1, np.int32), None, 0.0),
                             (np.full((s * h, s * w), 7, np.int32), None, 1.0),
                             (None, np.zeros((s * h, s * w), np.uint8), 0.0),
                             (None, np.full((s * h, s * w), 1, np.uint8), 0.0),  # the scene is not the subject
                             (None, np.full((s * h, s * w), 2, np.uint8), 1.0)):
        cov = rr.resolve(None, None if face is None else depth, face, mask, s)[4]
        assert cov.dtype == np.float32 and np.array_equal(cov, np.full((h, w), want, np.float32))
    # a mask outranks the face ids: the subject's samples are those the composite says show the subject
    face = np.full((s * h, s * w), 3, np.int32)
    mask = np.full((s * h, s * w), 1, np.uint8)
    mask[0, 0] = 2
    cov = rr.resolve(None, None, face, mask, s)[4]
    assert cov[0, 0] == np.float32(1.0) / np.float32(s * s) and not cov[1:].any() and not cov[0, 1:].any()
    # nothing shows: depth +0.0 and face -1
    _, d, f, m, _ = rr.resolve(None, np.full((s * h, s * w), 5.0, np.float32), np.full((s * h, s * w), -1, np.int32),
                               None, s)
    assert np.array_equal(_bits(d), np.zeros((h, w), np.uint32)) and np.array_equal(f, np.full((h, w), -1, np.int32))
    assert m is None


def test_ties_take_the_first_sample_and_min_is_the_sign_flipped_key():
    s = 2
    face = np.array([[10, 11], [12, 13]], np.int32)
    depth = np.array([[1.0, 2.0], [2.0, 0.5]], np.float32)
    _, d, f, _, _ = rr.resolve(None, depth, face, None, s, "max")
    assert d[0, 0] == 2.0 and f[0, 0] == 11  # of the two 2.0, the first in sample order
    _, d, f, _, _ = rr.resolve(None, depth, face, None, s, "min")
    assert d[0, 0] == 0.5 and f[0, 0] == 13
    depth = np.array([[0.5, 0.5], [0.5, 0.5]], np.float32)
    for nearest in ("max", "min"):
        assert rr.resolve(None, depth, face, None, s, nearest)[2][0, 0] == 10
    # the key orders the bits: +0 is nearer than -0 under "max", -0 nearer than +0 under "min" (the key of -depth)
    depth = np.array([[-0.0, 0.0], [-0.0, 0.0]], np.float32)
    _, d, f, _, _ = rr.resolve(None, depth, face, None, s, "max")
    assert _bits(d)[0, 0] == 0 and f[0, 0] == 11
    _, d, f, _, _ = rr.resolve(None, depth, face, None, s, "min")
    assert _bits(d)[0, 0] == 0x80000000 and f[0, 0] == 10
    # "min" is the key of the sign-flipped depth, whatever the values
    rng = np.random.default_rng(2)
    depth = rng.standard_normal((8, 12)).astype(np.float32)
    face = rng.integers(-1, 50, (8, 12)).astype(np.int32)
    lo = rr.resolve(None, depth, face, None, 4, "min")
    hi = rr.resolve(None, -depth, face, None, 4, "max")
    shown = lo[2] >= 0
    assert np.array_equal(lo[2], hi[2]) and np.array_equal(lo[1][shown], -hi[1][shown])
    # an uncovered sample never wins, however near; a sample the mask hides never wins either
    depth = np.array([[9.0, 1.0], [1.0, 1.0]], np.float32)
    face = np.array([[-1, 4], [5, 6]], np.int32)
    assert rr.resolve(None, depth, face, None, s)[2][0, 0] == 4
    face = np.array([[3, 4], [5, 6]], np.int32)
    mask = np.array([[0, 1], [2, 2]], np.uint8)
    _, d, f, m, cov = rr.resolve(None, depth, face, mask, s)
    assert f[0, 0] == 4 and d[0, 0] == 1.0 and m[0, 0] == 2 and cov[0, 0] == 0.5


def test_mask_out_is_the_maximum():
    rng = np.random.default_rng(3)
    for s in (2, 3, 4):
        mask = rng.integers(0, 3, (4 * s, 5 * s)).astype(np.uint8)
        got = rr.resolve(None, None, None, mask, s)[3]
        want = mask.reshape(4, s, 5, s).max(axis=(1, 3))
        assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_outputs_follow_their_inputs_and_leading_views():
    rng = np.random.default_rng(4)
    s, nv, h, w = 3, 2, 2, 3
    image = rng.random((nv, s * h, s * w, 3)).astype(np.float32)
    depth = rng.random((nv, s * h, s * w)).astype(np.float32)
    face = rng.integers(-1, 9, (nv, s * h, s * w)).astype(np.int32)
    mask = rng.integers(0, 3, (nv, s * h, s * w)).astype(np.uint8)
    got = rr.resolve(image, depth, face, mask, s)
    assert [None if g is None else g.shape for g in got] == [(nv, h, w, 3), (nv, h, w), (nv, h, w), (nv, h, w), (nv, h, w)]
    for v in range(nv):
        one = rr.resolve(image[v], depth[v], face[v], mask[v], s)
        assert all(rr.same_bits(a[v], b) for a, b in zip(got, one))
    assert [g is None for g in rr.resolve(image, None, None, None, s)] == [False, True, True, True, True]
    assert [g is None for g in rr.resolve(None, depth, None, mask, s)] == [True, True, True, False, False]
    assert [g is None for g in rr.resolve(None, None, face, None, s)] == [True, True, True, True, False]


# ---- coverage against area: independent of the restatement's own logic ------------------------------------------------

def _clip(poly, axis, bound, keep_above):
    """Sutherland-Hodgman against one axis-aligned half-plane, float64."""
    out = []
    for k in range(len(poly)):
        p, q = poly[k], poly[(k + 1) % len(poly)]
        pin = p[axis] >= bound if keep_above else p[axis] <= bound
        qin = q[axis] >= bound if keep_above else q[axis] <= bound
        if pin:
            out.append(p)
        if pin != qin:
            t = (bound - p[axis]) / (q[axis] - p[axis])
            out.append(p + t * (q - p))
    return out


def _area_in_pixel(tri, i, j):
    poly = [np.asarray(p, np.float64) for p in tri]
    for axis, bound, above in ((0, i, True), (0, i + 1, False), (1, j, True), (1, j + 1, False)):
        poly = _clip(poly, axis, float(bound), above)
        if len(poly) < 3:
            return 0.0
    x, y = np.array([p[0] for p in poly]), np.array([p[1] for p in poly])
    return 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))


def _crosses(p, q, i, j):
    """Whether a piece of positive length of the segment p-q lies strictly inside pixel (i, j) (Liang-Barsky)."""
    d = q - p
    t0, t1 = 0.0, 1.0
    for axis, lo, hi in ((0, i, i + 1), (1, j, j + 1)):
        if d[axis] == 0:
            if not lo < p[axis] < hi:
                return False
            continue
        ta, tb = (lo - p[axis]) / d[axis], (hi - p[axis]) / d[axis]
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return t1 - t0 > 1e-9


# pixel coordinates of a 16 x 16 picture, multiples of 1/256 pixel = 1/2048 of the projected range [-1, 1]: the
# rasteriser's snap to 1/256 pixel is exact at 1, 2, 3 and 4 times the size
TRIANGLES = ([(1.25, 2.5), (14.125, 4.75), (5.5, 13.875)],
             [(0.0, 0.0), (15.99609375, 3.0), (2.0, 12.0)],
             [(3.0, 3.0), (13.0, 3.0), (8.21875, 14.6015625)])


@pytest.mark.parametrize("tri", TRIANGLES)
def test_coverage_against_the_exact_area(tri):
    n = 16
    pix = np.asarray(tri, np.float64)
    xyz = mrr.to_ndc(pix, n, n)  # the identity orthogonal camera: projected = world
    assert np.array_equal(xyz[:, :2] * 2048, np.rint(xyz[:, :2] * 2048))
    faces = np.array([[0, 1, 2]], np.int32)
    area = np.array([[_area_in_pixel(pix, i, j) for j in range(n)] for i in range(n)])
    (ax, ay), (bx, by) = pix[1] - pix[0], pix[2] - pix[0]
    assert abs(area.sum() - 0.5 * abs(ax * by - ay * bx)) < 1e-9
    edges = np.array([[sum(_crosses(pix[k], pix[(k + 1) % 3], i, j) for k in range(3)) for j in range(n)]
                      for i in range(n)])
    assert (edges == 1).sum() >= 20
    means = {}
    for s in (1, 2, 3, 4):
        fine = mrr.render(xyz, faces, s * n, s * n)
        if s == 1:
            cov = (fine.face >= 0).astype(np.float32)
        else:
            cov = rr.resolve(None, fine.depth, fine.face, None, s)[4]
        inner = edges == 0
        assert np.array_equal(cov[inner], np.rint(area[inner]).astype(np.float32))
        assert np.all(np.abs(area[inner] - np.rint(area[inner])) < 1e-9)
        err = np.abs(cov.astype(np.float64) - area)
        one = edges == 1
        assert np.all(err[one] <= (2 * s - 1) / s ** 2 + 1e-12), (s, err[one].max())
        means[s] = float(err[edges > 0].mean())
    assert means[1] > means[2] > means[4], means
