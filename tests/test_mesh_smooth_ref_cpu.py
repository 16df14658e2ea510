"""The numpy restatement of mp_mesh_smooth (tests/mesh_smooth_ref.py) on its own: against the dict-and-loop
implementation beside it, bit for bit, and the facts the feature is built on, as conditions: Taubin passes halve the
normal error of a terraced sphere and keep its volume, plain Laplacian passes shrink it.  CPU only."""
import numpy as np
import pytest

import mesh_simplify_ref as simp
import mesh_smooth_ref as sm


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _both(v, f, iterations, pin, lam=0.5, mu=-0.53):
    got = sm.smooth_ref(v, f, iterations, lam, mu, pin)
    want, ring = sm.loop_ref(v, f, iterations, lam, mu, pin)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert sm.same_bits(got, want)
    assert np.array_equal(sm.ring_ref(v, f), ring)
    return got, ring


def test_equals_the_loop_on_a_closed_mesh():
    v, f = sm.oracle_mesh("blob17_3")
    assert len(v) == 298
    got, ring = _both(v, f, 3, True)
    assert (ring > 0).all()  # closed: no border vertex, none without a neighbour
    assert not np.array_equal(_bits(got), _bits(v))
    assert sm.same_bits(got, sm.smooth_ref(v, f, 3, pin=False))  # nothing to pin


@pytest.mark.parametrize("pin", [True, False])
def test_equals_the_loop_on_an_open_mesh(pin):
    v, f = sm.open_mesh()
    got, ring = _both(v, f, 2, pin)
    border = ring < 0
    assert len(v) == 1562 and border.sum() == 227
    moved = (_bits(got) != _bits(v)).any(1)
    if pin:  # border vertices keep their bits, and they still pull their neighbours
        assert not moved[border].any() and moved[~border].all()
    else:
        assert moved[border].all()


@pytest.mark.parametrize("pin", [True, False])
def test_equals_the_loop_on_the_soup(pin):
    v, f = sm.soup()
    got, ring = _both(v, f, 2, pin)
    lonely = ring == 0
    assert lonely.sum() >= 4  # the unreferenced vertices keep their bits
    assert np.array_equal(_bits(got)[lonely], _bits(v)[lonely])
    assert np.abs(ring).max() >= 200  # the fan's centre


def test_equals_the_loop_on_the_book():
    v, f = sm.book(60)
    got, ring = _both(v, f, 2, False)
    assert ring[0] == ring[1] == -61 and (ring[2:] == -2).all()  # the shared edge is even, every page's other two are open
    assert not np.array_equal(_bits(got), _bits(v))
    assert np.array_equal(_bits(sm.smooth_ref(v, f, 2)), _bits(v))  # pinned: every vertex is a border vertex


def test_zero_factors_return_the_input_bits():
    v, f = sm.soup()
    got = sm.smooth_ref(v, f, 3, 0.0, 0.0, False)
    # p + 0 * (m - p) gives p's bits, except +0 for p = -0, and NaN where m - p is not finite (huge coordinates)
    same = _bits(got) == _bits(v)
    assert same.mean() > 0.99 and ((got == v) | np.isnan(got))[~same].all()
    v, f = sm.oracle_mesh("blob17_3")
    assert np.array_equal(_bits(sm.smooth_ref(v, f, 3, 0.0, 0.0)), _bits(v))


def test_rings():
    for name in ("blob17_3", "blob33_5", "steps65"):
        v, f = sm.oracle_mesh(name)
        ring = sm.ring_ref(v, f)
        assert (ring >= 3).all() and ring.max() <= 13, name  # a closed marching-cubes mesh: no border vertex
    # a closed mesh after the vertex clustering: duplicate faces and all, every multiplicity is even
    v, f = sm.oracle_mesh("blob33_5")
    sv, sf, _ = simp.simplify_ref(v, f, 16)
    assert len(sv) == 285 and (sm.ring_ref(sv, sf) >= 0).all()
    # one triangle: three border vertices of degree 2; an index out of range drops the face
    tri = np.zeros((3, 3), np.float32)
    assert sm.ring_ref(tri, [[0, 1, 2]]).tolist() == [-2, -2, -2]
    assert sm.ring_ref(tri, [[0, 1, 2], [2, 1, 0]]).tolist() == [2, 2, 2]
    assert sm.ring_ref(tri, [[0, 1, 3], [0, -1, 2], [1, 1, 1]]).tolist() == [0, 0, 0]
    assert sm.ring_ref(tri, [[0, 0, 1]]).tolist() == [1, 1, 0]  # (0,0) is skipped; (0,1) and (1,0): m = 2, even


def _vertex_normals(v, f):
    """Accumulated per-vertex normals (unit face normals summed over the incident corners), in double."""
    v = v.astype(np.float64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n /= np.maximum(np.linalg.norm(n, axis=1), 1e-30)[:, None]
    out = np.zeros_like(v)
    for c in range(3):
        np.add.at(out, f[:, c], n)
    return out / np.maximum(np.linalg.norm(out, axis=1), 1e-30)[:, None]


def _radial_error_deg(v, f):
    radial = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1)[:, None]
    cos = np.clip((_vertex_normals(v, f) * radial).sum(1), -1.0, 1.0)
    return np.degrees(np.arccos(cos))


def _volume(v, f):
    v = v.astype(np.float64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def test_taubin_fairs_a_terraced_sphere_and_keeps_its_volume():
    v, f = sm.oracle_mesh("steps65")
    out = sm.smooth_ref(v, f, 10)
    before, after = _radial_error_deg(v, f), _radial_error_deg(out, f)
    vol0, vol1 = _volume(v, f), _volume(out, f)
    r0, r1 = np.linalg.norm(v, axis=1), np.linalg.norm(out, axis=1)
    print("median %.2f -> %.2f deg, p99 %.1f -> %.1f deg, radius std %.5f -> %.5f, volume %.5f -> %.5f (%+.3f %%)"
          % (np.median(before), np.median(after), np.percentile(before, 99), np.percentile(after, 99), r0.std(),
             r1.std(), vol0, vol1, 100.0 * (vol1 / vol0 - 1.0)))
    assert vol0 > 0.8
    assert np.median(after) <= 0.5 * np.median(before)
    assert abs(vol1 / vol0 - 1.0) <= 0.002
    assert r1.std() < r0.std()
    laplace = sm.smooth_ref(v, f, 10, 0.5, 0.0)
    shrink = 1.0 - _volume(laplace, f) / vol0
    print("mu = 0: the volume shrinks by %.2f %%" % (100.0 * shrink))
    assert shrink > 0.01


def test_64_iterations_stay_finite():
    v, f = sm.oracle_mesh("steps65")
    out = sm.smooth_ref(v, f, 64)
    print("64 iterations: volume %+.3f %%" % (100.0 * (_volume(out, f) / _volume(v, f) - 1.0)))
    assert np.isfinite(out).all()


def test_a_smooth_field_gains_little():
    """The caveat the documents state: on a field that is already smooth the normals gain a little and the radius
    loses a little."""
    v, f = sm.oracle_mesh("sphere65")
    out = sm.smooth_ref(v, f, 10)
    r0, r1 = np.linalg.norm(v, axis=1).std(), np.linalg.norm(out, axis=1).std()
    e0, e1 = np.median(_radial_error_deg(v, f)), np.median(_radial_error_deg(out, f))
    print("smooth field: radius std %.1e -> %.1e, median normal error %.2f -> %.2f deg" % (r0, r1, e0, e1))
    assert r0 < r1 < 1e-3 and e1 < e0 < 1.0
