"""The numpy restatement of mp_mesh_simplify (tests/mesh_simplify_ref.py) on its own: against a dict-and-loop
implementation written independently here, against exact rational arithmetic, and the properties the definition
promises (one vertex per occupied cell, means inside their members' boxes, edge parity of closed meshes).  CPU only."""
import fractions
import math

import numpy as np
import pytest

import mesh_simplify_ref as ms


def slow_simplify(verts, faces, n, b_min, b_max):
    """The definition once more, one vertex and one face at a time, with Python integers for the sums."""
    f32 = np.float32
    inv = [f32(n) / (f32(b_max[a]) - f32(b_min[a])) for a in range(3)]
    cells = {}
    keys = []
    for v in np.asarray(verts, np.float32):
        if not all(math.isfinite(float(x)) and abs(float(x)) < 32768.0 for x in v):
            keys.append(None)
            continue
        c = []
        for a in range(3):
            t = float(f32(f32(v[a] - f32(b_min[a])) * inv[a]))
            c.append(0 if t < 0 else n - 1 if t >= n else int(math.floor(t)))
        key = (c[2] * n + c[1]) * n + c[0]
        keys.append(key)
        cells.setdefault(key, []).append(v)
    order = {key: i for i, key in enumerate(sorted(cells))}
    out = np.zeros((len(order), 3), np.float32)
    for key, members in cells.items():
        for a in range(3):
            s = sum(int(round(float(p[a]) * 1048576.0)) for p in members)  # round(): ties to even, on an exact product
            out[order[key], a] = f32(float(fractions.Fraction(s, len(members) * 1048576)))  # one rounding to double
    vmap = np.array([-1 if k is None else order[k] for k in keys], np.int32).reshape(-1)
    kept = []
    for face in np.asarray(faces):
        if any(i < 0 or i >= len(keys) for i in face):
            continue
        g = [int(vmap[i]) for i in face]
        if min(g) < 0 or len(set(g)) < 3:
            continue
        kept.append(g)
    return out, np.array(kept, np.int32).reshape(-1, 3), vmap


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 17])
def test_equals_the_slow_implementation_on_a_mesh(n):
    v, f = ms.oracle_mesh("blob17_3")
    _same(ms.simplify_ref(v, f, n), slow_simplify(v, f, n, ms.BMIN, ms.BMAX))


def test_equals_the_slow_implementation_on_the_soup():
    v, f = ms.soup()
    got = ms.simplify_ref(v, f, ms.SOUP_CELLS, ms.SOUP_BMIN, ms.SOUP_BMAX)
    _same(got, slow_simplify(v, f, ms.SOUP_CELLS, ms.SOUP_BMIN, ms.SOUP_BMAX))
    out, faces, vmap = got
    key, valid = ms.cell_keys(v, ms.SOUP_CELLS, ms.SOUP_BMIN, ms.SOUP_BMAX)
    assert (~valid).sum() == 6 and (vmap[~valid] == -1).all() and (vmap[valid] >= 0).all()
    # the vertices on b_max and those outside land in border cells
    hi = np.asarray(ms.SOUP_BMAX, np.float32)
    assert key[np.flatnonzero((v == hi).all(1))[0]] == ms.SOUP_CELLS ** 3 - 1
    print("soup: %d -> %d vertices, %d -> %d faces" % (len(v), len(out), len(f), len(faces)))
    assert 0 < len(faces) < len(f) - 30  # faces were dropped for every reason, many stay
    # duplicates and mirror images both stay
    rows = [tuple(r) for r in faces.tolist()]
    assert len(set(rows)) < len(rows)


@pytest.mark.parametrize("name,r", [("blob33_5", 33), ("blob17_3", 17), ("sphere33", 33)])
def test_properties_on_closed_meshes(name, r):
    v, f = ms.oracle_mesh(name)
    assert ms.edge_parity_even(f)
    for n in (1, 2, 3, 8, 16, r // 2, r, 2 * r):
        out, faces, vmap = ms.simplify_ref(v, f, n)
        key, valid = ms.cell_keys(v, n)
        assert valid.all() and len(out) == len(np.unique(key)) == vmap.max() + 1
        assert np.array_equal(np.unique(key)[vmap], key)  # ascending key order
        # inside the members' bounding box -- that of their fixed-point positions rint(v 2^20) / 2^20, which is what is
        # averaged (a member is moved by up to 2^-21 before): the mean of integers lies between their extremes, and
        # the roundings to double and to f32 are monotone, so no tolerance is needed
        q = (np.rint(v.astype(np.float64) * ms.SCALE) / ms.SCALE).astype(np.float32)
        assert np.abs(q.astype(np.float64) - v).max() <= 2.0 ** -21
        lo = np.full((len(out), 3), np.inf, np.float32)
        hi = np.full((len(out), 3), -np.inf, np.float32)
        np.minimum.at(lo, vmap, q)
        np.maximum.at(hi, vmap, q)
        assert (out >= lo).all() and (out <= hi).all(), n
        assert ms.edge_parity_even(faces), n
        assert len(out) <= len(v) and len(faces) <= len(f)
        if n == 1:
            assert len(out) == 1 and len(faces) == 0
    if name == "blob33_5":
        sizes = {n: tuple(len(x) for x in ms.simplify_ref(v, f, n)[:2]) for n in (16, 33, 66)}
        print("blob_volume(33, 5): %d vertices, %d faces -> %s" % (len(v), len(f), sizes))
        assert (len(v), len(f)) == (1562, 3124)
        assert sizes == {16: (285, 576), 33: (848, 1710), 66: (1372, 2746)}


def test_no_shared_cell_leaves_the_mesh_alone():
    """A soup whose vertices lie in distinct cells: the faces are unchanged, the positions are the fixed-point ones."""
    rng = np.random.RandomState(22)
    n = 64
    cells = rng.choice(n ** 3, 500, replace=False)
    c = np.stack([cells % n, (cells // n) % n, cells // (n * n)], 1)
    v = (-1.0 + (c + 0.25 + 0.5 * rng.rand(500, 3)) * (2.0 / n)).astype(np.float32)
    f = np.stack([rng.permutation(500)[:300], rng.permutation(500)[:300], rng.permutation(500)[:300]], 1).astype(np.int32)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    out, faces, vmap = ms.simplify_ref(v, f, n)
    assert len(out) == 500 and np.array_equal(np.sort(vmap), np.arange(500))
    assert np.array_equal(faces, vmap[f])  # the same faces, under the renumbering by key
    want = (np.rint(v.astype(np.float64) * 2.0 ** 20) / 2.0 ** 20).astype(np.float32)
    assert np.array_equal(out[vmap].view(np.uint32), want.view(np.uint32))


def test_a_sum_beyond_2_53_is_rounded_once():
    v = ms.crowd()
    out, faces, vmap = ms.simplify_ref(v, np.zeros((0, 3), np.int32), ms.CROWD_CELLS, ms.CROWD_BMIN, ms.CROWD_BMAX)
    assert out.shape == (1, 3) and len(faces) == 0 and (vmap == 0).all()
    for a in range(3):
        s = sum(int(round(float(x) * 1048576.0)) for x in v[:, a])
        assert abs(s) > 2 ** 53
        want = np.float32(float(fractions.Fraction(s, len(v) * 1048576)))
        assert out[0, a].view(np.uint32) == want.view(np.uint32), a
