"""The numpy restatement of mp_volume_keep_largest (tests/keep_largest_ref.py), which the GPU tests compare the
kernels with, against scipy.ndimage.label: component count, sizes and the kept mask under the tie rule, at r = 17 and
33, for both connectivities.  No GPU."""
import numpy as np
import pytest

import keep_largest_ref as kl

ndimage = pytest.importorskip("scipy.ndimage")

NAMES = ["spheres33", "serpentine33", "equal_cubes17", "nan_bridge17", "empty17", "full17", "body_floater33",
         (1, 1, 1), (1, -1, 1), (1, 1, 0), (0, 1, -1), (-1, 0, 1), (0, 0, 1)]


def _noise(r, seed):
    return kl.paint(np.random.RandomState(seed).random_sample((r, r, r)) < 0.30, seed + 1)


def _scipy_keep_largest(vol, connectivity):
    """(kept mask, sizes by ascending smallest index, stats) from scipy's labels."""
    with np.errstate(invalid="ignore"):
        fg = vol > np.float32(kl.LEVEL)
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)  # face cross / all ones
    lab, n = ndimage.label(fg, structure=structure)
    if n == 0:
        return np.zeros_like(fg), [], [0, 0, 0, -1]
    flat = lab.ravel()
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))  # smallest linear index of every scipy label
    sizes = np.bincount(flat, minlength=n + 1)
    order = np.argsort(first[1:]) + 1  # scipy's labels by ascending id
    k = order[int(np.argmax(sizes[order]))]  # the first maximum: the smallest id of a tie
    return lab == k, sizes[order].tolist(), [int(fg.sum()), n, int(sizes[k]), int(first[k])]


def _check(vol, connectivity):
    out, stats = kl.keep_largest_ref(vol, kl.LEVEL, connectivity, 0.0)
    kept, sizes, want = _scipy_keep_largest(vol, connectivity)
    assert stats == want
    with np.errstate(invalid="ignore"):
        fg = vol > np.float32(kl.LEVEL)
    lab = kl.label_components(fg, connectivity)
    ids, got_sizes = np.unique(lab[fg], return_counts=True)
    assert got_sizes.tolist() == sizes
    assert all(lab.ravel()[i] == i for i in ids)  # an id is a voxel of its own component: the smallest index
    want_out = vol.copy()
    want_out[fg & ~kept] = 0.0
    assert np.array_equal(out.view(np.uint32), want_out.view(np.uint32))
    return stats


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", NAMES, ids=str)
def test_labeller_matches_scipy(name, connectivity):
    _check(kl.volume(name), connectivity)


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("r", [17, 33])
def test_labeller_matches_scipy_on_noise(r, connectivity):
    stats = _check(_noise(r, 40 + r), connectivity)
    assert stats[1] > (20 if connectivity == 6 else 1)


def test_the_cases_are_what_they_claim():
    """The properties the GPU cases are there for, from the reference alone."""
    assert kl.reference("spheres33", 6)[1][1] == 2
    s = kl.reference("serpentine33", 6)[1]
    assert s[1] == 2 and s[2] == 6935 and s[0] == 6935 + 125 and s == kl.reference("serpentine33", 26)[1]
    s = kl.reference("equal_cubes17", 6)[1]
    assert s == [128, 2, 64, (2 * 17 + 2) * 17 + 2]  # the tie goes to the smaller id
    for d in kl.EDGE_DIRECTIONS + kl.CORNER_DIRECTIONS:
        assert kl.reference(d, 6)[1][:3] == [91, 2, 64] and kl.reference(d, 26)[1][:3] == [91, 1, 91]
    assert len(kl.EDGE_DIRECTIONS) == 12 and len(kl.CORNER_DIRECTIONS) == 8
    assert kl.reference((0, 0, 1), 6)[1][:3] == [91, 1, 91]  # a shared face joins under both
    for c in (6, 26):
        out, s = kl.reference("nan_bridge17", c)
        assert s == [144, 2, 80, (2 * 17 + 2) * 17 + 8]
        assert np.array_equal(out.view(np.uint32)[2:6, 2:6, 6:8], kl.volume("nan_bridge17").view(np.uint32)[2:6, 2:6, 6:8])
        assert kl.reference("empty17", c)[1] == [0, 0, 0, -1] and kl.reference("full17", c)[1] == [4913, 1, 4913, 0]
        assert np.array_equal(kl.reference("full17", c)[0], kl.volume("full17"))
    assert kl.reference("noise65", 6)[1][1] > 1000 and kl.reference("noise65", 26)[1][1] > 10
    s = kl.reference("body129", 6)[1]
    assert s[1] == 4 and s[2] > 20000 and 129 ** 3 > 2 ** 21
    assert kl.reference("body_floater33", 6)[1][1] == 2


def test_forward_offsets():
    assert len(kl.forward_offsets(6)) == 3 and len(kl.forward_offsets(26)) == 13
    r = 17
    for c in (6, 26):
        assert all((dz * r + dy) * r + dx > 0 for dz, dy, dx in kl.forward_offsets(c))
