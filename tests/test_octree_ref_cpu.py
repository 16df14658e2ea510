"""The numpy restatement of the lossless octree rules (tests/octree_ref.py) and the inputs of
tests/test_octree_select_gpu.py, checked without a GPU: oracle.dilate_box against scipy on volumes narrower than the
box, select_level / conflicts chained level by level against oracle.seg3d_lossless, and the properties that make the
GPU inputs adversarial (a weak input fails here, not silently on the GPU)."""
import numpy as np
import pytest

import octree_ref as orf
from oracle import pifu_oracle as po
from test_box_threshold_cpu import B_MAX, B_MIN, all_idx

FIN_RES = [6, 11, 21, 41, 81]


@pytest.mark.parametrize("k", [3, 7, 9])
@pytest.mark.parametrize("n", [3, 5, 12])
def test_dilate_box_matches_scipy(n, k):
    """Zero-padded all-ones k^3 dilation, also where the volume is narrower than the half width of the box."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(100 * n + k)
    for density in (0.02, 0.2):
        mask = rng.random((n, n, n)) < density
        mask[tuple(rng.integers(0, n, 3))] = True
        want = ndimage.binary_dilation(mask, structure=np.ones((k, k, k), bool))
        assert np.array_equal(po.dilate_box(mask, k), want), (n, k, density)
    slab = rng.random((2, n, 1)) < 0.3  # sides of 1 and 2
    assert np.array_equal(po.dilate_box(slab, k), ndimage.binary_dilation(slab, structure=np.ones((k, k, k), bool)))


def _zyx(codes):
    return np.stack([codes >> 20, (codes >> 10) & 1023, codes & 1023], -1)


def chain_levels(field, res, balance=0.5, faster=True, final_level="dilate3"):
    """seg3d_lossless rebuilt from octree_ref.select_level / conflicts: (volume, stats, rounds, evaluated)."""
    rf, r0 = res[-1], res[0]
    query = lambda zyx, r: field(po.lattice_points(zyx, (rf - 1) // (r - 1), rf, B_MIN, B_MAX))
    occ = query(all_idx(r0), r0).reshape(r0, r0, r0)
    stats, rounds = [r0 ** 3], [0]
    if not (occ > np.float32(balance)).any():
        return None, stats, rounds, None
    ev = np.ones((r0, r0, r0), bool)
    for level in range(1, len(res)):
        r = res[level]
        box = po.dilation_for_level(level) if faster else 3
        if faster and level == len(res) - 1:
            box = {"dilate3": box, "upstream": 1, "interpolate": 0}[final_level]
        cur, _, sel, ev = orf.select_level(occ, ev, box, balance)
        nodes = orf.mask_codes(sel)
        n_level, n_rounds = nodes.size, 0
        while nodes.size:
            zyx = _zyx(nodes)
            vals = query(zyx, r)
            if not faster:
                grown, ev = orf.conflicts(nodes, vals, cur, ev, balance)
            cur[zyx[:, 0], zyx[:, 1], zyx[:, 2]] = vals
            if faster:
                break
            nodes = grown
            n_level += nodes.size
            n_rounds += 1 if nodes.size else 0
        occ = cur
        stats.append(n_level)
        rounds.append(n_rounds)
    return occ, stats, rounds, ev


MODES = [(True, "dilate3"), (True, "upstream"), (True, "interpolate"), (False, "dilate3")]


@pytest.mark.parametrize("faster,final_level", MODES)
@pytest.mark.parametrize("res", [[6, 11, 21, 41], [2, 3, 5, 9, 17], [5, 9, 17, 33]], ids=lambda r: "r%d" % r[0])
@pytest.mark.parametrize("name", ["fin", "corner"])
def test_chained_select_level_reproduces_seg3d_lossless(name, res, faster, final_level):
    field = orf.FIELDS[name]
    for balance in (0.5, 0.3):
        stats, rounds = [], []
        evaluated = np.zeros((res[-1],) * 3, bool)
        want = po.seg3d_lossless(field, B_MIN, B_MAX, res, balance_value=balance, stats=stats, rounds=rounds,
                                 evaluated_out=evaluated, faster=faster, final_level=final_level)
        got, g_stats, g_rounds, g_ev = chain_levels(field, res, balance, faster, final_level)
        assert g_stats == stats and g_rounds == rounds
        if name == "fin" and res[0] == 2:  # the eight corners of the box are outside: both stop after level 0
            assert want is None and got is None
            continue
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(g_ev, evaluated)


def test_fin_field_reaches_faces_and_needs_conflict_rounds():
    stats, rounds = [], []
    vol = po.seg3d_lossless(orf.fin_field, B_MIN, B_MAX, FIN_RES, stats=stats)
    assert orf.faces_reached(vol > np.float32(0.5)) >= 4
    slow = po.seg3d_lossless(orf.fin_field, B_MIN, B_MAX, FIN_RES, rounds=rounds, faster=False)
    assert max(rounds) >= 2, rounds
    assert orf.faces_reached(slow > np.float32(0.5)) >= 4
    vol = po.seg3d_lossless(orf.fin_field, B_MIN, B_MAX, [12, 23, 45, 89])
    assert orf.faces_reached(vol > np.float32(0.5)) >= 4


def test_corner_field_is_not_empty_at_two_nodes_per_side():
    res = [2, 3, 5, 9, 17, 33]
    level0 = po.dense_volume(orf.corner_field, B_MIN, B_MAX, 2, 33)
    assert (level0 > np.float32(0.5)).any() and not (level0 > np.float32(0.5)).all()
    stats = []
    vol = po.seg3d_lossless(orf.corner_field, B_MIN, B_MAX, res, stats=stats)
    assert vol is not None and len(stats) == 6 and min(stats) > 0
    assert np.array_equal(vol > np.float32(0.5), po.dense_volume(orf.corner_field, B_MIN, B_MAX, 33) > np.float32(0.5))


@pytest.mark.parametrize("rp", [64, 65, 66])
def test_seam_volumes_select_across_the_word_boundary(rp):
    """Boxes 9, 7 and 3 select nodes at x = 63 that have a flag of their box in word 1 and nodes at x = 64 that have
    one in word 0.  At x = 64 some are selected ONLY through word 0 (the carry into the word) for every box, at
    x = 63 ONLY through word 1 for the boxes 9 and 7.  For box 3 no input can do that: a flag at x = 64 (mask strictly
    between 0 and 1) makes mask(63) = (mask(62) + mask(64)) / 2 of the same row lie strictly between 0 and 1 too."""
    prev, ev_prev = orf.seam(rp, rp)
    for box in (9, 7, 3):
        _, flags, sel, _ = orf.select_level(prev, ev_prev, box)
        lo, hi = flags.copy(), flags.copy()
        lo[:, :, 64:] = False
        hi[:, :, :64] = False
        assert lo.any() and hi.any()
        from_lo, from_hi = po.dilate_box(lo, box), po.dilate_box(hi, box)
        assert (sel & from_hi)[:, :, 63].any() and (sel & from_lo)[:, :, 64].any(), box
        assert (sel & from_lo & ~from_hi)[:, :, 64].any(), box
        if box != 3:
            assert (sel & from_hi & ~from_lo)[:, :, 63].any(), box
        if rp == 65:  # the second boundary, next to the last parent node
            assert sel[:, :, 127].any() and sel[:, :, 128].any(), box


@pytest.mark.parametrize("rp", [2, 3, 5, 12, 32, 33])
def test_plateau_selection_depends_on_the_strict_comparison(rp):
    prev, ev_prev = orf.plateau(rp, rp)
    above = np.nextafter(np.float32(0.5), np.float32(1))
    assert (prev == np.float32(0.5)).any() and (prev == above).any()
    for box in (9, 7, 3, 1):
        a = orf.select_level(prev, ev_prev, box, 0.5)
        b = orf.select_level(prev, ev_prev, box, float(above))
        assert not np.array_equal(a[1], b[1]), box
        if rp >= 12 or box == 1:  # a small volume is inside the 9^3 box of any flag
            assert not np.array_equal(a[2], b[2]), box


@pytest.mark.parametrize("name", ["noise", "faces", "sparse", "plateau"])
def test_volume_builders_are_seeded_and_not_trivial(name):
    for rp in (2, 3, 5, 12, 32, 33):
        prev, ev_prev = orf.VOLUMES[name](rp, 7)
        again, ev_again = orf.VOLUMES[name](rp, 7)
        assert prev.dtype == np.float32 and prev.shape == (rp, rp, rp) and ev_prev.dtype == bool
        assert np.array_equal(prev.view(np.uint32), again.view(np.uint32)) and np.array_equal(ev_prev, ev_again)
        with np.errstate(invalid="ignore"):
            inside = prev > np.float32(0.5)
        assert inside.any() and not inside.all()
        if rp >= 5:
            assert 0 < ev_prev.sum() < rp ** 3
            _, flags, sel, ev_after = orf.select_level(prev, ev_prev, 3)
            assert flags.any() and sel.any()
            if rp >= 12:  # nodes in reach of a flag that were evaluated one level up, and some that were not
                even = np.zeros(sel.shape, bool)
                even[::2, ::2, ::2] = True
                reach = po.dilate_box(flags, 3)
                assert (reach & orf.even_image(ev_prev)).any() and (sel & even).any()
    prev, _ = orf.noise(33, 1)
    assert np.isnan(prev).sum() > 30 and abs((prev > 0.5).mean() - 0.03) < 0.005
    prev, _ = orf.faces(33, 1)
    inside = prev > np.float32(0.5)
    assert all(inside.take(i, a).sum() > 100 for a, i in ((0, 0), (1, -1), (2, 0), (2, -1)))
    assert not inside[1:, :-1, 1:-1].any()


def test_bit_helpers_round_trip():
    rng = np.random.default_rng(5)
    for r in (3, 63, 64, 65, 131):
        mask = rng.random((r, r, r)) < 0.3
        words = orf.pack_bits(mask)
        assert words.dtype == np.uint64 and words.size == r * r * ((r + 63) // 64)
        back, pad = orf.unpack_bits(words, r)
        assert np.array_equal(back, mask) and not pad.any()
        z, y, x = np.nonzero(mask)
        assert np.array_equal(orf.mask_codes(mask), np.sort(x | (y << 10) | (z << 20)))
