"""The inputs of tests/test_box_threshold_gpu.py can tell a right kernel from a wrong one (no GPU needed).

Every other test runs the octree, the lattice, marching cubes and the colour matrix on the box [-1, 1]^3 with the
thresholds 0.5.  There ``u * 2`` is exact, all three axes share b_min and length, and 0.5 is the only threshold:
an axis mix-up, a reordered rounding or a literal 0.5 in place of ``balance`` / ``level`` gives the same bits.
Box B below has three different corners and three different lengths, none a power of two; the thresholds are
0.3 / 0.5 / 0.7.  Here the CPU restatements in oracle/ show that on these inputs each such slip changes the result.
"""
import numpy as np
import pytest

from monoport_amd import synthetic as syn

B_MIN = np.array([-0.83, -1.17, -0.61], np.float32)
B_MAX = np.array([0.97, 1.06, 1.27], np.float32)
BALANCES = (0.3, 0.5, 0.7)
SWAP_XZ = [2, 1, 0]
# the off-centre ellipsoid of the generic-engine tests (float32 numpy sigmoid)
ELL_CENTRE = np.array([0.21, -0.13, 0.34], np.float32)
ELL_RADII = np.array([0.47, 0.63, 0.39], np.float32)
ELL_SHARP = np.float32(6.0)


def ellipsoid_np(p, amplitude=1.0):
    """[3,N] f32 -> [N] f32: amplitude * sigmoid(k (1 - |(p - c) / radii|)), every step in float32."""
    p = np.asarray(p, np.float32)
    q = (p - ELL_CENTRE[:, None]) / ELL_RADII[:, None]
    d = np.sqrt((q * q).sum(0, dtype=np.float32)).astype(np.float32)
    s = (np.float32(1) / (np.float32(1) + np.exp(-ELL_SHARP * (np.float32(1) - d)))).astype(np.float32)
    return (np.float32(amplitude) * s).astype(np.float32)


def all_idx(r):
    return np.stack(np.meshgrid(np.arange(r), np.arange(r), np.arange(r), indexing="ij"), -1).reshape(-1, 3)


def lattice_f64(idx_zyx, stride, rf, b_min, b_max):
    """((c / R) + 1/(2R)) * len + b_min in float64 from the f32 box: [3,N]."""
    bmin = np.asarray(b_min, np.float32).astype(np.float64)
    blen = (np.asarray(b_max, np.float32) - np.asarray(b_min, np.float32)).astype(np.float64)
    out = np.empty((3, idx_zyx.shape[0]), np.float64)
    for axis, col in ((0, 2), (1, 1), (2, 0)):
        c = idx_zyx[:, col].astype(np.float64) * stride
        out[axis] = (c / rf + 0.5 / rf) * blen[axis] + bmin[axis]
    return out


def test_box_b_is_off_centre_and_not_dyadic():
    blen = B_MAX - B_MIN
    assert len(set(B_MIN.tolist())) == 3 and len(set(blen.tolist())) == 3
    for v in blen:
        m, _ = np.frexp(np.float32(v))
        assert m != 0.5, "length %r is a power of two" % v
    # a permutation or a shared length really changes the box
    assert not np.array_equal(B_MIN[SWAP_XZ], B_MIN) and not np.array_equal(blen[SWAP_XZ], blen)


def test_box_b_holds_the_body_and_reaches_outside_the_image(oracle):
    """The body of the GPU tests lies inside B (recon non-empty, nothing occupied on the box faces), and a visible
    share of the level-0 nodes projects outside the image (those must come out exactly 0)."""
    calib = oracle.pifu_calib(*syn.scene_camera(30))
    p = oracle.lattice_points(all_idx(17), 8, 129, B_MIN, B_MAX)
    xyz = oracle.orthogonal(p, calib[0])
    outside = (np.abs(xyz[0]) > 1) | (np.abs(xyz[1]) > 1)
    assert outside.mean() >= 0.01
    layers = syn.body_mlp("G", noise=0.05, seed=1)
    f = syn.body_feat(256, 128, 128, 2)
    q = lambda pts: oracle.query(f, pts, calib[0], layers, 1, syn.Z_SCALE, precision="f32")[0]
    assert (q(p)[outside] == 0).all()
    for b in BALANCES:
        vol = oracle.seg3d_lossless(q, B_MIN, B_MAX, [17, 33], balance_value=b)
        assert vol is not None
        occ = vol > np.float32(b)
        assert occ.sum() > 100
        for axis in range(3):
            assert not occ.take(0, axis).any() and not occ.take(-1, axis).any(), (b, axis)


@pytest.mark.parametrize("stride", [1, 8])
def test_lattice_points_on_box_b(oracle, stride):
    """oracle.lattice_points on B at R = 129 against the float64 lattice: within 1.25 ulp of the largest of |u len|,
    |b_min| and the result (u = c/R + 1/(2R) and the product are rounded before b_min is added, so near a
    cancelling b_min the result's own ulp is no bar: measured 1.22).  A permuted box or one length or corner for
    every axis moves coordinates."""
    rf = 129
    r = (rf - 1) // stride + 1
    idx = all_idx(r)
    if stride == 1:
        idx = idx[np.random.RandomState(5).choice(idx.shape[0], 300000, replace=False)]
    got = oracle.lattice_points(idx, stride, rf, B_MIN, B_MAX)
    want = lattice_f64(idx, stride, rf, B_MIN, B_MAX)
    blen = (B_MAX - B_MIN).astype(np.float64)
    mag = np.maximum(np.abs(want - B_MIN.astype(np.float64)[:, None]), np.abs(B_MIN.astype(np.float64))[:, None])
    ulp = np.spacing(np.maximum(mag, np.abs(want)).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want) <= 1.25 * ulp).all()
    assert (blen > 0).all()
    swapped = oracle.lattice_points(idx, stride, rf, B_MIN[SWAP_XZ], B_MAX[SWAP_XZ])
    assert (swapped[0] != got[0]).mean() > 0.9 and (swapped[2] != got[2]).mean() > 0.9
    for a, b in ((0, 1), (1, 2)):
        perm = [0, 1, 2]
        perm[a], perm[b] = b, a
        assert not np.array_equal(oracle.lattice_points(idx, stride, rf, B_MIN[perm], B_MAX[perm]), got)
    # one length (x's) for all three axes, every step in f32 as the kernels do it
    r32 = np.float32(rf)
    half = np.float32(np.float32(1) / r32) / np.float32(2)
    one_len = np.empty_like(got)
    for axis, col in ((0, 2), (1, 1), (2, 0)):
        u = ((idx[:, col] * stride).astype(np.float32) / r32 + half).astype(np.float32)
        one_len[axis] = (u * (B_MAX[0] - B_MIN[0]) + B_MIN[axis]).astype(np.float32)
    assert np.array_equal(one_len[0], got[0])
    assert (one_len[1] != got[1]).mean() > 0.9 and (one_len[2] != got[2]).mean() > 0.9
    # one corner (x's) for all three axes
    assert (got[1] - B_MIN[1] + B_MIN[0] != got[1]).mean() > 0.9


@pytest.mark.parametrize("r", [65, 129, 257])
def test_color_matrix_on_box_b(oracle, r):
    from monoport_amd.recon import color_matrix
    m = color_matrix(B_MIN, B_MAX, r)
    assert m.dtype == np.float32 and np.array_equal(m, oracle.color_matrix(B_MIN, B_MAX, r))
    d = np.diag(m)[:3]
    assert len(set(d.tolist())) == 3 and len(set(m[:3, 3].tolist())) == 3
    assert np.array_equal(m[:3, 3], B_MIN)
    assert not np.array_equal(m, m.T)  # a transposed matrix loses the translation


RES_E = [9, 17, 33, 65]


def test_octree_threshold_and_box_discriminate(oracle):
    """oracle.seg3d_lossless on the off-centre ellipsoid: the three balances give different per-level counts and
    different thresholded volumes; the box with x and z swapped gives another volume."""
    vols, stats = {}, {}
    for b in BALANCES:
        st = []
        v = oracle.seg3d_lossless(ellipsoid_np, B_MIN, B_MAX, RES_E, balance_value=b, stats=st)
        assert v is not None
        vols[b], stats[b] = v, st
        occ = v > np.float32(b)
        assert occ.sum() > 1000 and not occ[0].any() and not occ[-1].any()
    assert len({tuple(s) for s in stats.values()}) == 3
    occs = [vols[b] > np.float32(b) for b in BALANCES]
    assert not np.array_equal(occs[0], occs[1]) and not np.array_equal(occs[1], occs[2])
    # the 0.5 schedule thresholded at 0.3 is not the 0.3 schedule: a literal 0.5 for balance shows in the values
    assert not np.array_equal(vols[0.3], vols[0.5])
    swapped = oracle.seg3d_lossless(ellipsoid_np, B_MIN[SWAP_XZ], B_MAX[SWAP_XZ], RES_E, balance_value=0.3)
    assert swapped is not None and not np.array_equal(swapped, vols[0.3])
    # the faster=False schedule (conflict re-examination) also depends on the balance
    st3, st7 = [], []
    oracle.seg3d_lossless(ellipsoid_np, B_MIN, B_MAX, RES_E, balance_value=0.3, stats=st3, faster=False)
    oracle.seg3d_lossless(ellipsoid_np, B_MIN, B_MAX, RES_E, balance_value=0.7, stats=st7, faster=False)
    assert st3 != st7


def test_level0_maximum_between_thresholds(oracle):
    """A field whose level-0 maximum lies in (0.5, 0.7): empty (None) at 0.7, a volume at 0.5."""
    field = lambda p: ellipsoid_np(p, amplitude=0.66)
    lv0 = field(oracle.lattice_points(all_idx(RES_E[0]), 8, RES_E[-1], B_MIN, B_MAX))
    assert 0.5 < lv0.max() < 0.7
    assert oracle.seg3d_lossless(field, B_MIN, B_MAX, RES_E, balance_value=0.7) is None
    assert oracle.seg3d_lossless(field, B_MIN, B_MAX, RES_E, balance_value=0.5) is not None


def ellipsoid_volume(r):
    return ellipsoid_np(oracle_lattice(r)).reshape(r, r, r)


def oracle_lattice(r):
    from oracle import pifu_oracle
    return pifu_oracle.lattice_points(all_idx(r), 1, r, B_MIN, B_MAX)


def test_marching_cubes_level_and_box_discriminate(oracle):
    vol = ellipsoid_volume(33)
    counts = set()
    for level in BALANCES:
        v, f = oracle.marching_cubes(vol, level, B_MIN, B_MAX)
        assert len(v) > 100
        counts.add((len(v), len(f)))
    assert len(counts) == 3
    v, f = oracle.marching_cubes(vol, 0.3, B_MIN, B_MAX)
    vs, fs = oracle.marching_cubes(vol, 0.3, B_MIN[SWAP_XZ], B_MAX[SWAP_XZ])
    assert np.array_equal(f, fs) and not np.allclose(v, vs, atol=1e-3)
    # one length for every axis
    vx, _ = oracle.marching_cubes(vol, 0.3, B_MIN, B_MIN + (B_MAX[0] - B_MIN[0]))
    assert np.array_equal(vx[:, 0], v[:, 0]) and not np.allclose(vx[:, 1:], v[:, 1:], atol=1e-3)


def mc_verts_f64(vol, level, b_min, b_max):
    """Vertex positions of oracle.marching_cubes' edge order in float64 from the f32 volume."""
    vol = np.asarray(vol, np.float32)
    r = vol.shape[0]
    inside = vol > np.float32(level)
    cross = np.zeros((r, r, r, 3), bool)
    cross[:, :, :-1, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    cross[:, :-1, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    cross[:-1, :, :, 2] = inside[:-1, :, :] != inside[1:, :, :]
    zz, yy, xx, aa = np.nonzero(cross)
    va = vol[zz, yy, xx].astype(np.float64)
    vb = vol[zz + (aa == 2), yy + (aa == 1), xx + (aa == 0)].astype(np.float64)
    t = (np.float64(np.float32(level)) - va) / (vb - va)
    pos = np.stack([xx, yy, zz], 1).astype(np.float64)
    pos[np.arange(len(pos)), aa] += t
    bmin = np.asarray(b_min, np.float32).astype(np.float64)
    blen = (np.asarray(b_max, np.float32) - np.asarray(b_min, np.float32)).astype(np.float64)
    return (pos / r + 0.5 / r) * blen + bmin


def mc_f64_tolerance(b_min, b_max, ulps=4):
    """A few ulp of the largest coordinate magnitude of the box."""
    return ulps * float(np.spacing(np.float32(max(np.abs(b_min).max(), np.abs(b_max).max()))))


def test_marching_cubes_oracle_vs_float64(oracle):
    """The f32 vertex arithmetic stays within a few ulp of |B| of the float64 crossing (the bar the GPU file uses)."""
    vol = ellipsoid_volume(65)
    for level in (0.3, 0.7):
        v, _ = oracle.marching_cubes(vol, level, B_MIN, B_MAX)
        w = mc_verts_f64(vol, level, B_MIN, B_MAX)
        assert v.shape == w.shape and len(v) > 1000
        assert np.abs(v - w).max() <= mc_f64_tolerance(B_MIN, B_MAX)
