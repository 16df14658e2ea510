"""The inputs of tests/test_surface_cases_gpu.py hold what they are meant to hold, and the oracle they are compared
with is pinned: oracle.forward_vertices to the reference's own forward_vertices on those inputs
(tests/golden/forward_vertices_edges.npz, written by oracle/gen_golden.py gen_forward_vertices_edges), and
oracle.marching_cubes to the float64 crossing and to the case table.  No GPU needed."""
import numpy as np
import pytest

import surface_cases as sc
from conftest import load_golden
from test_box_threshold_cpu import B_MAX, B_MIN, mc_f64_tolerance, mc_verts_f64

K_SEG = 32  # csrc/vertices.hip: kSeg, the voxels of a column one thread scans
UNIT = (np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32))


# ---------------------------------------------------------------------------------------------------------------
# what the inputs contain
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,least", [(13, 1), (17, 3)])
def test_noise_volumes_hold_all_256_cases(r, least):
    n = np.bincount(sc.corner_cases(sc.noise_volume(r, sc.NOISE[r])).ravel(), minlength=256)
    print("noise%d: rarest case occurs %d times" % (r, n.min()))
    assert (n >= least).all()


def test_smooth_bodies_miss_most_cases():
    """Why the noise is needed: the blob of the other marching-cubes tests reaches fewer than half of the cases."""
    from monoport_amd import synthetic as syn
    assert len(np.unique(sc.corner_cases(syn.blob_volume(33, 5)))) < 128


def test_quarters_volume_has_nodes_at_every_level():
    vol = sc.quarters_volume(*sc.QUARTERS)
    assert set(np.unique(vol).tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}
    for level in (0.25, 0.5, 0.75):
        assert (vol == np.float32(level)).sum() > 900, level


def test_one_cell_volumes_are_their_cases():
    vols = sc.one_cell_volumes()
    assert vols.shape == (256, 2, 2, 2)
    for case in range(256):
        assert int(sc.corner_cases(vols[case])[0, 0, 0]) == case
    assert ((vols > 0.5) | (vols < 0.5)).all() and vols.min() >= 0 and vols.max() <= 1


def test_nonfinite_volume_has_all_three_kinds():
    vol = sc.nonfinite_volume(*sc.NONFINITE)
    assert np.isnan(vol).sum() >= 90 and np.isposinf(vol).sum() >= 90 and np.isneginf(vol).sum() >= 90


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("r", [40, 65])
def test_depth_volume_reaches_borders_segments_and_plateaus(oracle, r, kind):
    vol, d = sc.depth_case(r, kind)
    s = vol[::-1].transpose(2, 1, 0)  # s[x, y, z']
    zp = np.arange(r)[None, None, :]
    assert (s[zp < d[:, :, None]] <= 0.5).all()
    xs, ys = np.nonzero(d < r)
    assert (s[xs, ys, d[xs, ys]] > 0.5).all()
    x, y, z, n = oracle.forward_vertices(vol, "front")
    assert np.array_equal(np.stack([xs, ys], 1), np.stack([x, y], 1))  # the oracle finds exactly these hits
    z1 = d[xs, ys]
    assert (xs < 2).sum() >= 50 and (ys < 2).sum() >= 50 and (z1 < 2).sum() >= 50
    assert (z1 == r - 1).sum() >= r - 2  # row x = 5: the last voxel only
    seg = np.bincount(z1 // K_SEG, minlength=(r + K_SEG - 1) // K_SEG)
    print("depth%d %s: hits per segment %s, no hit %d, NaN Z %d of %d" % (r, kind, seg.tolist(), (d == r).sum(),
                                                                        np.isnan(z).sum(), len(z)))
    assert (seg >= 100).all()
    assert (d == r).sum() >= 20
    assert np.isfinite(z).mean() >= 0.9
    assert (np.isnan(z) == (z1 == 0)).all()  # 0/0 at the front face and nowhere else
    if kind == "binary":
        # all three differences zero, 0/0 in every component: a few rows from the front (a hit at z' = 0 whose two
        # neighbours hit there too), and from the back, where 70 % of the far face is 1, about a third of all rows
        assert np.isnan(n).all(1).sum() > 0
        nb = oracle.forward_vertices(vol, "back")[3]
        assert np.isnan(nb).all(1).sum() >= 100 and np.array_equal(np.isnan(nb).all(1), np.isnan(nb).any(1))
    if kind == "quant":
        z2 = np.clip(z1 - 2, 0, r)
        assert (s[xs, ys, z2] == 0.5).sum() >= 100  # 0.5 itself right in the interpolation, and it is no hit


# ---------------------------------------------------------------------------------------------------------------
# oracle.forward_vertices against the reference's own forward_vertices
# ---------------------------------------------------------------------------------------------------------------
SMOOTH_NORMAL_BOUND = 2.4e-7  # twice the 1.2e-7 measured: torch.norm sums the three squares in another order than
#                               the written one, and one rounding of the length moves a component by <= 1 ulp of 1


def _edge_cases():
    out = [("d40_%s" % kind, kind, d) for kind in sc.KINDS for d in sc.DIRECTIONS]
    return out + [("nonfinite", "nonfinite", d) for d in ("front", "left")]


@pytest.fixture(scope="module")
def edge_volumes():
    vols = {"d40_%s" % kind: sc.depth_case(40, kind)[0] for kind in sc.KINDS}
    vols["nonfinite"] = sc.nonfinite_volume(*sc.NONFINITE)
    return vols


@pytest.mark.parametrize("name,kind,direction", _edge_cases())
def test_oracle_forward_vertices_is_the_reference_on_the_edges(oracle, edge_volumes, name, kind, direction):
    g = load_golden("forward_vertices_edges")
    key = "%s_%s_" % (name, direction)
    x, y, z, n = oracle.forward_vertices(edge_volumes[name], direction)
    assert len(x) > 300
    assert np.array_equal(x, g[key + "X"]) and np.array_equal(y, g[key + "Y"])
    sc.same_bits(z, g[key + "Z"], key + "Z")
    want = g[key + "norm"]
    assert np.array_equal(np.isnan(n), np.isnan(want))
    ok = ~np.isnan(want)
    err = float(np.abs(n[ok] - want[ok]).max())
    print("%s %s: normals differ from the reference by at most %.3g" % (name, direction, err))
    if kind in ("binary", "quant"):
        sc.same_bits(n, want, key + "norm")
    else:
        assert err <= SMOOTH_NORMAL_BOUND


# ---------------------------------------------------------------------------------------------------------------
# oracle.marching_cubes on every case
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", ["unit", "B"])
@pytest.mark.parametrize("r", [13, 17])
def test_marching_cubes_oracle_on_noise_vs_float64(oracle, r, box):
    bmin, bmax = UNIT if box == "unit" else (B_MIN, B_MAX)
    vol = sc.noise_volume(r, sc.NOISE[r])
    v, f = oracle.marching_cubes(vol, 0.5, bmin, bmax)
    w = mc_verts_f64(vol, 0.5, bmin, bmax)
    assert v.shape == w.shape and len(v) > 1000 and f.min() == 0 and f.max() == len(v) - 1
    err = float(np.abs(v - w).max())
    print("noise%d %s: %d vertices within %.3g of float64 (tolerance %.3g)"
          % (r, box, len(v), err, mc_f64_tolerance(bmin, bmax)))
    assert err <= mc_f64_tolerance(bmin, bmax)


def test_marching_cubes_oracle_on_every_single_cell(oracle):
    """Case c gives count[c] faces and one vertex per edge of the cell whose ends lie on different sides, every face
    names three different vertices, and the vertices are the float64 crossings."""
    t = oracle._mc_tables()
    vols = sc.one_cell_volumes()
    faces = 0
    for case in range(256):
        v, f = oracle.marching_cubes(vols[case])
        ins = (vols[case] > 0.5).reshape(-1)
        crossing = sum(int(ins[a] != ins[b]) for a, b in t["edges"])
        assert len(f) == t["count"][case] and len(v) == crossing, case
        if len(f):
            assert f.min() >= 0 and f.max() < len(v), case
            assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all(), case
            assert len(np.unique(f)) == len(v), case  # every crossing edge is used
            assert np.abs(v - mc_verts_f64(vols[case], 0.5, *UNIT)).max() <= mc_f64_tolerance(*UNIT), case
        faces += len(f)
    assert faces == int(t["count"].sum()) == 820
