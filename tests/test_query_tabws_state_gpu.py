"""The per-lane point state of the skip-table query kernel (csrc/query_table.hip: a producer lane's tap offsets,
weights, depth, layer-4 row, scatter code and flags, carried through three tiles as next / current / previous):
the table path against the plain fused kernels on the same inputs, at the shapes where that state can go wrong.
The bound is the one tests/test_query_gpu.py::test_skip_table_* hold the two paths to (2e-6: the same products
summed in another order); points outside the image are exactly 0 and non-finite results sit at the same places.
Needs an MI355X."""
import numpy as np
import pytest

from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
TOL_PATHS = 2e-6  # |table path - plain path|, tests/test_query_gpu.py::test_skip_table_registry_semantics
FH, FW = 24, 16   # 384 texels = 6 table tiles of 64: a small, non-square map


@pytest.fixture(scope="module")
def scene():
    """Heads with Cout 1 (sigmoid) and 3 (tanh) on one 256-channel map, and the map's skip table per head (made on
    request, dropped with the module)."""
    from monoport_amd import ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    heads = {}
    for cout in (1, 3):
        layers = syn.rand_mlp("G", 31 + cout, 2.0)
        if cout == 3:
            rs = np.random.RandomState(5)
            w4 = layers[-1][0]
            layers[-1] = (rs.uniform(-0.1, 0.1, (3, w4.shape[1])).astype(np.float32),
                          rs.uniform(-0.1, 0.1, (3,)).astype(np.float32))
        heads[cout] = ops.PackedMLP.from_layers(DEV, layers, 1 if cout == 1 else 2)
    fh = ops.pack_features(torch.from_numpy(syn.rand_feat(256, FH, FW, 6))[None].to(DEV))
    yield {"ops": ops, "heads": heads, "fh": fh}
    for mlp in heads.values():
        ops.skip_table_release(mlp.ctx)


def both_paths(scene, cout, run):
    """run(mlp, fh) on the plain kernels, then through the registered skip table -> (plain, table) as numpy."""
    ops, mlp, fh = scene["ops"], scene["heads"][cout], scene["fh"]
    ops.skip_table_release(mlp.ctx)
    plain = run(mlp, fh)
    table = ops.skip_table(mlp, fh)
    try:
        tab = run(mlp, fh)
        torch.cuda.synchronize()
    finally:
        table.release()
    return plain, tab


def assert_same_field(tab, plain, what=""):
    tab, plain = np.asarray(tab), np.asarray(plain)
    assert tab.shape == plain.shape, what
    bad_t, bad_p = ~np.isfinite(tab), ~np.isfinite(plain)
    assert np.array_equal(np.isnan(tab), np.isnan(plain)), what
    assert np.array_equal(bad_t, bad_p), what
    ok = ~bad_p
    err = float(np.abs(tab[ok] - plain[ok]).max()) if ok.any() else 0.0
    print("%s: max |table - plain| = %.3g over %d values" % (what, err, int(ok.sum())))
    assert err <= TOL_PATHS, what


def calib_eye(sx=1.0, sy=1.0):
    cal = np.eye(4, dtype=np.float32)[None]
    cal[0, 0, 0], cal[0, 1, 1] = sx, sy
    return torch.from_numpy(cal).to(DEV)


def query_np(ops, mlp, fh, pts, cal, projection="orthogonal"):
    p = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32))[None].to(DEV)
    return ops.query(mlp, fh, p, cal, syn.Z_SCALE, projection=projection)[0].cpu().numpy()


@pytest.mark.parametrize("cout", [1, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_points_per_frame(scene, cout, n):
    """One frame of n explicit points: less than a tile, one short of it, a full tile, one over, two and a bit."""
    ops = scene["ops"]
    pts = syn.rand_points(n, 300 + n, 1.05)
    pts[:, 0] = (0.3, -0.2, 0.1)  # the first point is inside the image whatever the seed
    cal = calib_eye(0.93, 0.97)
    plain, tab = both_paths(scene, cout, lambda mlp, fh: query_np(ops, mlp, fh, pts, cal))
    assert plain.shape == (cout, n) and np.abs(plain[:, 0]).min() > 0
    if n >= 31:
        assert not np.array_equal(tab, plain)  # the table kernel really ran
    assert_same_field(tab, plain, "n=%d cout=%d" % (n, cout))


def counted_batch(ops, mlp, fh, pts_all, counts, cals, projections=None):
    cap = pts_all[0].shape[1]
    n = len(counts)
    pts = [torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).to(DEV).contiguous() for p in pts_all]
    cnts = [torch.tensor([c], dtype=torch.int32, device=DEV) for c in counts]
    outs = ops.query_counted_batch(mlp, [fh] * n, pts, cnts, cals, syn.Z_SCALE, projections=projections)
    assert all(tuple(o.shape) == (mlp.cout, cap) for o in outs)
    return np.stack([o.cpu().numpy() for o in outs])


@pytest.mark.parametrize("cout", [1, 3])
@pytest.mark.parametrize("counts", [(33, 0, 1), (24577, 0, 1, 24000)], ids=["33-0-1", "three-tiles-per-workgroup"])
def test_frames_with_device_counts(scene, cout, counts):
    """Several frames in one launch, the counts on the device: a frame of a tile plus one point, an empty frame and
    a frame of one point.  The second case has some 1500 tiles for the 512 resident workgroups, so every workgroup
    walks through about three tiles -- both tile parities, the next / current / previous rotation of the point
    state, and for some workgroups the change of frame (across the empty one) between two of its tiles."""
    ops = scene["ops"]
    cap = max(counts) + 7
    pts_all = [syn.rand_points(cap, 400 + i, 1.05) for i in range(len(counts))]
    cals = [calib_eye(1.0 - 0.03 * i, 0.9 + 0.02 * i) for i in range(len(counts))]
    plain, tab = both_paths(scene, cout, lambda mlp, fh: counted_batch(ops, mlp, fh, pts_all, counts, cals))
    for i, c in enumerate(counts):
        assert_same_field(tab[i][:, :c], plain[i][:, :c], "frame %d of %s cout=%d" % (i, counts, cout))
        assert (tab[i][:, c:] == 0).all() and (plain[i][:, c:] == 0).all()  # beyond the count: never written
        if c:
            assert np.abs(tab[i][:, :c]).max() > 0
    assert not np.array_equal(tab, plain)


def border_points():
    """Points whose four taps touch every border and corner of the map, sit exactly on texels, fall just inside
    and just outside the image, and far outside: the cross product of such x and y (identity calibration)."""
    eps = np.float32(2.0 ** -23)
    tex_x, tex_y = np.float32(2.0 / (FW - 1)), np.float32(2.0 / (FH - 1))
    def axis(tex):
        return np.array([-1.0, -1.0 + eps, -1.0 + 0.5 * tex, -1.0 + tex, 0.0, 0.37, 1.0 - tex, 1.0 - 0.5 * tex,
                         1.0 - eps, 1.0, -1.0 - 2 * eps, 1.0 + 2 * eps, -1.5, 3.0], np.float32)
    xs, ys = axis(tex_x), axis(tex_y)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    rs = np.random.RandomState(9)
    pts = np.stack([gx.ravel(), gy.ravel(), rs.uniform(-1, 1, gx.size).astype(np.float32)])
    inside = (np.abs(pts[0]) <= 1.0) & (np.abs(pts[1]) <= 1.0)
    return pts.astype(np.float32), inside


@pytest.mark.parametrize("cout", [1, 3])
def test_taps_on_borders_corners_and_outside(scene, cout):
    ops = scene["ops"]
    pts, inside = border_points()  # 196 points: seven tiles, the last one short
    assert inside.sum() == 100
    cal = calib_eye()
    plain, tab = both_paths(scene, cout, lambda mlp, fh: query_np(ops, mlp, fh, pts, cal))
    assert_same_field(tab, plain, "borders cout=%d" % cout)
    assert (tab[:, ~inside] == 0).all() and (plain[:, ~inside] == 0).all()  # MonoPortNet.py:89: exactly 0
    assert (np.abs(tab[:, inside]) > 0).all()


@pytest.mark.parametrize("cout", [1, 3])
def test_non_finite_coordinates(scene, cout):
    """NaN and +-inf in x, y or z among ordinary points, on an orthogonal and on a perspective frame (where z = 0
    also projects to +-inf / NaN): the same values, zeros and NaNs as the plain kernels, and the neighbours of
    such a point in its tile are not disturbed."""
    ops = scene["ops"]
    n = 70
    pts = syn.rand_points(n, 77, 0.9)
    pts[2] = np.abs(pts[2]) + 0.5  # a positive depth for the perspective frame
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for k, (axis, v) in enumerate([(0, nan), (1, nan), (2, nan), (0, inf), (0, -inf), (1, inf), (1, -inf), (2, inf),
                                   (2, -inf), (2, 0.0)]):
        pts[axis, 3 + 6 * k] = v  # spread over the three tiles, ordinary points in between
    special = np.zeros(n, bool)
    special[3:3 + 6 * 10:6] = True
    cal = calib_eye(0.8, 0.8)
    for projection in ("orthogonal", "perspective"):
        plain, tab = both_paths(scene, cout, lambda mlp, fh: query_np(ops, mlp, fh, pts, cal, projection))
        assert_same_field(tab, plain, "%s cout=%d" % (projection, cout))
        assert np.isfinite(tab[:, ~special]).all() and np.abs(tab[:, ~special]).max() > 0
        if projection == "orthogonal":  # NaN / inf in x or y: not in the image, exactly 0
            assert (tab[:, 3:3 + 6 * 2:6] == 0).all() and (tab[:, 3 + 6 * 3:3 + 6 * 7:6] == 0).all()


def test_lattice_point_lists(scene):
    """The octree's point lists are packed lattice codes (x | y << 10 | z << 20) that the kernel turns into
    coordinates and scatters by: three frames in one reconstruction, every level's launch through the table,
    against the plain kernels (the occupancy head: Cout = 1)."""
    ops = scene["ops"]
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), syn.LAST_OP["G"])
    fh = ops.pack_features(torch.from_numpy(syn.body_feat(256, 64, 64, 2))[None].to(DEV))
    from oracle import pifu_oracle as orc
    cals = [torch.from_numpy(orc.pifu_calib(*syn.scene_camera(s))).to(DEV) for s in (30, 31, 45)]
    res = [9, 17, 33]

    def run():
        vols, status = ops.recon_batch(mlp, [fh] * 3, cals, syn.Z_SCALE, [-1, -1, -1], [1, 1, 1], res)
        return torch.stack(list(vols)).cpu().numpy(), status.cpu().numpy()

    vol_p, st_p = run()
    table = ops.skip_table(mlp, fh)
    try:
        vol_t, st_t = run()
    finally:
        table.release()
        ops.skip_table_release(mlp.ctx)
    assert np.array_equal(st_t, st_p) and (st_p[:, 0] == 1).all()
    assert not np.array_equal(vol_t, vol_p)
    assert_same_field(vol_t, vol_p, "recon_batch 9-17-33 x 3 frames")
