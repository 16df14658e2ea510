"""Multi-view queries (SurfaceClassifier num_views = V > 1, csrc/query_views.hip) against fixtures the reference
produced (tools/gen_golden_query_views.py) and against a float64 model built from ops.index samples.  Needs an
MI355X."""
import ast
import contextlib
import warnings

import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
TOL_REF = 1e-4    # the repository's bar against the reference
TOL_MODEL = 1e-5  # against the float64 model of the same samples
RES = [17, 33, 65]  # Seg3dLossless resolutions of the octree test


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops
    return ops


# ---- inputs of the fixtures (restated from tools/gen_golden_query_views.py, which needs the reference) ----
CHANNELS = {"G": [257, 1024, 512, 256, 128, 1], "C": [513, 1024, 512, 256, 128, 3]}
F, DEPTH = 2.0, 3.0


def persp_calib_yaw(s, c):
    r = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]], np.float64)
    k = np.diag([F, F, 1.0])
    m = np.eye(4)
    m[:3, :3] = k @ r
    m[:3, 3] = k @ np.array([0.0, 0.0, DEPTH])
    return m.astype(np.float32)


def calibs_of(case):
    from oracle import pifu_oracle as orc
    if case["proj"] == "orthogonal":
        return np.stack([orc.pifu_calib(*syn.scene_camera(s))[0] for s in case["steps"]])
    return np.stack([persp_calib_yaw(*sc) for sc in case["yaws"]])


def case_inputs(g):
    """fixture -> (case, layers, [V,C,H,W] maps, [3,N] points, [V,4,4] calibs)."""
    case = ast.literal_eval(str(g["case"][0]))
    kind, mlp = case["kind"], case["mlp"]
    layers = syn.rand_mlp(kind, mlp[1], mlp[2]) if mlp[0] == "rand" else syn.body_mlp(kind, noise=mlp[2], seed=mlp[1])
    mk = syn.rand_feat if case["feat"] == "rand" else syn.body_feat
    f = np.stack([mk(CHANNELS[kind][0] - 1, 128, 128, s) for s in case["feats"]])
    pts = case["pts"]
    if pts[0] == "lattice":
        r = pts[1]
        q = ((np.arange(r, dtype=np.float32) / np.float32(r)) + (np.float32(1.0) / np.float32(r)) / np.float32(2))
        q = q * np.float32(2.0) + np.float32(-1.0)
        zz, yy, xx = np.meshgrid(q, q, q, indexing="ij")
        p = np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)]).astype(np.float32)
    else:
        p = syn.rand_points(pts[1], pts[2], pts[3])
        p[:, :g["special"].shape[1]] = g["special"]
    return case, layers, f, p, calibs_of(case)


@contextlib.contextmanager
def small_gate(mode):
    from monoport_amd import _lib
    lib = _lib.load()
    lib.mp_query_tune(mode)
    try:
        yield
    finally:
        lib.mp_query_tune(-1)


def pack_views(ops, f):
    return [ops.pack_features(torch.from_numpy(np.ascontiguousarray(f[v]))[None].to(DEV)) for v in range(f.shape[0])]


def run_fixture(ops, name):
    g = load_golden(name)
    case, layers, f, p, calibs = case_inputs(g)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP[case["kind"]])
    fh = pack_views(ops, f)
    pts = torch.from_numpy(p)[None].repeat(case["V"], 1, 1).to(DEV)
    out = ops.query_views(mlp, fh, pts, torch.from_numpy(calibs).to(DEV), case["proj"], syn.Z_SCALE).cpu().numpy()
    return g, out


@pytest.mark.parametrize("name", ["query_views_G_ortho", "query_views_G_persp", "query_views_C_ortho"])
def test_query_views_vs_reference(ops, name):
    g, out = run_fixture(ops, name)
    ref = g["out"]
    assert out.shape == ref.shape
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    err = float(np.nanmax(np.abs(out - ref)))
    print("%s: max |d| = %.3g" % (name, err))
    assert err <= TOL_REF
    zero = (ref == 0).all((0, 1))
    assert zero.sum() > 100 and (out[:, :, zero] == 0).all()
    if name.endswith("persp"):
        assert np.isnan(out[:, :, :4]).all() and not np.isnan(out[:, :, 4:]).any()


# ---- float64 model of the same samples ----------------------------------------------------------------------
def model_views(ops, layers, fh, pts, calibs, last_op):
    """[V,Cout,N] float64: ops.index samples (grid_sample, zero padding) of every view, layers 0-2 per view, the view
    means, layers 3-4, last_op, per-view mask (orthogonal)."""
    v_n, n = pts.shape[0], pts.shape[2]
    feats, masks = [], []
    for v in range(v_n):
        xyz = ops.orthogonal(pts[v:v + 1], calibs[v:v + 1])[0]
        s = ops.index(fh[v], xyz[:2])[0].double()
        feats.append(torch.cat([s, (xyz[2:3] * np.float32(syn.Z_SCALE)).double()], 0))
        masks.append(((xyz[0].abs() <= 1) & (xyz[1].abs() <= 1)).double())
    w = [(torch.as_tensor(a).to(DEV).double(), torch.as_tensor(b).to(DEV).double()) for a, b in layers]
    ys = []
    for v in range(v_n):
        y = feats[v]
        for i in range(3):
            y = torch.nn.functional.leaky_relu(w[i][0] @ (y if i == 0 else torch.cat([y, feats[v]], 0)) + w[i][1][:, None])
        ys.append(y)
    y = sum(ys) / v_n
    tmpy = sum(feats) / v_n
    y = torch.nn.functional.leaky_relu(w[3][0] @ torch.cat([y, tmpy], 0) + w[3][1][:, None])
    y = w[4][0] @ torch.cat([y, tmpy], 0) + w[4][1][:, None]
    y = torch.sigmoid(y) if last_op == 1 else torch.tanh(y)
    return torch.stack([m[None] * y for m in masks]).cpu().numpy()


@pytest.mark.parametrize("v_n,n", [(2, 1), (2, 63), (3, 64 * 3 + 1), (4, 20000), (5, 64 * 5 + 1), (8, 63),
                                   (8, 64 * 8 + 1), (3, 1000003)])
def test_query_views_vs_float64_model(ops, v_n, n):
    layers = syn.rand_mlp("G", 300 + v_n, 2.0)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP["G"])
    fh = [ops.pack_features(torch.from_numpy(syn.rand_feat(256, 64, 64, 310 + v))[None].to(DEV)) for v in range(v_n)]
    calibs = torch.from_numpy(np.stack([calibs_of(dict(proj="orthogonal", steps=[37 * v]))[0]
                                        for v in range(v_n)])).to(DEV)
    p = torch.from_numpy(syn.rand_points(n, 320 + v_n, 1.25)).to(DEV)
    pts = p[None].expand(v_n, 3, n)  # stride 0 over the views: any strides are accepted
    out = ops.query_views(mlp, fh, pts, calibs, "orthogonal", syn.Z_SCALE)
    m = n if n < 200000 else 65536  # the model on a prefix (the kernel's grid still strides over all points)
    ref = model_views(ops, layers, fh, pts[:, :, :m].contiguous(), calibs, 1)
    err = float(np.abs(out[:, :, :m].cpu().numpy() - ref).max())
    print("V=%d N=%d: max |d| vs float64 = %.3g" % (v_n, n, err))
    assert err <= TOL_MODEL
    if n >= 200000:  # the tail of the multi-pass grid
        tail = model_views(ops, layers, fh, pts[:, :, n - 4096:].contiguous(), calibs, 1)
        assert float(np.abs(out[:, :, n - 4096:].cpu().numpy() - tail).max()) <= TOL_MODEL


@pytest.mark.parametrize("v_n,n", [(3, 5000), (8, 64 * 8 + 1)])
def test_query_views_distinct_points_per_view(ops, v_n, n):
    """Every view gets its OWN points (one pointer per view in the C-ABI): row v of the reference is view v's
    projection of its own row of points, the means run across the rows of the group.  A kernel that read view 0's
    points for every view, or mixed up the views' points in the z mean or the mask, fails here."""
    layers = syn.rand_mlp("G", 330 + v_n, 2.0)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP["G"])
    fh = [ops.pack_features(torch.from_numpy(syn.rand_feat(256, 64, 64, 340 + v))[None].to(DEV)) for v in range(v_n)]
    calibs = torch.from_numpy(np.stack([calibs_of(dict(proj="orthogonal", steps=[29 * v]))[0]
                                        for v in range(v_n)])).to(DEV)
    pts = torch.from_numpy(np.stack([syn.rand_points(n, 350 + v, 1.25) for v in range(v_n)])).to(DEV)
    pts = pts.permute(0, 2, 1).contiguous().permute(0, 2, 1)  # [V,3,N] with point-major strides
    out = ops.query_views(mlp, fh, pts, calibs, "orthogonal", syn.Z_SCALE).cpu().numpy()
    ref = model_views(ops, layers, fh, pts.contiguous(), calibs, 1)
    err = float(np.abs(out - ref).max())
    print("distinct points V=%d N=%d: max |d| vs float64 = %.3g" % (v_n, n, err))
    assert err <= TOL_MODEL
    # the same points in every view give a different field: the test sees which points each view reads
    same = model_views(ops, layers, fh, pts[:1].expand(v_n, 3, n).contiguous(), calibs, 1)
    assert float(np.abs(same - ref).max()) > 100 * TOL_MODEL


def test_query_views_empty(ops):
    mlp = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("G", 5, 2.0), syn.LAST_OP["G"])
    fh = [ops.pack_features(torch.from_numpy(syn.rand_feat(256, 32, 32, 6 + v))[None].to(DEV)) for v in range(3)]
    out = ops.query_views(mlp, fh, torch.zeros((3, 3, 0), device=DEV), torch.eye(4, device=DEV)[None].expand(3, 4, 4),
                          "orthogonal", syn.Z_SCALE)
    assert out.shape == (3, 1, 0)


@pytest.mark.parametrize("n", [100, 50000])
@pytest.mark.parametrize("projection", ["orthogonal", "perspective"])
def test_one_view_equals_plain_query(ops, n, projection):
    layers = syn.rand_mlp("G", 401, 2.0)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP["G"])
    fh = ops.pack_features(torch.from_numpy(syn.rand_feat(256, 128, 128, 402))[None].to(DEV))
    cal = torch.from_numpy(persp_calib_yaw(0.6, 0.8) if projection == "perspective"
                           else calibs_of(dict(proj="orthogonal", steps=[11]))[0]).to(DEV)
    p = syn.rand_points(n, 403, 1.2)
    p[:, :4] = np.array([[0.0] * 4, [0.0, 0.5, -0.5, 0.25], [-3.75] * 4], np.float32)  # z == 0 under perspective
    pts = torch.from_numpy(p)[None].to(DEV)
    one = ops.query_views(mlp, [fh], pts, cal[None], projection, syn.Z_SCALE)
    for gate in (0, 1):  # the 64-point and the 32-point plain kernels (same bits)
        with small_gate(gate):
            plain = ops.query(mlp, fh, pts, cal, syn.Z_SCALE, projection)
        assert torch.equal(torch.isnan(one), torch.isnan(plain))  # the z == 0 points under perspective
        assert torch.equal(one.nan_to_num(7.0), plain.nan_to_num(7.0))


def test_skip_tables_do_not_change_views(ops):
    g = load_golden("query_views_G_ortho")
    case, layers, f, p, calibs = case_inputs(g)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP["G"])
    fh = pack_views(ops, f)
    pts = torch.from_numpy(p)[None].repeat(3, 1, 1).to(DEV)
    cal = torch.from_numpy(calibs).to(DEV)
    before = ops.query_views(mlp, fh, pts, cal, "orthogonal", syn.Z_SCALE)
    single_before = ops.query(mlp, fh[0], pts[:1], cal[0], syn.Z_SCALE)
    tables = [ops.skip_table(mlp, m) for m in fh]
    try:
        after = ops.query_views(mlp, fh, pts, cal, "orthogonal", syn.Z_SCALE)
        single_table = ops.query(mlp, fh[0], pts[:1], cal[0], syn.Z_SCALE)
    finally:
        for t in tables:
            t.release()
    single_after = ops.query(mlp, fh[0], pts[:1], cal[0], syn.Z_SCALE)
    assert torch.equal(before, after)
    assert torch.equal(single_before, single_after)
    assert float((single_table - single_before).abs().max()) <= 2e-6  # the table kernel ran for one view


def _net(kind, layers, v_n, projection="orthogonal"):
    from monoport_amd.modeling import PIFuNetC, PIFuNetG, geometry, heads
    net = PIFuNetG() if kind == "G" else PIFuNetC()
    ch = heads.PIFuNetGMLP().filter_channels if kind == "G" else heads.PIFuNetCMLP().filter_channels
    net.surface_classifier = heads.SurfaceClassifier(ch, v_n, False, "sigmoid" if kind == "G" else "tanh")
    with torch.no_grad():
        for i, (w, b) in enumerate(layers):
            net.surface_classifier.filters[i].weight.copy_(torch.from_numpy(w)[:, :, None])
            net.surface_classifier.filters[i].bias.copy_(torch.from_numpy(b))
    net.projection = getattr(geometry, projection)
    return net.to(DEV).eval()


def test_monoportnet_query_end_to_end(ops):
    """V images -> netG.filter (synthetic encoder weights) -> query equals ops.query_views on the same maps."""
    v_n = 3
    layers = syn.rand_mlp("G", 501, 2.0)
    net = _net("G", layers, v_n)
    shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
    net.image_filter.load_state_dict(
        {k: torch.from_numpy(v).to(DEV) for k, v in syn.seeded_state_dict(shapes, 71).items()})
    images = torch.from_numpy(np.stack([syn.synthetic_image(510 + v) for v in range(v_n)])).to(DEV)
    calibs = torch.from_numpy(calibs_of(dict(proj="orthogonal", steps=[0, 50, 100]))).to(DEV)
    p = torch.from_numpy(syn.rand_points(20000, 520, 1.1)).to(DEV)
    with torch.no_grad():
        feats = net.filter(images)
        out = net.query(feats, p[None].repeat(v_n, 1, 1), calibs)[0]
        maps = [ops.pack_features(feats[-1][0][v:v + 1]) for v in range(v_n)]
        ref = ops.query_views(net.surface_classifier.packed(), maps, p[None].repeat(v_n, 1, 1), calibs,
                              "orthogonal", syn.Z_SCALE)
    assert out.shape == (v_n, 1, 20000) and torch.equal(out, ref)
    assert (out > 0).any() and (out == 0).any()
    # calibs=None: xyz = points for every view
    with torch.no_grad():
        none = net.query(feats, p[None].repeat(v_n, 1, 1))[0]
        eye = ops.query_views(net.surface_classifier.packed(), maps, p[None].repeat(v_n, 1, 1),
                              torch.eye(4, device=DEV)[None].expand(v_n, 4, 4), "orthogonal", syn.Z_SCALE)
    assert torch.equal(none, eye)


def test_surface_classifier_forward_views(ops):
    g = load_golden("forward_views_G_b2")
    case = ast.literal_eval(str(g["case"][0]))
    rng = np.random.default_rng(case["seed"])
    feat = (rng.standard_normal((case["B"] * case["V"], CHANNELS["G"][0], case["n"])) * case["scale"]).astype(np.float32)
    net = _net("G", syn.rand_mlp("G", case["mlp"][1], case["mlp"][2]), case["V"])
    with torch.no_grad():
        out = net.surface_classifier(torch.from_numpy(feat).to(DEV)).cpu().numpy()
    err = float(np.abs(out - g["out"]).max())
    print("forward_views_G_b2: max |d| = %.3g" % err)
    assert out.shape == g["out"].shape and err <= TOL_REF


def undecided_reach(vals, ambiguous=1e-4):
    """Nodes of the final lattice where two fp32-class evaluations may take different octree decisions (as in
    tests/test_query_batch_persp_gpu.py): the reach of every node within ``ambiguous`` of 0.5 (or NaN)."""
    nl = len(RES)
    spacing = [(RES[-1] - 1) // (r - 1) for r in RES]
    box = [0, 9, 7]
    reach = [spacing[l] + sum((box[m] - 1) // 2 * spacing[m] for m in range(l + 1, nl)) + 2 for l in range(nl)]
    mask = np.zeros(vals.shape, bool)
    for z, y, x in np.argwhere(~(np.abs(vals - 0.5) > ambiguous)):
        level = next(l for l in range(nl) if z % spacing[l] == 0 and y % spacing[l] == 0 and x % spacing[l] == 0)
        r = reach[level]
        mask[max(z - r, 0):z + r + 1, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return mask


def test_octree_multi_view_vs_dense_reference(ops):
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    g = load_golden("views_dense65")
    case, layers, f, _, calibs = case_inputs(g)
    v_n = case["V"]
    net = _net("G", layers, v_n)
    feats = [[torch.zeros(v_n, 256, 2, 2, device=DEV)]] * 3 + [[torch.from_numpy(f).to(DEV)]]
    calib = torch.from_numpy(calibs).to(DEV)

    def query_func(points, im_feat_list, calib_tensor):  # RTL/main.py:169-183, one row: get_preds()[0][0]
        samples = points.repeat(v_n, 1, 1).permute(0, 2, 1)
        return net.query(im_feat_list, points=samples, calibs=calib_tensor)[0][:1]

    eng = Seg3dLossless(query_func=query_func, b_min=np.array([[-1.0, -1, -1]]), b_max=np.array([[1.0, 1, 1]]),
                        resolutions=RES, balance_value=0.5, faster=True).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        vol = eng(im_feat_list=feats, calib_tensor=calib)
    assert eng.last_path == "generic"
    vol = vol[0, 0].cpu().numpy()
    ref = g["out"]
    firm = ~undecided_reach(ref)
    assert firm.mean() > 0.5
    flips = int(((vol > 0.5) != (ref > 0.5))[firm].sum())
    print("views_dense65: %d of %d firm nodes, %d thresholded nodes differ, inside %.4f"
          % (int(firm.sum()), firm.size, flips, float((ref > 0.5).mean())))
    assert flips == 0


def test_error_paths(ops):
    from monoport_amd._lib import MonoportError
    from monoport_amd.modeling import heads
    layers = syn.rand_mlp("G", 601, 2.0)
    net = _net("G", layers, 3)
    feats = [[torch.zeros(6, 256, 16, 16, device=DEV)]]
    p = torch.zeros((6, 3, 10), device=DEV)
    with pytest.raises(RuntimeError):  # B = 2 point sets of 3 views: the reference's broadcast raises
        net.query(feats, p, torch.eye(4, device=DEV)[None].expand(6, 4, 4))
    with pytest.raises(RuntimeError):  # 4 rows are not groups of 3 views
        net.query([[torch.zeros(4, 256, 16, 16, device=DEV)]], p[:4], torch.eye(4, device=DEV)[None].expand(4, 4, 4))
    with pytest.raises(RuntimeError):
        net.surface_classifier(torch.zeros((4, 257, 10), device=DEV))
    with pytest.raises(ValueError):
        heads.SurfaceClassifier(CHANNELS["G"], 9, False, "sigmoid")
    with pytest.raises(ValueError):
        net.surface_classifier.set_precision("f16")
    # the C-ABI refuses what the Python side never sends
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP["G"])
    fh = [ops.pack_features(torch.zeros((1, 256, 16, 16), device=DEV)) for _ in range(2)]
    pts, cal = torch.zeros((2, 3, 10), device=DEV), torch.eye(4, device=DEV)[None].expand(2, 4, 4)
    mlp.set_precision("f16w")
    with pytest.raises(MonoportError, match="f32"):
        ops.query_views(mlp, fh, pts, cal, "orthogonal", syn.Z_SCALE)
    with pytest.raises(MonoportError, match="f32"):
        ops.mlp_forward_views(mlp, torch.zeros((2, 257, 10), device=DEV))
    for one in (lambda: ops.query_views(mlp, fh[:1], pts[:1], cal[:1], "orthogonal", syn.Z_SCALE),
                lambda: ops.mlp_forward_views(mlp, torch.zeros((1, 257, 10), device=DEV))):
        with pytest.raises(MonoportError, match="f32"):  # both entry points refuse non-f32 heads at every V
            one()
    mlp.set_precision("f32")
    import ctypes
    ptrs = ctypes.c_void_p * 9
    out = torch.empty((9, 1, 10), device=DEV)
    rc = mlp.ctx.lib.mp_query_views(mlp.ctx.handle, mlp.id, 9, ptrs(*[fh[0].data_ptr()] * 9), 256, 16, 16,
                                    ptrs(*[pts[0].data_ptr()] * 9), 10, 1, 10, ptrs(*[cal[0].data_ptr()] * 9), 0,
                                    ctypes.c_float(1.0), ptrs(*[out[0].data_ptr()] * 9), None)
    assert rc == -3  # MP_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.query_views(mlp, fh * 5, pts.repeat(5, 1, 1)[:10], cal.repeat(5, 1, 1)[:10], "orthogonal", syn.Z_SCALE)


def test_colorization_refuses_multi_view_head(ops):
    """recon.colorization binds netC for the single-view counted query: a multi-view netC is refused, not run as a
    single-view head."""
    from monoport_amd.recon import colorization
    net_c = _net("C", syn.rand_mlp("C", 701, 2.0), 2)
    feats = [[torch.zeros(2, 512, 16, 16, device=DEV)]]
    x = torch.zeros(5, dtype=torch.int64, device=DEV)
    z = torch.zeros(5, dtype=torch.float32, device=DEV)
    with pytest.raises(NotImplementedError, match="num_views"):
        colorization(net_c, feats, x, x, z, torch.eye(4, device=DEV)[None].expand(2, 4, 4), None, resolution=33)
