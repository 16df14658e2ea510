"""MonoPortNet.query over B > 1 frames and under the perspective projection (mp_query_batch, the per-frame
MP_PROJ_* mode of the fused kernels), against fixtures the reference produced
(tools/gen_golden_query_ext.py).  Needs an MI355X."""
import ast
import contextlib

import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
TOL_REF = 1e-4  # the repository's bar against the reference
TOL_F16 = {"f16w": 3e-4, "f16": 5e-3}  # the bounds of the orthogonal f16w / f16 tests (test_query_gpu.py)
DEPTH = 3.0  # the perspective fixtures' camera distance (tools/gen_golden_query_ext.py)


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops
    return ops


def persp_body_mlp(kind, seed, noise, k=40.0):
    """body_mlp with its surface moved to the camera distance (layer 0 biases -k D, +k D)."""
    layers = syn.body_mlp(kind, k=k, noise=noise, seed=seed)
    layers[0][1][0] -= np.float32(k * DEPTH)
    layers[0][1][1] += np.float32(k * DEPTH)
    return layers


def case_inputs(g):
    """Regenerate a fixture's inputs from its ``case`` record: (kind, layers, [C,H,W] map, [3,N] points)."""
    case = ast.literal_eval(str(g["case"][0]))
    kind, mlp, feat, pts = case["kind"], case["mlp"], case["feat"], case["pts"]
    if mlp[0] == "rand":
        layers = syn.rand_mlp(kind, mlp[1], mlp[2])
    elif mlp[0] == "body":
        layers = syn.body_mlp(kind, noise=mlp[2], seed=mlp[1])
    else:
        layers = persp_body_mlp(kind, mlp[1], mlp[2])
    f = syn.rand_feat(feat[1], 128, 128, feat[2]) if feat[0] == "rand" else syn.body_feat(feat[1], 128, 128, feat[2])
    p = None
    if pts[0] == "rand":
        p = syn.rand_points(pts[1], pts[2], pts[3])
        p[:, :4] = g["special"]  # the points on z_cam == 0
    return kind, layers, f, p


@contextlib.contextmanager
def small_gate(mode):
    """mp_query_tune: 0 = 64-point kernel (query.hip), 1 = 32-point kernel (query_small.hip)."""
    from monoport_amd import _lib
    lib = _lib.load()
    lib.mp_query_tune(mode)
    try:
        yield
    finally:
        lib.mp_query_tune(-1)


def run_path(ops, mlp, fh, pts, cal, path, projection="perspective"):
    """One query through a pinned kernel: plain64 / plain32 (exact f32), table (exact f32 skip table),
    f16x3 / f16x3_table, f16w, f16."""
    prec = {"plain64": "f32", "plain32": "f32", "table": "f32"}.get(path, path.replace("_table", ""))
    mlp.set_precision(prec)
    handle = ops.skip_table(mlp, fh) if path.endswith("table") else None
    try:
        with small_gate(0 if path == "plain64" else 1):
            return ops.query(mlp, fh, pts, cal, syn.Z_SCALE, projection)[0].cpu().numpy()
    finally:
        if handle is not None:
            handle.release()
        mlp.set_precision("f32")


def _setup(ops, name):
    g = load_golden(name)
    kind, layers, f, p = case_inputs(g)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP[kind])
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    return g, kind, mlp, fh, torch.from_numpy(p)[None].to(DEV), torch.from_numpy(g["calib"]).to(DEV)


def _check_zeros_and_nans(ops, out, g, pts, cal):
    ref = g["out"]
    xyz = ops.perspective(pts, cal)[0].cpu().numpy()
    finite = np.isfinite(xyz[:2]).all(0)
    inside = finite & (np.abs(xyz[0]) <= 1) & (np.abs(xyz[1]) <= 1)
    assert np.array_equal(np.isnan(out), np.isnan(ref))  # NaN exactly where the reference has NaN ...
    assert np.isnan(out[:, ~finite]).all()               # ... which is every point on z_cam == 0
    assert (~finite).sum() == 4
    assert (out[:, finite & ~inside] == 0).all()          # every other out-of-image point is exactly 0
    return inside


def test_perspective_op_vs_reference(ops):
    """geometry.perspective on HIP is bit-identical to the reference's, NaN and +-inf positions included."""
    from monoport_amd.modeling import geometry
    g = load_golden("perspective")
    p = torch.from_numpy(g["points"])[None].to(DEV)
    cal = torch.from_numpy(g["calib"]).to(DEV)
    out = geometry.perspective(p, cal)[0].cpu().numpy()
    np.testing.assert_array_equal(out, g["out"])
    assert np.array_equal(np.isinf(out), np.isinf(g["out"])) and np.array_equal(np.signbit(out), np.signbit(g["out"]))
    assert (g["out"][2] < 0).sum() >= 50 and (g["out"][2] == 0).sum() >= 8
    two = geometry.perspective(p.repeat(2, 1, 1), cal.repeat(2, 1, 1)).cpu().numpy()
    np.testing.assert_array_equal(two[1], g["out"])


@pytest.mark.parametrize("path", ["plain64", "plain32", "table", "f16x3", "f16x3_table"])
@pytest.mark.parametrize("name", ["query_G_persp", "query_G_persp_body"])
def test_netg_perspective_vs_reference(ops, name, path):
    g, kind, mlp, fh, pts, cal = _setup(ops, name)
    out = run_path(ops, mlp, fh, pts, cal, path)
    assert out.shape == g["out"].shape
    _check_zeros_and_nans(ops, out, g, pts, cal)
    ok = ~np.isnan(g["out"])
    err = float(np.abs(out - g["out"])[ok].max())
    print("%s %s: max |gpu - reference| %.3g" % (name, path, err))
    assert err <= TOL_REF


@pytest.mark.parametrize("path", ["plain64"])
def test_netc_perspective_vs_reference(ops, path):
    g, kind, mlp, fh, pts, cal = _setup(ops, "query_C_persp")
    out = run_path(ops, mlp, fh, pts, cal, path)
    _check_zeros_and_nans(ops, out, g, pts, cal)
    ok = ~np.isnan(g["out"])
    err = float(np.abs(out - g["out"])[ok].max())
    print("query_C_persp: max |gpu - reference| %.3g" % err)
    assert err <= TOL_REF


@pytest.mark.parametrize("name,precision", [("query_G_persp", "f16w"), ("query_G_persp_body", "f16w"),
                                            ("query_G_persp", "f16")])
def test_f16_modes_perspective(ops, name, precision):
    """f16w / f16 at the bounds of their orthogonal tests.  Plain f16 (f16 activations) is held to its bound on
    the random head only: the perspective body head moves its surface to the camera distance through layer-0
    biases of +-k D = +-120, where an f16 activation carries ~0.06 of rounding (measured 1.5e-2 at the output)."""
    g, kind, mlp, fh, pts, cal = _setup(ops, name)
    out = run_path(ops, mlp, fh, pts, cal, precision)
    _check_zeros_and_nans(ops, out, g, pts, cal)
    ok = ~np.isnan(g["out"])
    assert float(np.abs(out - g["out"])[ok].max()) <= TOL_F16[precision]


def _net(kind, layers, projection):
    from monoport_amd.modeling import PIFuNetC, PIFuNetG, geometry
    net = PIFuNetG() if kind == "G" else PIFuNetC()
    sd = {}
    for i, (w, b) in enumerate(layers):
        sd["filters.%d.weight" % i] = torch.from_numpy(w)[:, :, None]
        sd["filters.%d.bias" % i] = torch.from_numpy(b)
    net.surface_classifier.load_state_dict(sd)
    net.surface_classifier.to(DEV)
    net.opt.projection = projection
    net.projection = getattr(geometry, projection)
    return net.eval()


def test_monoportnet_query_b3_vs_reference(ops, monkeypatch):
    monkeypatch.setattr(ops, "SKIP_TABLE", False)  # the plain kernels for both calls below (no table mid-way)
    g = load_golden("query_G_b3")
    case = ast.literal_eval(str(g["case"][0]))
    net = _net("G", syn.rand_mlp("G", *case["mlp"][1:]), "orthogonal")
    f = torch.from_numpy(np.stack([syn.rand_feat(256, 128, 128, s) for s in case["feats"]])).to(DEV)
    p = torch.from_numpy(np.stack([syn.rand_points(*t) for t in case["pts"]])).to(DEV)
    feats = [[torch.zeros(3, 256, 2, 2, device=DEV)]] * 3 + [[f]]
    out = net.query(feats, p, calibs=torch.from_numpy(g["calib"]).to(DEV))[0]
    assert out.shape == (3, 1, p.shape[2])
    out = out.cpu().numpy()
    assert float(np.abs(out - g["out"]).max()) <= TOL_REF
    # a strided [B,N,3] view (RTL/main.py:176-177 builds one) gives the same bits
    p_nc = p.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert p_nc.stride(1) == 1
    again = net.query(feats, p_nc, calibs=torch.from_numpy(g["calib"]).to(DEV))[0].cpu().numpy()
    assert np.array_equal(again, out)
    # every map with its skip table: one table-kernel launch for the three frames
    monkeypatch.setattr(ops, "SKIP_TABLE", True)
    monkeypatch.setattr(ops, "SKIP_TABLE_MIN_POINTS", 0)
    tab = net.query(feats, p_nc, calibs=torch.from_numpy(g["calib"]).to(DEV))[0].cpu().numpy()
    assert all(net.has_skip_table(net._packed_features([f], b)) for b in range(3))
    assert float(np.abs(tab - g["out"]).max()) <= TOL_REF


@pytest.mark.parametrize("projection", ["orthogonal", "perspective"])
@pytest.mark.parametrize("b", [3, 40])
def test_batch_equals_single_frames(ops, monkeypatch, b, projection):
    """B frames in mp_query_batch launches (two for B = 40) equal B one-frame calls bit for bit on the plain
    kernel (no skip tables: MONOPORT_SKIP_TABLE=off)."""
    monkeypatch.setattr(ops, "SKIP_TABLE", False)
    net = _net("G", syn.rand_mlp("G", 7, 2.0), projection)
    n = 3000
    f = torch.from_numpy(np.stack([syn.rand_feat(256, 32, 32, 300 + i) for i in range(b)])).to(DEV)
    p = torch.from_numpy(np.stack([syn.rand_points(n, 400 + i, 1.2) for i in range(b)])).to(DEV)
    if projection == "perspective":
        calib = torch.from_numpy(np.stack([_persp_calib(2.0 + 0.01 * i) for i in range(b)])).to(DEV)
    else:
        calib = torch.from_numpy(np.stack([syn_calib(i) for i in range(b)])).to(DEV)
    feats = [[f]]
    with small_gate(1):
        out = net.query(feats, p, calibs=calib)[0].cpu().numpy()
        assert out.shape == (b, 1, n)
        for i in range(b):
            one = net.query([[f[i:i + 1]]], p[i:i + 1], calibs=calib[i:i + 1])[0].cpu().numpy()
            assert np.array_equal(one[0], out[i], equal_nan=True), i
        # [B,N,3] view of the same points
        view = p.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert view.stride(1) == 1
        assert np.array_equal(net.query(feats, view, calibs=calib)[0].cpu().numpy(), out, equal_nan=True)
    assert (out != 0).any()


def _persp_calib(focal):
    r = np.array([[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]])
    m = np.eye(4)
    m[:3, :3] = np.diag([focal, focal, 1.0]) @ r
    m[:3, 3] = [0.0, 0.0, DEPTH]
    return m.astype(np.float32)


def syn_calib(i):
    from oracle import pifu_oracle as orc
    return orc.pifu_calib(*syn.scene_camera(7 * i))[0]


def test_mixed_projection_batch_through_ops(ops):
    """One mp_query_batch launch with an orthogonal and a perspective frame equals the two one-frame calls."""
    mlp = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("G", 8, 2.0), syn.LAST_OP["G"])
    fh = [ops.pack_features(torch.from_numpy(syn.rand_feat(256, 64, 64, 500 + i))[None].to(DEV)) for i in range(2)]
    p = torch.from_numpy(np.stack([syn.rand_points(5000, 510 + i, 1.2) for i in range(2)])).to(DEV)
    cals = [torch.from_numpy(syn_calib(3)).to(DEV), torch.from_numpy(_persp_calib(2.0)).to(DEV)]
    with small_gate(1):
        both = ops.query_batch(mlp, fh, p, cals, ["orthogonal", "perspective"], syn.Z_SCALE).cpu().numpy()
        ortho = ops.query(mlp, fh[0], p[0:1], cals[0], syn.Z_SCALE).cpu().numpy()
        persp = ops.query(mlp, fh[1], p[1:2], cals[1], syn.Z_SCALE, "perspective").cpu().numpy()
    assert np.array_equal(both[0], ortho[0]) and np.array_equal(both[1], persp[0])
    assert not np.array_equal(both[1], ops.query(mlp, fh[1], p[1:2], cals[1], syn.Z_SCALE).cpu().numpy()[0])
    from monoport_amd._lib import MonoportError
    with pytest.raises(MonoportError):  # an unknown mode is refused by the C-ABI
        ctx = mlp.ctx
        import ctypes
        ptrs = ctypes.c_void_p * 1
        out = torch.empty((1, 1, 5000), device=DEV)
        ctx.check(ctx.lib.mp_query_batch(ctx.handle, mlp.id, 1, ptrs(fh[0].data_ptr()), 256, 64, 64,
                                         ptrs(p[0].data_ptr()), 5000, 1, 5000, ptrs(cals[0].data_ptr()),
                                         (ctypes.c_int * 1)(7), ctypes.c_float(syn.Z_SCALE), ptrs(out.data_ptr()),
                                         None), "mp_query_batch")


@pytest.mark.parametrize("path", ["plain64", "plain32", "table"])
def test_orthogonal_batch_unchanged(ops, path):
    """mp_query_batch with MP_PROJ_ORTHOGONAL is bit-identical to mp_query on query_G_rand."""
    kind, layers = "G", syn.rand_mlp("G", 11, 2.0)  # query_G_rand's inputs (oracle/gen_golden.py: gen_query)
    f, p = syn.rand_feat(256, 128, 128, 21), syn.rand_points(49152, 31, 0.8)
    g = load_golden("query_G_rand")
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP[kind])
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    pts = torch.from_numpy(p)[None].to(DEV)
    cal = torch.from_numpy(g["calib"]).to(DEV)
    handle = ops.skip_table(mlp, fh) if path == "table" else None
    with small_gate(0 if path == "plain64" else 1):
        a = ops.query(mlp, fh, pts, cal, syn.Z_SCALE).cpu().numpy()
        b = ops.query_batch(mlp, [fh], pts, [cal], ["orthogonal"], syn.Z_SCALE).cpu().numpy()
    if handle is not None:
        handle.release()
    assert np.array_equal(a, b)
    assert np.abs(a[0] - g["out"]).max() <= TOL_REF


# ---- octree engine ------------------------------------------------------------------------------------------
RES = [17, 33, 65]


def undecided_reach(vals, ambiguous=1e-4):
    """Nodes of the final lattice where two fp32-class evaluations may take different octree decisions: the
    reach of every node within ``ambiguous`` of 0.5 (or NaN), counted from the coarsest level it belongs to --
    spacing s_l plus the dilation boxes 9 / 7 of the finer levels, plus 2 for the interpolation footprint."""
    nl, rf = len(RES), RES[-1]
    spacing = [(rf - 1) // (r - 1) for r in RES]
    box = [0, 9, 7]
    reach = [spacing[l] + sum((box[m] - 1) // 2 * spacing[m] for m in range(l + 1, nl)) + 2 for l in range(nl)]
    mask = np.zeros(vals.shape, bool)
    for z, y, x in np.argwhere(~(np.abs(vals - 0.5) > ambiguous)):
        level = next(l for l in range(nl) if z % spacing[l] == 0 and y % spacing[l] == 0 and x % spacing[l] == 0)
        r = reach[level]
        mask[max(z - r, 0):z + r + 1, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return mask


def _engine_setup(validate="always"):
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    g = load_golden("persp_dense65")
    kind, layers, f, _ = case_inputs(g)
    net = _net("G", layers, "perspective")
    feats = [[torch.zeros(1, 256, 2, 2, device=DEV)]] * 3 + [[torch.from_numpy(f)[None].to(DEV)]]
    calib = torch.from_numpy(g["calib"]).to(DEV)

    def query_func(points, im_feat_list, calib_tensor):  # RTL/main.py:169-183
        samples = points.repeat(1, 1, 1).permute(0, 2, 1)
        return net.query(im_feat_list, points=samples, calibs=calib_tensor)[0]

    def make(faster=True):
        return Seg3dLossless(query_func=query_func, b_min=np.array([[-1.0, -1, -1]]), b_max=np.array([[1.0, 1, 1]]),
                             resolutions=RES, balance_value=0.5, faster=faster, validate=validate).to(DEV)
    return g, net, feats, calib, query_func, make


def test_octree_fused_perspective_vs_dense_reference(ops):
    g, net, feats, calib, query_func, make = _engine_setup()
    eng = make()
    vol = eng(im_feat_list=feats, calib_tensor=calib)
    assert eng.last_path == "fused"
    vol = vol[0, 0].cpu().numpy()
    ref = g["out"]
    firm = ~undecided_reach(ref)
    assert firm.mean() > 0.5
    flips = int(((vol > 0.5) != (ref > 0.5))[firm].sum())
    print("persp_dense65: %d of %d firm nodes, %d thresholded nodes differ, inside %.4f"
          % (int(firm.sum()), firm.size, flips, float((ref > 0.5).mean())))
    assert flips == 0


def test_octree_generic_perspective_equals_fused(ops):
    g, net, feats, calib, query_func, make = _engine_setup()
    fused = make()(im_feat_list=feats, calib_tensor=calib)[0, 0].cpu().numpy()
    gen = make(faster=False)
    vol = gen(im_feat_list=feats, calib_tensor=calib)
    assert gen.last_path == "generic"
    firm = ~undecided_reach(g["out"])
    vol = vol[0, 0].cpu().numpy()
    assert int(((vol > 0.5) != (g["out"] > 0.5))[firm].sum()) == 0
    assert int(((vol > 0.5) != (fused > 0.5))[firm].sum()) == 0


def test_trusted_path_never_crosses_projection(ops):
    """validate="first": after VALIDATE_CALLS agreeing calls the engine trusts the binding key and skips the
    validation query.  Alternating an orthogonal and a perspective query_func on the same head must never take
    the trusted path across the switch, and every volume equals the one a fresh engine computes."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import geometry
    g, net, feats, calib, query_func, make = _engine_setup()
    ortho = syn_calib(5)
    ortho[2, 3] += DEPTH  # the head's surface sits at depth DEPTH: an orthogonal camera that reaches it
    calibs = {False: torch.from_numpy(ortho[None]).to(DEV), True: calib}
    fresh = {}
    for persp in (False, True):
        net.projection = geometry.perspective if persp else geometry.orthogonal
        fresh[persp] = make()(im_feat_list=feats, calib_tensor=calibs[persp])[0, 0].cpu().numpy()
    assert not np.array_equal(fresh[False], fresh[True]) and (fresh[False] > 0.5).any()
    eng = make()
    eng.validate = "first"
    trusted = []
    inner = eng._forward_trusted

    def spy(kwargs):
        out = inner(kwargs)
        trusted.append(out is not NotImplemented)
        return out
    eng._forward_trusted = spy
    n0 = Seg3dLossless.VALIDATE_CALLS + 1
    seq = [False] * n0 + [True, False, True, True, False]
    for i, persp in enumerate(seq):
        net.projection = geometry.perspective if persp else geometry.orthogonal
        trusted.clear()
        vol = eng(im_feat_list=feats, calib_tensor=calibs[persp])[0, 0].cpu().numpy()
        assert eng.last_path == "fused"
        assert eng._trusted_key[-1] == ops.PROJECTIONS["perspective" if persp else "orthogonal"]
        if i > 0 and seq[i - 1] != persp:
            assert not any(trusted), "trusted path taken across the projection switch at call %d" % i
        assert np.array_equal(vol, fresh[persp]), i


# ---- colour ---------------------------------------------------------------------------------------------------
def test_colorization_perspective_netc(ops):
    from monoport_amd.recon import color_matrix, colorization, forward_vertices
    res = 33
    net = _net("C", syn.rand_mlp("C", 61, 2.0), "perspective")
    feat_C = [[torch.from_numpy(syn.rand_feat(512, 128, 128, 62))[None].to(DEV)]]
    vol = torch.from_numpy(syn.blob_volume(res, 63)).to(DEV)[None, None]
    X, Y, Z, norm = forward_vertices(vol, "front")
    calib = torch.from_numpy(_persp_calib(2.0)[None]).to(DEV)
    mat = color_matrix([-1, -1, -1], [1, 1, 1], res)
    tex = colorization(net, feat_C, X, Y, Z, calib, None, resolution=res, mat_color=mat).cpu().numpy()
    count = torch.tensor([X.shape[0]], dtype=torch.int32, device=DEV)
    pts = ops.vertex_points(X, Y, Z.float(), count, res, mat)
    pred = net.query(feat_C, pts[None], calibs=calib)[0][0]
    ref = ops.paint(X, Y, pred.contiguous(), 1, count, res, 0.5, 0.5, -np.inf, np.inf).cpu().numpy()
    assert np.array_equal(tex, ref)
    orth = colorization(_net("C", syn.rand_mlp("C", 61, 2.0), "orthogonal"), feat_C, X, Y, Z, calib, None,
                        resolution=res, mat_color=mat).cpu().numpy()
    assert not np.array_equal(tex, orth)
