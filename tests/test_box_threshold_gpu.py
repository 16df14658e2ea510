"""The octree, lattice, marching-cubes and colour kernels on an off-centre box B and thresholds other than 0.5.

Every other GPU test runs them on [-1, 1]^3 with balance = level = 0.5, where an axis mix-up, a reordered rounding
or a literal 0.5 for the parameter gives the same bits.  Box B (tests/test_box_threshold_cpu.py, which also shows
that B, the thresholds and the ellipsoid field discriminate) has three different corners and three different
lengths.  Each reference below is the CPU restatement in oracle/ fed the same values the GPU path sees.  Needs an
MI355X."""
import numpy as np
import pytest

from monoport_amd import synthetic as syn
from test_box_threshold_cpu import (B_MAX, B_MIN, SWAP_XZ, all_idx, ellipsoid_np, mc_f64_tolerance,
                                    mc_verts_f64, oracle_lattice)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
RES = [17, 33, 65, 129]
PERSP_DEPTH = 3.0


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


def _query_fn(ops, mlp, fh, cal, projection="orthogonal"):
    def gpu_query(pts):  # [3,N] numpy -> [N] numpy through the HIP query kernel
        p = torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV)
        return ops.query(mlp, fh, p, cal, syn.Z_SCALE, projection)[0, 0].cpu().numpy()
    return gpu_query


@pytest.fixture(scope="module")
def body(ops, oracle):
    layers = syn.body_mlp("G", noise=0.05, seed=1)
    f = syn.body_feat(256, 128, 128, 2)
    calib = oracle.pifu_calib(*syn.scene_camera(30))
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    cal = torch.from_numpy(calib).to(DEV)
    return dict(layers=layers, f=f, calib=calib, mlp=mlp, fh=fh, cal=cal, gpu_query=_query_fn(ops, mlp, fh, cal))


def _outside_level0(oracle, calib, res):
    """Level-0 nodes of B (z,y,x) whose orthogonal projection falls outside the image."""
    r0 = res[0]
    p = oracle.lattice_points(all_idx(r0), (res[-1] - 1) // (r0 - 1), res[-1], B_MIN, B_MAX)
    xyz = oracle.orthogonal(p, calib[0])
    return ((np.abs(xyz[0]) > 1) | (np.abs(xyz[1]) > 1)).reshape(r0, r0, r0)


def _check_recon(ops, oracle, mlp, fh, cal, gpu_query, balance, res=RES, final_level="dilate3",
                 projection="orthogonal"):
    """ops.recon on B == oracle.seg3d_lossless driven by ``gpu_query`` (explicit points from oracle.lattice_points,
    while the fused kernels decode packed lattice codes): status and volume bit for bit."""
    vol, status = ops.recon(mlp, fh, cal, syn.Z_SCALE, B_MIN, B_MAX, res, balance, final_level=final_level,
                            projection=projection)
    st = status.cpu().numpy()
    stats = []
    ref = oracle.seg3d_lossless(gpu_query, B_MIN, B_MAX, res, balance_value=balance, stats=stats,
                                final_level=final_level)
    assert ref is not None and st[0] == 1
    assert list(st[1:]) == stats
    v = vol.cpu().numpy()
    assert np.array_equal(v, ref)
    return v, st


@pytest.mark.parametrize("balance", [0.3, 0.5, 0.7])
def test_fused_octree_on_box_b_bit_exact(ops, oracle, body, balance, monkeypatch):
    monkeypatch.setattr(ops, "SKIP_TABLE", False)
    v, st = _check_recon(ops, oracle, body["mlp"], body["fh"], body["cal"], body["gpu_query"], balance)
    out = _outside_level0(oracle, body["calib"], RES)
    assert out.mean() >= 0.01
    s = (RES[-1] - 1) // (RES[0] - 1)
    lv0 = v[::s, ::s, ::s]
    assert (lv0[out] == 0).all() and (lv0[~out] != 0).any()
    assert (v > np.float32(balance)).sum() > 1000


def test_fused_octree_balances_differ(ops, body):
    """The three balances take different decisions on B (a literal 0.5 in a kernel would make them agree)."""
    got = {}
    for b in (0.3, 0.5, 0.7):
        vol, st = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, B_MIN, B_MAX, RES, b)
        got[b] = (st.cpu().numpy(), vol)
    assert len({tuple(s[1:]) for s, _ in got.values()}) == 3
    assert not torch.equal(got[0.3][1], got[0.5][1]) and not torch.equal(got[0.5][1], got[0.7][1])


@pytest.mark.parametrize("rule", ["upstream", "interpolate"])
def test_final_level_rules_on_box_b(ops, oracle, body, rule):
    _check_recon(ops, oracle, body["mlp"], body["fh"], body["cal"], body["gpu_query"], 0.3, final_level=rule)


@pytest.mark.parametrize("path", ["table", "plain", "tile0", "tile1", "f16x3", "f16w", "f16"])
def test_every_lattice_decoding_query_kernel_on_box_b(ops, oracle, body, path, monkeypatch):
    """Each query kernel that decodes packed lattice codes (its own copy of the lattice arithmetic: the skip-table
    kernel, the plain and small-tile kernels, the f16 kernels) against the oracle fed by the same kernel."""
    from monoport_amd import _lib
    lib = _lib.load()
    monkeypatch.setattr(ops, "SKIP_TABLE", False)
    mlp = ops.PackedMLP.from_layers(DEV, body["layers"], 1)
    fh = ops.pack_features(torch.from_numpy(body["f"])[None].to(DEV))
    if path.startswith("f16"):
        mlp.set_precision(path)
    q = _query_fn(ops, mlp, fh, body["cal"])
    table = None
    try:
        if path == "table":
            plain = q(syn.rand_points(20000, 3, 1.0))
            table = ops.skip_table(mlp, fh)
            assert not np.array_equal(q(syn.rand_points(20000, 3, 1.0)), plain), "the skip-table kernel did not run"
        elif path.startswith("tile"):
            lib.mp_query_tune(int(path[-1]))
        _check_recon(ops, oracle, mlp, fh, body["cal"], q, 0.7)
    finally:
        if table is not None:
            table.release()
        lib.mp_query_tune(-1)


def test_recon_batch_on_box_b_equals_single_frames(ops, oracle, body):
    feats, cals = [], []
    for i in range(3):
        feats.append(ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2 + i))[None].to(DEV)))
        cals.append(torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(30 + 25 * i))).to(DEV))
    vols, status = ops.recon_batch(body["mlp"], feats, cals, syn.Z_SCALE, B_MIN, B_MAX, RES, 0.3)
    st = status.cpu().numpy()
    assert (st[:, 0] == 1).all() and len({tuple(r) for r in st[:, 1:].tolist()}) == 3
    for i in range(3):
        v1, s1 = ops.recon(body["mlp"], feats[i], cals[i], syn.Z_SCALE, B_MIN, B_MAX, RES, 0.3)
        assert np.array_equal(s1.cpu().numpy(), st[i]), i
        assert torch.equal(v1, vols[i]), i


def test_perspective_recon_on_box_b(ops, oracle):
    k = 40.0
    layers = syn.body_mlp("G", k=k, noise=0.05, seed=171)  # the surface moved to the camera distance
    layers[0][1][0] -= np.float32(k * PERSP_DEPTH)
    layers[0][1][1] += np.float32(k * PERSP_DEPTH)
    r = np.array([[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]])
    calib = np.eye(4)
    calib[:3, :3] = np.diag([2.0, 2.0, 1.0]) @ r
    calib[:3, 3] = [0.0, 0.0, PERSP_DEPTH]
    cal = torch.from_numpy(calib.astype(np.float32)[None]).to(DEV)
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    fh = ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 172))[None].to(DEV))
    v, st = _check_recon(ops, oracle, mlp, fh, cal, _query_fn(ops, mlp, fh, cal, "perspective"), 0.3,
                         projection="perspective")
    assert (v > np.float32(0.3)).sum() > 1000


def test_recon_on_box_b_matches_float64_oracle(ops, oracle, body):
    """Against the all-CPU oracle with the float64 query: the field is as close to it as the CPU's own f32 query
    is (measured 1.67e-4 for both: the body head's slope of 40 amplifies f32 rounding, on [-1, 1]^3 too), within
    1e-4 of the all-CPU f32 oracle, and the thresholded volume is identical away from the threshold."""
    res = [9, 17, 33, 65]
    vol, status = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, B_MIN, B_MAX, res, 0.3)
    refs = {}
    for prec in ("f64", "f32"):
        q = lambda p: oracle.query(body["f"], p, body["calib"][0], body["layers"], 1, syn.Z_SCALE,
                                   precision=prec)[0]
        refs[prec] = oracle.seg3d_lossless(q, B_MIN, B_MAX, res, balance_value=0.3)
    ref = refs["f64"]
    v = vol.cpu().numpy()
    assert int(status[0]) == 1
    err, err_cpu32 = np.abs(v - ref).max(), np.abs(refs["f32"] - ref).max()
    print("recon on B vs float64 oracle: %.3g (CPU f32 oracle: %.3g)" % (err, err_cpu32))
    assert err <= max(2 * err_cpu32, 1e-5)
    assert np.abs(v - refs["f32"]).max() <= 1e-4
    safe = np.abs(ref - 0.3) > 1e-3
    assert np.array_equal((v > 0.3)[safe], (ref > 0.3)[safe])
    assert (ref > 0.3).sum() > 1000


def _lexsorted(p):  # [N,3] rows in a canonical order
    return p[np.lexsort(p.T[::-1])]


@pytest.mark.parametrize("faster", [True, False])
@pytest.mark.parametrize("balance", [0.3, 0.7])
def test_generic_engine_on_box_b(ops, oracle, faster, balance):
    """Seg3dLossless with a plain query_func (LevelEngine: lattice_points_kernel, scatter, conflicts): the
    off-centre ellipsoid evaluated on the host in float32, so GPU and oracle see identical values for identical
    points.  Volume and counts equal the oracle; every point the engine hands over is oracle.lattice_points of
    its node bit for bit, and each call hands over the oracle's set of nodes."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    seen, seen_ref = [], []

    def query_func(points):  # [1,N,3] on the device
        p = points[0].cpu().numpy()
        seen.append(p.copy())
        return torch.from_numpy(ellipsoid_np(p.T)).to(points.device)[None, None]

    def ref_query(p):  # [3,N]
        seen_ref.append(p.T.copy())
        return ellipsoid_np(p)

    res = [9, 17, 33, 65]
    eng = Seg3dLossless(query_func=query_func, b_min=B_MIN[None], b_max=B_MAX[None], resolutions=res,
                        balance_value=balance, faster=faster).to(DEV)
    sdf = eng()
    assert eng.last_path == "generic"
    stats = []
    ref = oracle.seg3d_lossless(ref_query, B_MIN, B_MAX, res, balance_value=balance, stats=stats, faster=faster)
    assert ref is not None and sdf is not None
    assert list(eng.last_status[1:].numpy()) == stats
    assert np.array_equal(sdf[0, 0].cpu().numpy(), ref)
    rf = res[-1]
    bmin, blen = B_MIN.astype(np.float64), (B_MAX - B_MIN).astype(np.float64)
    assert len(seen) == len(seen_ref)
    for got, want in zip(seen, seen_ref):
        c = np.rint(((got.astype(np.float64) - bmin) / blen - 0.5 / rf) * rf).astype(np.int64)  # [N,3] x,y,z
        assert (c >= 0).all() and (c < rf).all()
        assert np.array_equal(oracle.lattice_points(c[:, ::-1], 1, rf, B_MIN, B_MAX).T, got)
        assert np.array_equal(_lexsorted(got), _lexsorted(want))


def test_seg3d_lossless_fused_on_box_b_equals_recon(ops, body, monkeypatch):
    """Through a MonoPortNet closure (the fused path) Seg3dLossless(b_min = B, balance_value = 0.3) is ops.recon
    with the same arguments."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    monkeypatch.setattr(ops, "SKIP_TABLE", False)  # the direct call below runs the plain kernel
    netG = PIFuNetG().eval()
    netG.surface_classifier.load_state_dict(
        {**{"filters.%d.weight" % i: torch.from_numpy(w)[:, :, None] for i, (w, _) in enumerate(body["layers"])},
         **{"filters.%d.bias" % i: torch.from_numpy(b) for i, (_, b) in enumerate(body["layers"])}})
    netG.surface_classifier.to(DEV)
    feats = [[torch.from_numpy(body["f"])[None].to(DEV)]]

    def query_func(points, feats, calib):
        return netG.query(feats, points.permute(0, 2, 1), calib)[0]

    eng = Seg3dLossless(query_func=query_func, b_min=[B_MIN], b_max=[B_MAX], resolutions=RES, balance_value=0.3,
                        faster=True).to(DEV)
    sdf = eng(feats=feats, calib=body["cal"])
    assert eng.last_path == "fused"
    vol, st = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, B_MIN, B_MAX, RES, 0.3)
    assert torch.equal(eng.last_status, st.cpu()) and int(st[0]) == 1
    assert torch.equal(sdf[0, 0], vol)


def _off_centre_sphere(r, centre=(0.21, -0.13, 0.34), radius=0.45, sharp=8.0):
    g = ((np.arange(r) + 0.5) / r) * 2 - 1
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return (1.0 / (1.0 + np.exp(-sharp * (radius - d) / radius))).astype(np.float32)


def _quantised(r=33):
    v = ellipsoid_np(oracle_lattice(r)).reshape(r, r, r)
    return (np.rint(v * np.float32(4)) / np.float32(4)).astype(np.float32)


@pytest.mark.parametrize("name,levels", [("blob33", (0.3, 0.7)), ("sphere65", (0.3, 0.7)),
                                         ("quant33", (0.5, 0.25)), ("recon129", (0.3, 0.7)),
                                         ("recon257", (0.3,))])
def test_marching_cubes_on_box_b(ops, oracle, body, name, levels):
    """Faces identical to oracle.marching_cubes(vol, level, B), vertices within 1e-6 of it and within a few ulp of
    |B| of the float64 crossing computed from the same f32 volume.  quant33 holds values in {0, .25, .5, .75, 1}:
    nodes lie exactly at the level, where inside is strictly above it."""
    from monoport_amd.recon import marching_cubes
    if name == "blob33":
        vol = syn.blob_volume(33, 5)
    elif name == "sphere65":
        vol = _off_centre_sphere(65)
    elif name == "quant33":
        vol = _quantised()
        assert set(np.unique(vol).tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}
    else:
        res = RES if name == "recon129" else RES + [257]
        v, st = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, B_MIN, B_MAX, res, levels[0])
        assert int(st[0]) == 1
        vol = v.cpu().numpy()
    for level in levels:
        if name == "quant33":
            assert (vol == np.float32(level)).sum() > 100
        verts, faces = marching_cubes(torch.from_numpy(vol).to(DEV)[None, None], level, B_MIN, B_MAX)
        rv, rf = oracle.marching_cubes(vol, level, B_MIN, B_MAX)
        assert len(rf) > 100
        assert tuple(verts.shape) == rv.shape and tuple(faces.shape) == rf.shape
        assert faces.dtype == torch.int32 and np.array_equal(faces.cpu().numpy(), rf)
        v = verts.cpu().numpy()
        assert np.abs(v - rv).max() <= 1e-6
        assert np.abs(v - mc_verts_f64(vol, level, B_MIN, B_MAX)).max() <= mc_f64_tolerance(B_MIN, B_MAX)
    if name == "sphere65":  # B with x and z swapped moves the vertices
        vs, _ = marching_cubes(torch.from_numpy(vol).to(DEV)[None, None], levels[0], B_MIN[SWAP_XZ], B_MAX[SWAP_XZ])
        v0, _ = marching_cubes(torch.from_numpy(vol).to(DEV)[None, None], levels[0], B_MIN, B_MAX)
        assert not torch.allclose(vs, v0, atol=1e-3)


def test_vertex_points_with_box_b_colour_matrix(ops, body):
    """vertex_points(color_matrix(B, r)) == ops.orthogonal of (X, Y, r - Z) with that matrix bit for bit, within 2 ulp
    (of the larger summand) of the float64 product, and x, y, z each scaled and moved by their own row."""
    from monoport_amd.recon import color_matrix
    r = RES[-1]
    vol, _ = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, B_MIN, B_MAX, RES, 0.3)
    for direction in ("front", "left"):
        x, y, z, _, count = ops.forward_vertices_raw(vol, direction)
        c = int(count.item())
        assert c > 500
        m = color_matrix(B_MIN, B_MAX, r)
        pts = ops.vertex_points(x, y, z, count, r, m)[:, :c]
        verts = torch.stack([x[:c].float(), y[:c].float(), float(r) - z[:c]])
        orth = ops.orthogonal(verts[None].contiguous(), torch.from_numpy(m)[None].to(DEV))[0]
        assert torch.equal(pts, orth)
        p = pts.cpu().numpy()
        vv = verts.cpu().numpy()
        m64 = m.astype(np.float64)
        want = m64[:3, :3] @ vv.astype(np.float64) + m64[:3, 3:4]
        mag = np.maximum(np.abs(m64[:3, :3] @ vv.astype(np.float64)), np.abs(m64[:3, 3:4]))
        assert (np.abs(p - want) <= 2 * np.spacing(mag.astype(np.float32))).all()
        for k in range(3):
            own = ((m[k, k] * vv[k]).astype(np.float32) + m[k, 3]).astype(np.float32)
            assert np.array_equal(p[k], own), k


def test_frame_pipeline_on_box_b_matches_direct_calls(ops):
    """FramePipeline(b_min = B, balance = 0.3, netC, hipGraph encoder, slots of 2): given the slot's own features,
    status, volume, normal render and texture render equal the direct calls with the same arguments bit for bit.
    (forward_vertices keeps its own 0.5: the reference's recon.py:56-60 constant, not the octree's balance.)"""
    from bench_common import build_netc, build_netg
    from monoport_amd.pipeline import FramePipeline
    from monoport_amd.recon import color_matrix, pifu_calib
    netG, _ = build_netg(DEV, "f32")
    netC = build_netc(DEV)
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(DEV)
    planes_hwc = planes.permute(1, 2, 0).contiguous()

    def hook(feat):
        feat[:, 0:2].copy_(planes[None].expand(feat.shape[0], -1, -1, -1))

    hook.hwc = lambda feat_hwc: feat_hwc[..., 0:2].copy_(planes_hwc[None].expand(feat_hwc.shape[0], -1, -1, -1))
    res = RES
    r = res[-1]
    pipe = FramePipeline(netG, DEV, depth=2, batch=2, resolutions=res, b_min=B_MIN, b_max=B_MAX, balance=0.3,
                         feature_hook=hook, use_graph=True, netC=netC)
    try:
        pipe.prepare()
        images = [torch.from_numpy(syn.synthetic_image(i))[None].to(DEV) for i in range(4)]
        calibs = [pifu_calib(*syn.scene_camera(9 * i + 30), device=DEV) for i in range(4)]
        got = []
        for s0 in (0, 2):
            slot = pipe.submit(images[s0:s0 + 2], calibs[s0:s0 + 2])
            slot.wait()
            assert np.array_equal(slot.mat_color, color_matrix(B_MIN, B_MAX, r))
            for b in range(2):
                got.append(dict(feat=slot.feats_hwc[b].clone(), feat_c=slot.feats_hwc_c[b].clone(),
                                status=slot.status[b].clone(), volume=slot.volumes[b].clone(),
                                render=slot.renders[b].clone(), tex=slot.renders_tex[b].clone(),
                                tables=slot.tables is not None))
        mlp = netG.surface_classifier.packed()
        mlp_c = netC.surface_classifier.packed()
        mat = color_matrix(B_MIN, B_MAX, r)
        for f, g in enumerate(got):
            with torch.no_grad():
                table = ops.skip_table(mlp, g["feat"]) if g["tables"] else None
                try:
                    vol, st = ops.recon(mlp, g["feat"], calibs[f], syn.Z_SCALE, B_MIN, B_MAX, res, 0.3)
                    x, y, z, n, c = ops.forward_vertices_raw(vol, "front")
                    render = ops.paint(x, y, n, 0, c, r, 0.5, 0.5, 0.0, 1.0)
                    pts = ops.vertex_points(x, y, z, c, r, mat)
                    pred = ops.query_counted(mlp_c, g["feat_c"], pts, c, calibs[f], syn.Z_SCALE)
                    tex = ops.paint(x, y, pred, 1, c, r, 0.5, 0.5, -np.inf, np.inf)
                    torch.cuda.synchronize()
                finally:
                    if table is not None:
                        table.release()
            assert int(st[0]) == 1 and int(c.item()) > 500, f
            assert torch.equal(st, g["status"]), f
            assert torch.equal(vol, g["volume"]), f
            assert torch.equal(render, g["render"]), f
            assert torch.equal(tex, g["tex"]), f
        assert len({tuple(g["status"].tolist()) for g in got}) > 1
    finally:
        pipe.close()
