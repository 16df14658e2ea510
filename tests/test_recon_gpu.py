"""GPU parity of the octree driver, forward_vertices and colorization kernels.  Needs an MI355X."""
import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def body(ops, oracle):
    layers = syn.body_mlp("G", noise=0.05, seed=1)
    f = syn.body_feat(256, 128, 128, 2)
    calib = oracle.pifu_calib(*syn.scene_camera(30))
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    cal = torch.from_numpy(calib).to(DEV)

    def gpu_query(pts):  # [3,N] numpy -> [N] numpy through the HIP kernel
        out = ops.query(mlp, fh, torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV), cal,
                        syn.Z_SCALE)
        return out[0, 0].cpu().numpy()

    return dict(layers=layers, f=f, calib=calib, mlp=mlp, fh=fh, cal=cal, gpu_query=gpu_query)


@pytest.mark.parametrize("res", [[9, 17, 33], [17, 33, 65], [17, 33, 65, 129]])
def test_recon_bit_exact_vs_oracle_driver(ops, oracle, body, res):
    """The HIP octree must make exactly the decisions of the CPU restatement.  Both sides get
    their occupancies from the same HIP query kernel, so the volumes must be identical bits."""
    vol, status = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, res)
    torch.cuda.synchronize()
    status = status.cpu().numpy()
    stats = []
    ref = oracle.seg3d_lossless(body["gpu_query"], BMIN, BMAX, res, stats=stats)
    assert status[0] == 1
    assert list(status[1:]) == stats
    v = vol.cpu().numpy()
    assert v.shape == ref.shape
    assert np.array_equal(v, ref)


def test_recon_matches_cpu_oracle_field(ops, oracle, body):
    """... and against the all-CPU oracle (CPU query) the field agrees to 1e-4 and the
    thresholded volume is identical (margin-checked)."""
    res = [9, 17, 33, 65]
    vol, status = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, res)
    q = lambda p: oracle.query(body["f"], p, body["calib"][0], body["layers"], 1, syn.Z_SCALE,
                               precision="f32")[0]
    ref = oracle.seg3d_lossless(q, BMIN, BMAX, res)
    v = vol.cpu().numpy()
    assert np.abs(v - ref).max() <= 1e-4
    safe = np.abs(ref - 0.5) > 1e-3
    assert np.array_equal((v > 0.5)[safe], (ref > 0.5)[safe])


def test_recon_empty_sets_status_zero(ops, body):
    layers = syn.body_mlp("G", c=-3.0)  # occupancy < 0.5 everywhere
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    vol, status = ops.recon(mlp, body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, [9, 17, 33])
    s = status.cpu().numpy()
    assert s[0] == 0 and s[1] == 9 ** 3 and s[2] == 0 and s[3] == 0


def test_recon_rejects_bad_resolutions(ops, body):
    from monoport_amd._lib import MonoportError
    with pytest.raises(MonoportError):
        ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, [9, 18])


@pytest.mark.parametrize("res,seed", [(33, 51), (65, 52)])
@pytest.mark.parametrize("direction", ["front", "back", "left", "right"])
def test_forward_vertices_vs_reference(ops, res, seed, direction):
    g = load_golden("forward_vertices")
    vol = torch.from_numpy(syn.blob_volume(res, seed)).to(DEV)
    x, y, z, n, count = ops.forward_vertices_raw(vol[None, None], direction)
    c = int(count.item())
    key = "r%d_%s_" % (res, direction)
    assert c == g[key + "X"].shape[0]
    assert np.array_equal(x[:c].cpu().numpy(), g[key + "X"])
    assert np.array_equal(y[:c].cpu().numpy(), g[key + "Y"])
    assert np.abs(z[:c].cpu().numpy() - g[key + "Z"]).max() <= 1e-4
    assert np.abs(n[:c].cpu().numpy() - g[key + "norm"]).max() <= 1e-5


@pytest.mark.parametrize("direction", ["front", "left"])
def test_forward_vertices_and_paint_batches_equal_single_calls(ops, direction):
    """mp_forward_vertices_batch / mp_paint_batch (all frames of a pipeline slot in one set of launches) give,
    frame by frame, the bits of the per-frame calls -- volumes with different surfaces, an EMPTY one included."""
    vols = [torch.from_numpy(syn.blob_volume(65, 60 + i)).to(DEV) for i in range(5)]
    vols[3] = torch.zeros_like(vols[3])
    single = [ops.forward_vertices_raw(v, direction) for v in vols]
    batch = ops.forward_vertices_raw_batch(vols, direction)
    for (x, y, z, n, c), (bx, by, bz, bn, bc) in zip(single, batch):
        k = int(c.item())
        assert k == int(bc.item())
        assert torch.equal(x[:k], bx[:k]) and torch.equal(y[:k], by[:k])
        assert torch.equal(z[:k], bz[:k]) and torch.equal(n[:k], bn[:k])
    assert int(batch[3][4].item()) == 0 and int(batch[0][4].item()) > 50
    one = [ops.paint(x, y, n, 0, c, 65, 0.5, 0.5, 0.0, 1.0) for x, y, z, n, c in single]
    many = ops.paint_batch([b[0] for b in batch], [b[1] for b in batch], [b[3] for b in batch], 0, [b[4] for b in batch],
                           65, 0.5, 0.5, 0.0, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(one, many))
    assert bool((many[3] == 1.0).all())


def test_forward_vertices_nan_at_front_face(ops, oracle):
    """A hit at z'=0 divides 0/0 in the reference: compare NaN for NaN."""
    vol = syn.blob_volume(33, 77)
    vol[-1, 10:14, 10:14] = 0.9  # occupied on the z' = 0 face
    x, y, z, n, count = ops.forward_vertices_raw(torch.from_numpy(vol).to(DEV), "front")
    c = int(count.item())
    rx, ry, rz, rn = oracle.forward_vertices(vol, "front")
    assert c == rx.shape[0] and np.array_equal(x[:c].cpu().numpy(), rx)
    zz = z[:c].cpu().numpy()
    assert np.isnan(rz).sum() > 0 and np.array_equal(np.isnan(zz), np.isnan(rz))
    ok = ~np.isnan(rz)
    assert np.abs(zz[ok] - rz[ok]).max() <= 1e-4


def test_colorization_vs_reference(ops):
    g = load_golden("colorization")
    res = 33
    vol = torch.from_numpy(syn.blob_volume(res, 63)).to(DEV)
    x, y, z, n, count = ops.forward_vertices_raw(vol, "front")
    img_n = ops.paint(x, y, n, 0, count, res, 0.5, 0.5, 0.0, 1.0)
    assert np.abs(img_n.cpu().numpy() - g["norm_image"]).max() <= 1e-5
    mlp = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("C", 61, 2.0), 2)
    fh = ops.pack_features(torch.from_numpy(syn.rand_feat(512, 128, 128, 62))[None].to(DEV))
    mat = np.eye(4, dtype=np.float32)
    for i in range(3):
        mat[i, i] = np.float32(2.0) / np.float32(res)
    mat[0:3, 3] = -1.0
    pts = ops.vertex_points(x, y, z, count, res, mat)
    preds = ops.query_counted(mlp, fh, pts, count, torch.from_numpy(g["calib"]).to(DEV), syn.Z_SCALE)
    img_t = ops.paint(x, y, preds, 1, count, res, 0.5, 0.5, -np.inf, np.inf)
    assert np.abs(img_t.cpu().numpy() - g["tex_image"]).max() <= 1e-4


def test_query_counted_batch_equals_per_frame_calls(ops):
    """The colour queries of all frames of a slot in ONE launch (mp_query_counted_batch) give the
    bits of one mp_query_counted per frame: different maps, calibrations and device-side counts
    (including an empty frame)."""
    mlp = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("C", 61, 2.0), 2)
    cap, counts_host = 5000, [4097, 0, 64, 5000, 1]
    feats, pts, cnts, cals = [], [], [], []
    for i, c in enumerate(counts_host):
        feats.append(ops.pack_features(torch.from_numpy(syn.rand_feat(512, 128, 128, 70 + i))[None].to(DEV)))
        pts.append(torch.from_numpy(syn.rand_points(cap, 80 + i, 1.0)).to(DEV).contiguous())
        cnts.append(torch.tensor([c], dtype=torch.int32, device=DEV))
        cal = np.eye(4, dtype=np.float32)[None]
        cal[0, 0, 0] = 1.0 - 0.05 * i
        cals.append(torch.from_numpy(cal).to(DEV))
    outs = ops.query_counted_batch(mlp, feats, pts, cnts, cals, syn.Z_SCALE)
    for i, c in enumerate(counts_host):
        one = ops.query_counted(mlp, feats[i], pts[i], cnts[i], cals[i], syn.Z_SCALE)
        assert torch.equal(outs[i], one), i
        assert float(outs[i][:, c:].abs().max()) == 0.0 if c < cap else True
        if c:
            assert float(outs[i][:, :c].abs().max()) > 0.0


def _sphere(r, radius=0.6, sharp=8.0):
    g = ((np.arange(r) + 0.5) / r) * 2 - 1
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    d = np.sqrt(x * x + y * y + z * z)
    return (1.0 / (1.0 + np.exp(-sharp * (radius - d) / radius))).astype(np.float32)


@pytest.mark.parametrize("name", ["blob33", "sphere65", "empty9", "recon129"])
def test_marching_cubes_identical_connectivity(ops, oracle, body, name):
    """Triangle connectivity identical to the CPU oracle, vertices to 1e-6 (self-parity: the
    reference has no marching cubes)."""
    from monoport_amd.recon import marching_cubes
    if name == "blob33":
        vol = syn.blob_volume(33, 5)
    elif name == "sphere65":
        vol = _sphere(65)
    elif name == "empty9":
        vol = np.zeros((9, 9, 9), np.float32)
    else:
        v, _ = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX,
                         [17, 33, 65, 129])
        vol = v.cpu().numpy()
    verts, faces = marching_cubes(torch.from_numpy(vol).to(DEV)[None, None], 0.5, BMIN, BMAX)
    rv, rf = oracle.marching_cubes(vol, 0.5, BMIN, BMAX)
    assert tuple(verts.shape) == rv.shape and tuple(faces.shape) == rf.shape
    assert faces.dtype == torch.int32 and np.array_equal(faces.cpu().numpy(), rf)
    if len(rv):
        assert np.abs(verts.cpu().numpy() - rv).max() <= 1e-6


def test_marching_cubes_capacity_retry_and_none(ops, oracle):
    from monoport_amd.recon import marching_cubes
    assert marching_cubes(None) == (None, None)
    vol = torch.from_numpy(_sphere(33)).to(DEV)
    v, f, counts = ops.marching_cubes_raw(vol, max_verts=10, max_faces=10)
    nv, nf = counts.cpu().tolist()
    rv, rf = oracle.marching_cubes(_sphere(33))
    assert (nv, nf) == (len(rv), len(rf))  # needed sizes are reported even when truncated
    assert np.array_equal(f.cpu().numpy(), rf[:10])


@pytest.mark.parametrize("res", [[17, 33, 65, 129, 257], [17, 33, 65, 129, 257, 513]])
def test_full_size_properties(ops, oracle, body, res):
    """BASELINE sizes (257^3 and 513^3): size-independent properties of the coarse-to-fine volume.  (The
    reference-anchored comparisons at these sizes are tests/test_baseline_size_gpu.py -- 257^3 -- and
    tests/test_config5_gpu.py -- 513^3, incl. the octree bit for bit against the CPU restatement.)"""
    vol, status = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, res)
    st = status.cpu().numpy()
    r = res[-1]
    assert st[0] == 1 and st[1] == res[0] ** 3
    assert 0 < st[-1] < 0.05 * r ** 3  # the last level stays sparse
    # (1) "lossless": on a random sample of ALL nodes the thresholded octree volume equals the
    #     thresholded direct evaluation (dense evaluation of r^3 nodes is 40+ TFLOP)
    rs = np.random.RandomState(r)
    allpick = rs.randint(0, r, size=(50000, 3))
    direct_all = body["gpu_query"](oracle.lattice_points(allpick, 1, r, BMIN, BMAX))
    got_all = vol[allpick[:, 0], allpick[:, 1], allpick[:, 2]].cpu().numpy()
    assert np.array_equal(got_all > 0.5, direct_all > 0.5)
    # (2) surface voxels carry exact network values: the first-hit voxels of forward_vertices are
    #     occupied nodes with an empty neighbour in front; re-query them directly
    xf, yf, zf, _, cf = ops.forward_vertices_raw(vol, "front")
    nf = int(cf.item())
    z1 = (r - 1) - torch.ceil(zf[:nf]).long().clamp(0, r - 1)  # Z interpolates between z'-2 and z'
    pick = torch.stack([z1, yf[:nf], xf[:nf]], 1)[:20000].cpu().numpy()
    direct = body["gpu_query"](oracle.lattice_points(pick, 1, r, BMIN, BMAX))
    got = vol[pick[:, 0], pick[:, 1], pick[:, 2]].cpu().numpy()
    assert (got == direct).mean() >= 0.99 and np.abs(got - direct).max() < 0.5
    # (3) idempotence: the same call again gives the same bits
    vol2, _ = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, res)
    assert torch.equal(vol, vol2)
    # (4) a closed surface: forward_vertices from front and back see the same silhouette
    xb, yb, _, _, cb = ops.forward_vertices_raw(vol, "back")
    nb = int(cb.item())
    assert nf == nb and torch.equal(xf[:nf], xb[:nb]) and torch.equal(yf[:nf], yb[:nb])


def test_generic_query_func_engine(ops, oracle, body):
    """Seg3dLossless with an ARBITRARY query function (not a MonoPortNet): an analytic sphere.
    Must equal the CPU restatement driven by the same function."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless

    def sphere_np(p):  # [3,N] numpy
        d = np.sqrt((p.astype(np.float32) ** 2).sum(0, dtype=np.float32))
        return (1.0 / (1.0 + np.exp(-(np.float32(0.6) - d) * np.float32(12)))).astype(np.float32)

    def query_func(points, scale):  # torch, [1,N,3] -> [1,1,N]
        d = torch.sqrt((points[0] ** 2).sum(1))
        return torch.sigmoid((0.6 - d) * scale)[None, None]

    res = [9, 17, 33, 65]
    eng = Seg3dLossless(query_func=query_func, b_min=np.array([[-1., -1., -1.]]),
                        b_max=np.array([[1., 1., 1.]]), resolutions=res, faster=True).to(DEV)
    sdf = eng(scale=12.0)
    assert sdf.shape == (1, 1, 65, 65, 65)
    stats = []
    ref = oracle.seg3d_lossless(sphere_np, BMIN, BMAX, res, stats=stats)
    assert list(eng.last_status[1:].numpy()) == stats
    v = sdf[0, 0].cpu().numpy()
    assert np.abs(v - ref).max() <= 2e-6  # torch.sigmoid vs numpy exp
    assert np.array_equal(v > 0.5, ref > 0.5)
    # empty scene -> None
    eng2 = Seg3dLossless(query_func=lambda points: torch.zeros(1, 1, points.shape[1], device=DEV),
                         b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]),
                         resolutions=[9, 17]).to(DEV)
    assert eng2() is None


def test_non_faster_mode_equals_oracle_and_flags(ops, oracle, body, monkeypatch):
    """Seg3dLossless(faster=False): 3^3 boxes + conflict re-examination through the
    level-at-a-time engine -- same volume and per-level counts as the CPU restatement driven by
    the same HIP query kernel.  Plus the constructor contract: unsupported flags raise."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    # the CPU restatement is driven by the PLAIN query kernel (body["gpu_query"]): keep netG.query on
    # it too (bit-for-bit comparison of the schedules, not of two roundings of the field)
    monkeypatch.setattr(ops, "SKIP_TABLE", False)
    from monoport_amd.modeling import PIFuNetG
    netG = PIFuNetG().eval()
    netG.surface_classifier.load_state_dict(
        {**{"filters.%d.weight" % i: torch.from_numpy(w)[:, :, None] for i, (w, _) in enumerate(body["layers"])},
         **{"filters.%d.bias" % i: torch.from_numpy(b) for i, (_, b) in enumerate(body["layers"])}})
    netG.surface_classifier.to(DEV)
    feats = [[torch.from_numpy(body["f"])[None].to(DEV)]]

    def query_func(points, feats, calib):
        return netG.query(feats, points.permute(0, 2, 1), calib)[0]

    res = [9, 17, 33, 65, 129]
    box = dict(b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]), resolutions=res)
    eng = Seg3dLossless(query_func=query_func, faster=False, **box).to(DEV)
    sdf = eng(feats=feats, calib=body["cal"])
    assert eng.last_path == "generic"
    stats, rounds = [], []
    ref = oracle.seg3d_lossless(body["gpu_query"], BMIN, BMAX, res, stats=stats, faster=False,
                                rounds=rounds)
    assert list(eng.last_status[1:].numpy()) == stats and sum(rounds) >= 1
    assert np.array_equal(sdf[0, 0].cpu().numpy(), ref)
    # faster=True on the same closure takes the fused path and a different (9/7/3) schedule
    eng_f = Seg3dLossless(query_func=query_func, faster=True, use_cuda_impl=True, debug=True, **box).to(DEV)
    sdf_f = eng_f(feats=feats, calib=body["cal"])
    assert eng_f.last_path == "fused"
    assert list(eng_f.last_status[1:].numpy()) != stats
    assert torch.equal(sdf_f > 0.5, sdf > 0.5)
    for bad in (dict(align_corners=True), dict(visualize=True), dict(use_shadow=True), dict(channels=2)):
        with pytest.raises(NotImplementedError):
            Seg3dLossless(query_func=query_func, **box, **bad)
    with pytest.warns(UserWarning, match="ignoring unknown arguments"):  # upstream swallows **kwargs
        Seg3dLossless(query_func=query_func, no_such_flag=1, **box)


def test_engine_trusts_a_query_func_after_validated_calls(ops, oracle, body):
    """The 17^3 validation query runs for the first VALIDATE_CALLS frames; after that many agreeing
    calls the fused engine is bound through a one-point probe (no validation query, one host sync).
    Results are identical either way; validate="always" keeps the check; a changed head re-validates."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    import torch
    netG = PIFuNetG().eval()
    netG.surface_classifier.load_state_dict(
        {**{"filters.%d.weight" % i: torch.from_numpy(w)[:, :, None] for i, (w, _) in enumerate(body["layers"])},
         **{"filters.%d.bias" % i: torch.from_numpy(b) for i, (_, b) in enumerate(body["layers"])}})
    netG.surface_classifier.to(DEV)
    feats = [[torch.from_numpy(body["f"])[None].to(DEV)]]
    calls = []

    def query_func(points, feats, calib):
        calls.append(points.shape[1])
        return netG.query(feats, points.permute(0, 2, 1), calib)[0]

    res = [9, 17, 33, 65]
    # the class default validates EVERY call (a drop-in must honour a closure that changes between frames)
    dflt = Seg3dLossless(query_func=query_func, faster=True, b_min=np.array([[-1., -1., -1.]]),
                         b_max=np.array([[1., 1., 1.]]), resolutions=res).to(DEV)
    assert dflt.validate == "always"
    for frame in range(dflt.VALIDATE_CALLS + 2):
        dflt(feats=feats, calib=body["cal"])
    assert calls == [729] * (dflt.VALIDATE_CALLS + 2) and dflt.last_path == "fused"
    del calls[:]
    eng = Seg3dLossless(query_func=query_func, faster=True, b_min=np.array([[-1., -1., -1.]]),
                        b_max=np.array([[1., 1., 1.]]), resolutions=res, validate="first").to(DEV)
    vols = []
    for frame in range(eng.VALIDATE_CALLS + 2):
        vols.append(eng(feats=feats, calib=body["cal"]))
        assert eng.last_path == "fused"
    # validated frames evaluate the 9^3 lattice through query_func, trusted ones only probe one point
    assert calls == [729] * eng.VALIDATE_CALLS + [1, 1]
    assert all(torch.equal(v, vols[0]) for v in vols[1:])
    eng.validate = "always"
    eng(feats=feats, calib=body["cal"])
    assert calls[-1] == 729
    eng.validate = "first"
    netG.surface_classifier.set_precision("f16x3")  # another packed head: trust is dropped
    eng(feats=feats, calib=body["cal"])
    assert calls[-1] == 729 and eng.last_path == "fused"


def test_wrapped_query_func_is_not_short_circuited(ops, oracle, body, monkeypatch):
    """A query_func that does arithmetic AROUND MonoPortNet.query (here 1 - pred on mirrored
    points) must be honoured: the engine notices that the fused kernel's coarsest level differs
    from what the function returned and evaluates every level through the function.  An exception
    inside query_func propagates instead of being swallowed."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    monkeypatch.setattr(ops, "SKIP_TABLE", False)  # the oracle side runs the plain kernel (body["gpu_query"])
    from monoport_amd.modeling import PIFuNetG
    netG = PIFuNetG().eval()
    netG.surface_classifier.load_state_dict(
        {**{"filters.%d.weight" % i: torch.from_numpy(w)[:, :, None] for i, (w, _) in enumerate(body["layers"])},
         **{"filters.%d.bias" % i: torch.from_numpy(b) for i, (_, b) in enumerate(body["layers"])}})
    netG.surface_classifier.to(DEV)
    feats = [[torch.from_numpy(body["f"])[None].to(DEV)]]

    def wrapped(points, feats, calib):
        mirrored = points * torch.tensor([-1.0, 1.0, 1.0], device=points.device)
        return 1.0 - netG.query(feats, mirrored.permute(0, 2, 1), calib)[0]

    def wrapped_np(p):  # the same function on the oracle side, through the same HIP kernel
        q = p.copy()
        q[0] = -q[0]
        return (np.float32(1.0) - body["gpu_query"](q)).astype(np.float32)

    res = [9, 17, 33, 65]
    box = dict(b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]), resolutions=res)
    eng = Seg3dLossless(query_func=wrapped, faster=True, **box).to(DEV)
    with pytest.warns(UserWarning, match="not a plain MonoPortNet.query"):
        sdf = eng(feats=feats, calib=body["cal"])
    assert eng.last_path == "generic"
    stats = []
    ref = oracle.seg3d_lossless(wrapped_np, BMIN, BMAX, res, stats=stats)
    assert list(eng.last_status[1:].numpy()) == stats
    assert np.array_equal(sdf[0, 0].cpu().numpy(), ref)

    def broken(points, feats, calib):
        raise RuntimeError("bug inside query_func")

    with pytest.raises(RuntimeError, match="bug inside query_func"):
        Seg3dLossless(query_func=broken, faster=True, **box).to(DEV)(feats=feats, calib=body["cal"])


def test_recon_f16x3_bit_exact_vs_oracle_driver(ops, oracle):
    """Octree driven by the f16x3 kernel: same decisions as the CPU restatement fed by the same
    kernel, and the same thresholded volume as the f32 path."""
    layers = syn.body_mlp("G", noise=0.05, seed=1)
    f = syn.body_feat(256, 128, 128, 2)
    cal = torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(30))).to(DEV)
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    res = [17, 33, 65, 129]
    vol32, st32 = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, res)
    mlp.set_precision("f16x3")
    vol16, st16 = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, res)

    def gpu_query(pts):
        return ops.query(mlp, fh, torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV), cal,
                         syn.Z_SCALE)[0, 0].cpu().numpy()

    stats = []
    ref = oracle.seg3d_lossless(gpu_query, BMIN, BMAX, res, stats=stats)
    assert list(st16.cpu().numpy()[1:]) == stats
    assert np.array_equal(vol16.cpu().numpy(), ref)
    assert (vol16 - vol32).abs().max().item() <= 2e-6
    assert torch.equal(vol16 > 0.5, vol32 > 0.5) and torch.equal(st16, st32)


@pytest.mark.parametrize("precision", ["f16w", "f16"])
def test_config5_513_fp16_weights(ops, oracle, precision):
    """BASELINE configs[4]: octree to 513^3 with fp16 weights, against OUR f32 volume (how much the
    arithmetic moves the result).  The config's parity statement -- against the REFERENCE's values -- is
    tests/test_config5_gpu.py::test_pipeline513_fp16_weights_vs_reference."""
    layers = syn.body_mlp("G", noise=0.05, seed=1)
    f = syn.body_feat(256, 128, 128, 2)
    cal = torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(30))).to(DEV)
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    res = [17, 33, 65, 129, 257, 513]
    vol32, st32 = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, res)
    occ32 = vol32 > 0.5
    mlp.set_precision(precision)
    vol16, st16 = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, res)
    occ16 = vol16 > 0.5
    inter = (occ32 & occ16).sum().item()
    union = (occ32 | occ16).sum().item()
    dmax = (vol16 - vol32).abs().max().item()
    print("513^3 %s: IoU %.6f, max |delta occ| %.3g, points %s vs f32 %s"
          % (precision, inter / union, dmax, st16.cpu().tolist()[1:], st32.cpu().tolist()[1:]))
    assert st16[0].item() == 1
    assert inter / union >= (0.9999 if precision == "f16w" else 0.999)
    # the analytic body has a slope of k = 40 through the surface, which amplifies operand rounding:
    # plain f16 moves single near-surface values by up to ~0.2 while the surface itself stays put
    assert dmax <= (1e-3 if precision == "f16w" else 0.5)


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16w", "f16"])
def test_recon_batch_equals_single_frames(ops, oracle, precision):
    """mp_recon_batch (one fused-query launch per level for all frames) is bit-identical to one
    mp_recon per frame: different feature maps and cameras per frame, including an EMPTY frame."""
    layers = syn.body_mlp("G", noise=0.05, seed=1)
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    mlp.set_precision(precision)
    res = [17, 33, 65, 129]
    feats, cals = [], []
    for i in range(5):
        f = syn.body_feat(256, 128, 128, 2 + i)
        feats.append(ops.pack_features(torch.from_numpy(f)[None].to(DEV)))
        calib = oracle.pifu_calib(*syn.scene_camera(25 * i))
        if i == 3:
            calib[0, 0, 3] = 5.0  # camera looks past the box: every node projects out of the image
        cals.append(torch.from_numpy(calib).to(DEV))
    vols, status = ops.recon_batch(mlp, feats, cals, syn.Z_SCALE, BMIN, BMAX, res)
    st = status.cpu().numpy()
    assert st[:, 1].tolist() == [17 ** 3] * 5
    for i in range(5):
        v1, s1 = ops.recon(mlp, feats[i], cals[i], syn.Z_SCALE, BMIN, BMAX, res)
        assert np.array_equal(s1.cpu().numpy(), st[i]), i
        if st[i, 0]:
            assert torch.equal(v1, vols[i]), i
    assert st[3, 0] == 0 and (st[[0, 1, 2, 4], 0] == 1).all()
    assert len({tuple(r) for r in st[:, 2:].tolist()}) > 1  # the frames really differ


_CHUNK_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from monoport_amd import ops, synthetic as syn
from monoport_amd.recon import pifu_calib
mlp = ops.PackedMLP.from_layers("cuda:0", syn.body_mlp("G", noise=0.05, seed=1), 1)
feats, cals = [], []
for i in range(5):
    feats.append(ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2 + i))[None].to("cuda:0")))
    cals.append(pifu_calib(*syn.scene_camera(25 * i), device="cuda:0"))
vols, status = ops.recon_batch(mlp, feats, cals, syn.Z_SCALE, [-1.0] * 3, [1.0] * 3, [17, 33, 65, 129])
np.savez(sys.argv[2], status=status.cpu().numpy(), vols=torch.stack(vols).cpu().numpy())
"""


@pytest.mark.parametrize("chunk", ["1", "2"])
def test_recon_batch_same_bits_for_any_housekeeping_chunk(ops, oracle, tmp_path, chunk):
    """The octree's housekeeping kernels take all frames of a call per launch (blockIdx.z = frame);
    MONOPORT_OCTREE_CHUNK (read once per process) cuts them into launches of that many frames -- frames
    f0 .. f0 + n of the call as frames 0 .. n of a launch.  Status rows and volumes do not depend on it."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "chunk.py"
    script.write_text(_CHUNK_SCRIPT)
    got = {}
    for c in (chunk, None):
        env = dict(os.environ)
        env.pop("MONOPORT_OCTREE_CHUNK", None)
        if c is not None:
            env["MONOPORT_OCTREE_CHUNK"] = c
        out = str(tmp_path / ("out_%s.npz" % c))
        res = subprocess.run([sys.executable, str(script), root, out], env=env, capture_output=True, text=True,
                             timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        got[c] = np.load(out)
    assert (got[None]["status"][:, 0] == 1).all()
    assert np.array_equal(got[chunk]["status"], got[None]["status"])
    assert np.array_equal(got[chunk]["vols"], got[None]["vols"])


def test_recon_batch_of_32_frames(ops, oracle):
    """The full frame set of one launch (kMaxFrames = 32), every frame with its own camera."""
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    fh = ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2))[None].to(DEV))
    res = [9, 17, 33, 65]
    cals = [torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(11 * i))).to(DEV) for i in range(32)]
    vols, status = ops.recon_batch(mlp, [fh] * 32, cals, syn.Z_SCALE, BMIN, BMAX, res)
    st = status.cpu().numpy()
    assert (st[:, 0] == 1).all() and len({tuple(r) for r in st[:, 2:].tolist()}) > 16
    for i in (0, 7, 8, 15, 16, 23, 31):
        v1, s1 = ops.recon(mlp, fh, cals[i], syn.Z_SCALE, BMIN, BMAX, res)
        assert np.array_equal(s1.cpu().numpy(), st[i]) and torch.equal(v1, vols[i]), i


def test_recon_batch_rejects_too_many_frames(ops, body):
    from monoport_amd._lib import MonoportError
    assert ops.MAX_FRAMES == 32
    with pytest.raises(MonoportError):
        ops.recon_batch(body["mlp"], [body["fh"]] * 33, [body["cal"]] * 33, syn.Z_SCALE, BMIN, BMAX,
                        [9, 17])
    # 32 frames (kMaxFrames) in one call, every level one launch: the same volume 32 times
    vols, st = ops.recon_batch(body["mlp"], [body["fh"]] * 32, [body["cal"]] * 32, syn.Z_SCALE, BMIN, BMAX, [9, 17, 33])
    one, st1 = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, [9, 17, 33])
    assert all(torch.equal(v, one) for v in vols) and all(torch.equal(s, st1) for s in st)


def _dense_iou(ops, mlp, fh, cal, vol, r):
    """Thresholded octree volume vs the dense evaluation of ALL r^3 lattice nodes."""
    c = (torch.arange(r, device=DEV, dtype=torch.float32) + 0.5) / r * 2 - 1
    inter = union = inside = 0
    for z0 in range(0, r, 16):
        z1 = min(z0 + 16, r)
        zz, yy, xx = torch.meshgrid(c[z0:z1], c, c, indexing="ij")
        pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)])[None].contiguous()
        dense = ops.query(mlp, fh, pts, cal, syn.Z_SCALE)[0, 0].reshape(z1 - z0, r, r)
        a, b = dense > 0.5, vol[z0:z1] > 0.5
        inter += int((a & b).sum().item())
        union += int((a | b).sum().item())
        inside += int(a.sum().item())
    return inter, union, inside


@pytest.mark.parametrize("figure,step,seed", [("figure", 0, 11), ("figure", 135, 12), ("thin", 60, 13),
                                              ("thin", 200, 14), ("two", 20, 15), ("two", 290, 16)])
def test_octree_lossless_other_bodies_and_cameras(ops, oracle, figure, step, seed):
    """The dense-evaluation check on more than one scene: the capsule figure from other sides, a
    figure with limbs ~2 voxels thin (the hard case for a 17^3 start: parts can fall between
    coarse nodes) and two disconnected bodies at different depths.  The coarse-to-fine scheme (the
    upstream one included) can only find what the 17^3 lattice plus the 9^3 / 7^3 / 3^3 dilations
    reach: on the thin figure limb tips, or a whole limb that no coarse node sees, are lost
    (measured at 257^3: IoU 0.9997 from one camera, 0.966 from another -- 1640 of 48 k inside
    nodes; CPU oracle at 129^3: 0.992-0.997, and 0.93 for the faster=False schedule, which
    starts from 3^3 boxes).  Bars: IoU >= 0.95 (thin) / 0.99999 (others); values are printed."""
    layers = syn.body_mlp("G", noise=0.05, seed=seed)
    f = syn.body_feat(256, 128, 128, seed + 100, figure=figure)
    cal = torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(step))).to(DEV)
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    res = [17, 33, 65, 129, 257]
    vol, status = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, res)
    inter, union, inside = _dense_iou(ops, mlp, fh, cal, vol, 257)
    print("%s @ camera %d: IoU %.7f (%d of %d inside nodes differ), queried %s"
          % (figure, step, inter / union, union - inter, inside, status.cpu().tolist()[1:]))
    assert status[0].item() == 1 and inside > 1000
    assert inter / union >= (0.95 if figure == "thin" else 0.99999)


@pytest.mark.parametrize("res", [[17, 33, 65, 129, 257], [17, 33, 65, 129, 257, 513]])
def test_octree_lossless_against_full_dense_evaluation(ops, body, res):
    """The defining property of the engine at BASELINE sizes, checked on EVERY node: the thresholded
    coarse-to-fine volume equals the thresholded dense evaluation of all R^3 lattice points
    (17 M / 135 M fused queries -- 0.3 s / 2.5 s on the GPU).  Measured: 1-4 differing nodes of
    17 M at 257^3, 12-17 of 135 M at 513^3 (isolated nodes whose trilinear estimate sits on the
    other side of 0.5); the bar is IoU >= 0.99999."""
    r = res[-1]
    vol, status = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, res)
    c = (torch.arange(r, device=DEV, dtype=torch.float32) + 0.5) / r * 2 - 1
    inter = union = exact = evaluated = 0
    for z0 in range(0, r, 16):
        z1 = min(z0 + 16, r)
        zz, yy, xx = torch.meshgrid(c[z0:z1], c, c, indexing="ij")
        pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)])[None].contiguous()
        dense = ops.query(body["mlp"], body["fh"], pts, body["cal"], syn.Z_SCALE)[0, 0]
        dense = dense.reshape(z1 - z0, r, r)
        a, b = dense > 0.5, vol[z0:z1] > 0.5
        inter += int((a & b).sum().item())
        union += int((a | b).sum().item())
        exact += int((dense == vol[z0:z1]).sum().item())
    n_queried = int(status[1:].sum().item())
    print("R=%d: IoU %.7f (%d differing nodes), %d nodes carry the exact network value, %d queried"
          % (r, inter / union, union - inter, exact, n_queried))
    assert inter / union >= 0.99999
    assert exact >= n_queried  # every queried node holds its exact value (plus coincidences)


def test_recon_same_bits_with_either_query_tile(ops, oracle):
    """The coarse octree levels run on the 32-point-tile query kernel, the fine ones on the
    64-point kernel (device-side gate at 2048 tiles): volumes and statuses equal the ones with the
    small kernel switched off / always on, single frames and batches."""
    from monoport_amd import _lib
    lib = _lib.load()
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    res = [17, 33, 65, 129, 257]
    feats = [ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2 + i))[None].to(DEV))
             for i in range(3)]
    cals = [torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(40 * i))).to(DEV) for i in range(3)]
    got = {}
    for mode in (0, -1, 1):
        lib.mp_query_tune(mode)
        try:
            v1, s1 = ops.recon(mlp, feats[0], cals[0], syn.Z_SCALE, BMIN, BMAX, res)
            vb, sb = ops.recon_batch(mlp, feats, cals, syn.Z_SCALE, BMIN, BMAX, res)
            got[mode] = (v1.clone(), s1.clone(), [v.clone() for v in vb], sb.clone())
        finally:
            lib.mp_query_tune(-1)
    for mode in (-1, 1):
        assert torch.equal(got[0][0], got[mode][0]) and torch.equal(got[0][1], got[mode][1])
        assert torch.equal(got[0][3], got[mode][3])
        for a, b in zip(got[0][2], got[mode][2]):
            assert torch.equal(a, b)
    assert int(got[0][1][0]) == 1


def test_table_query_kernel_is_repeatable_under_perturbed_timing(ops, oracle):
    """Race screen for pifu_query_tabws_kernel (producer / consumer waves meeting at 14 barriers per tile, LDS
    regions reused across intervals): the same 8-frame reconstruction and the same scattered query, repeated
    with another stream hammering the GPU in between so that waves interleave differently every time, must
    return the same bits every time -- and stay within f32 rounding of the plain fused kernels (every wave does
    everything, no hand-offs), which serve the same calls once the tables are released.  That run must also differ
    from the table kernel's in at least one bit: the comparison is between two implementations (measured on an
    MI355X: query 4.17e-07, volumes 5.96e-07)."""
    import torch
    dev = torch.device(DEV)
    mlp = ops.PackedMLP.from_layers(dev, syn.rand_mlp("G", 19, 2.0), 1)
    frames = 8
    feats = [ops.pack_features(torch.from_numpy(syn.rand_feat(256, 128, 128, 40 + i))[None].to(dev)) for i in range(frames)]
    cals = [torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(17 * i + 3))).to(dev) for i in range(frames)]
    pts = torch.from_numpy(syn.rand_points(200003, 5, 1.05))[None].to(dev)  # scattered: every point its own texels
    res = [17, 33, 65, 129]
    tables = [ops.skip_table(mlp, f) for f in feats]
    side = torch.cuda.Stream(device=dev)
    noise = torch.randn((4096, 4096), device=dev)

    def run():
        with torch.cuda.stream(side):  # unrelated work that comes and goes
            for _ in range(3):
                (noise @ noise).sum()
        q = ops.query(mlp, feats[0], pts, cals[0], syn.Z_SCALE)
        v, st = ops.recon_batch(mlp, feats, cals, syn.Z_SCALE, [-1] * 3, [1] * 3, res)
        return q.clone(), [x.clone() for x in v], st.clone()

    try:
        first = run()
        for rep in range(6):
            q, v, st = run()
            assert torch.equal(q, first[0]), rep
            assert torch.equal(st, first[2]) and all(torch.equal(a, b) for a, b in zip(v, first[1])), rep
    finally:
        ops.skip_table_release(mlp.ctx)
    q1, v1, st1 = run()  # no tables any more: the plain fused kernels
    torch.cuda.synchronize()
    dq = (q1 - first[0]).abs().max().item()
    dv = max((a - b).abs().max().item() for a, b in zip(v1, first[1]))
    print("table kernel: 7 identical runs; vs the plain kernels: query %.3g, volumes %.3g" % (dq, dv))
    assert dq > 0 and dv > 0  # another kernel really ran
    assert dq <= 2e-6
    # the rand head's field is not a body: volumes are compared where both kernels evaluated (the same nodes
    # unless a value sits within rounding of the threshold)
    assert dv <= 2e-6 or int(((v1[0] > 0.5) != (first[1][0] > 0.5)).sum()) < 50
    del tables


@pytest.mark.parametrize("rule", ["upstream", "interpolate"])
@pytest.mark.parametrize("res", [[9, 17, 33], [17, 33, 65, 129]])
def test_final_level_rules_bit_exact_vs_oracle_driver(ops, oracle, body, rule, res):
    """mp_recon_batch_ex(final_level=...): the HIP octree takes exactly the decisions of the CPU restatement
    of the same rule (both sides evaluate with the same HIP query kernel: identical volumes and counts),
    one frame alone and as frames of one batch call."""
    stats = []
    ref = oracle.seg3d_lossless(body["gpu_query"], BMIN, BMAX, res, stats=stats, final_level=rule)
    vol, status = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, res, final_level=rule)
    assert list(status.cpu().numpy()) == [1] + stats
    assert np.array_equal(vol.cpu().numpy(), ref)
    vols, st = ops.recon_batch(body["mlp"], [body["fh"]] * 3, [body["cal"]] * 3, syn.Z_SCALE, BMIN, BMAX, res,
                               final_level=rule)
    assert all(torch.equal(v, vol) for v in vols) and all(list(s) == [1] + stats for s in st.cpu().numpy())
    with pytest.raises(ValueError):
        ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, res, final_level="no-such-rule")


def test_final_level_rules_through_seg3d_lossless_257(ops, oracle, body):
    """Seg3dLossless(final_level=...) at BASELINE configs[1] size through the drop-in surface, fused AND
    level-at-a-time engines, with the honest price of the cheaper rules against DENSE evaluation of the
    257^3 lattice (17 M points through the same kernel): "dilate3" reproduces the dense inside-set exactly
    on this body, "upstream" (the rule recalled from the un-vendored package: mask == 0.5, undilated) and
    "interpolate" (no evaluation at 257^3) do not -- the numbers are printed and bounded."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    netG = PIFuNetG().eval()
    netG.surface_classifier.load_state_dict(
        {**{"filters.%d.weight" % i: torch.from_numpy(w)[:, :, None] for i, (w, _) in enumerate(body["layers"])},
         **{"filters.%d.bias" % i: torch.from_numpy(b) for i, (_, b) in enumerate(body["layers"])}})
    netG.surface_classifier.to(DEV)
    feats = [[torch.from_numpy(body["f"])[None].to(DEV)]]
    res = [17, 33, 65, 129, 257]
    box = dict(b_min=np.array([BMIN]), b_max=np.array([BMAX]), resolutions=res)

    def query_func(points, feats, calib):
        return netG.query(feats, points.permute(0, 2, 1), calib)[0]

    def wrapped(points, feats, calib):  # two netG.query calls: not fusable, the level-at-a-time engine serves it
        netG.query(feats, points[:, :1].permute(0, 2, 1), calib)
        return query_func(points, feats, calib)

    r = res[-1]
    g = ((torch.arange(r, device=DEV, dtype=torch.float32) / r) + (1.0 / r) / 2) * 2 - 1
    dense = torch.empty((r, r, r), device=DEV)
    for z in range(0, r, 32):  # dense 257^3 in slabs of 32 planes
        zz, yy, xx = torch.meshgrid(g[z:z + 32], g, g, indexing="ij")
        pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 0)[None]
        dense[z:z + 32] = netG.query(feats, pts, body["cal"])[0][0, 0].reshape(-1, r, r)
    inside = dense > 0.5
    n_in = int(inside.sum())
    got = {}
    for rule in ("dilate3", "upstream", "interpolate"):
        eng = Seg3dLossless(query_func=query_func, faster=True, final_level=rule, **box).to(DEV)
        sdf = eng(feats=feats, calib=body["cal"])
        assert eng.last_path == "fused"
        wrong = int(((sdf[0, 0] > 0.5) != inside).sum())
        inter = int(((sdf[0, 0] > 0.5) & inside).sum())
        union = int(((sdf[0, 0] > 0.5) | inside).sum())
        got[rule] = (sdf, eng.last_status.clone(), wrong)
        print("final_level=%-11s points per level %s (sum %d); %d of %d inside voxels differ from dense "
              "evaluation (%.3f %%), IoU %.5f" % (rule, eng.last_status[1:].tolist(), int(eng.last_status[1:].sum()),
                                                 wrong, n_in, 100.0 * wrong / n_in, inter / union))
        eng_g = Seg3dLossless(query_func=wrapped, faster=True, final_level=rule, **box).to(DEV)
        gen = eng_g(feats=feats, calib=body["cal"])
        assert eng_g.last_path == "generic" and eng_g.last_status.tolist() == eng.last_status.tolist()
        assert torch.equal(gen, sdf)  # the two engines take the same decisions under every rule
    d3, up, ip = got["dilate3"], got["upstream"], got["interpolate"]
    assert d3[2] <= 1e-4 * n_in  # lossless (a handful of voxels at most: values within fp32 noise of 0.5)
    assert d3[1][1:-1].tolist() == up[1][1:-1].tolist() == ip[1][1:-1].tolist()
    assert int(ip[1][-1]) == 0 and 0 < int(up[1][-1]) < 0.4 * int(d3[1][-1])
    assert 0 < up[2] <= 0.01 * n_in and up[2] <= ip[2] <= 0.08 * n_in
    with pytest.raises(NotImplementedError):
        Seg3dLossless(query_func=query_func, faster=False, final_level="upstream", **box)
    with pytest.raises(ValueError):
        Seg3dLossless(query_func=query_func, faster=True, final_level="nope", **box)


def _distinct_frames(ops, oracle, n, empty=None):
    """``n`` frames with their own feature maps (body_feat seed 2 + i) and cameras (scene_camera(25 i)); frame
    ``empty`` gets a camera that looks past the box, so every node projects out of the image."""
    feats, cals = [], []
    for i in range(n):
        feats.append(ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2 + i))[None].to(DEV)))
        calib = oracle.pifu_calib(*syn.scene_camera(25 * i))
        if i == empty:
            calib[0, 0, 3] = 5.0
        cals.append(torch.from_numpy(calib).to(DEV))
    return feats, cals


@pytest.mark.parametrize("rule", ["upstream", "interpolate"])
@pytest.mark.parametrize("res", [[17, 33, 65, 129], [17, 33, 65, 129, 257]])
def test_final_level_rules_batch_of_distinct_frames(ops, oracle, rule, res):
    """mp_recon_batch_ex(final_level=rule) over 7 frames with different feature maps and cameras, one of them
    empty: every frame's status row and volume = ops.recon(..., final_level=rule) on that frame alone, bit for bit
    (the rule's kernels index every buffer by frame: a kernel reading frame 0's buffers passes on identical
    frames), and frames 1 and 5 = the CPU restatement oracle.seg3d_lossless(final_level=rule) driven by the same
    HIP query kernel on that frame's map and camera (volume and points per level)."""
    import time
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    feats, cals = _distinct_frames(ops, oracle, 7, empty=4)
    vols, status = ops.recon_batch(mlp, feats, cals, syn.Z_SCALE, BMIN, BMAX, res, final_level=rule)
    st = status.cpu().numpy()
    assert st[:, 1].tolist() == [17 ** 3] * 7
    assert st[4, 0] == 0 and (st[[0, 1, 2, 3, 5, 6], 0] == 1).all()
    for i in range(7):
        v1, s1 = ops.recon(mlp, feats[i], cals[i], syn.Z_SCALE, BMIN, BMAX, res, final_level=rule)
        assert np.array_equal(s1.cpu().numpy(), st[i]), i
        if st[i, 0]:
            assert torch.equal(v1, vols[i]), i
    # the frames really differ: per-level counts, and every non-empty frame's volume against frame 0's
    assert len({tuple(r) for r in st[[0, 1, 2, 3, 5, 6], 2:].tolist()}) > 1
    assert all(not torch.equal(vols[i], vols[0]) for i in (1, 2, 3, 5, 6))
    last = st[[0, 1, 2, 3, 5, 6], -1]
    if rule == "interpolate":
        assert (last == 0).all()  # nothing is evaluated at the last level
    else:
        assert (last > 0).all()
    t0 = time.perf_counter()
    for i in (1, 5):
        def gpu_query(pts, i=i):
            return ops.query(mlp, feats[i], torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV), cals[i],
                             syn.Z_SCALE)[0, 0].cpu().numpy()

        stats = []
        ref = oracle.seg3d_lossless(gpu_query, BMIN, BMAX, res, stats=stats, final_level=rule)
        assert list(st[i]) == [1] + stats, i
        assert np.array_equal(vols[i].cpu().numpy(), ref), i
    print("final_level=%s, %d^3, 7 distinct frames: batch == single frames; frames 1 and 5 == oracle driver "
          "(%.1f s)" % (rule, res[-1], time.perf_counter() - t0))


@pytest.mark.parametrize("precision,res", [(p, [17, 33, 65, 129, 257]) for p in ("f16x3", "f16w", "f16")]
                         + [(p, [17, 33, 65, 129, 257, 513]) for p in ("f16w", "f16")])
def test_recon_batch_of_16_at_large_grids_equals_single_frames(ops, oracle, precision, res):
    """mp_recon_batch with the f16 heads at 257^3 and 513^3 (BASELINE configs[4] runs 16 frames of 17..513 per
    fused launch): 16 frames cycling through 5 distinct maps and cameras (frames 8 and 15 hold other inputs than
    frames 0 and 7), every frame = ops.recon on that frame alone, bit for bit.  At 513^3 every distinct frame's
    volume against the f32 head's on the same inputs: IoU >= 0.9999 (f16w) / 0.999 (f16), the bars of
    test_config5_513_fp16_weights."""
    import time
    t0 = time.perf_counter()
    layers = syn.body_mlp("G", noise=0.05, seed=1)
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    mlp.set_precision(precision)
    feats, cals = _distinct_frames(ops, oracle, 5)
    k = [f % 5 for f in range(16)]
    vols, status = ops.recon_batch(mlp, [feats[i] for i in k], [cals[i] for i in k], syn.Z_SCALE, BMIN, BMAX, res)
    st = status.cpu().numpy()
    assert (st[:, 0] == 1).all() and len({tuple(r) for r in st[:5, 2:].tolist()}) > 1
    assert all(not torch.equal(vols[i], vols[0]) for i in range(1, 5))  # the frames really differ
    ious = []
    for i in range(5):
        v1, s1 = ops.recon(mlp, feats[i], cals[i], syn.Z_SCALE, BMIN, BMAX, res)
        s1 = s1.cpu().numpy()
        for f in range(i, 16, 5):
            assert np.array_equal(s1, st[f]), f
            assert torch.equal(v1, vols[f]), f
        if res[-1] == 513:
            mlp32 = ops.PackedMLP.from_layers(DEV, layers, 1)
            v32, _ = ops.recon(mlp32, feats[i], cals[i], syn.Z_SCALE, BMIN, BMAX, res)
            occ32, occ16 = v32 > 0.5, v1 > 0.5
            ious.append((occ32 & occ16).sum().item() / (occ32 | occ16).sum().item())
            del v32, occ32, occ16, mlp32
        del v1
    del vols
    torch.cuda.empty_cache()
    print("recon_batch %s, 16 frames at %d^3 == single frames; IoU vs f32 %s (%.1f s)"
          % (precision, res[-1], ["%.6f" % v for v in ious], time.perf_counter() - t0))
    assert all(v >= (0.9999 if precision == "f16w" else 0.999) for v in ious)
