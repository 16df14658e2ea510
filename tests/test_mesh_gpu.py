"""mp_mesh_normals / mp_mesh_points (csrc/mesh.hip) and recon.reconstruct_mesh on the GPU: the normals bit for bit
against the reference's compute_normal (tests/golden/mesh_normals.npz) and against the np.add.at restatement, the
capacity / count contract, and the volume -> verts, faces -> normals -> colours chain.  Needs an MI355X."""
import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn
from test_mesh_normals_cpu import accumulate_model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def golden():
    return dict(load_golden("mesh_normals"))


def mesh_of(golden, name):
    if name == "soup":
        v, f, _ = syn.normals_soup_mesh()
        return v, f
    return golden[name + "_verts"], golden[name + "_faces"]


def expected(golden, name, mode):
    v, f = mesh_of(golden, name)
    return golden[name + "_ref32"] if mode == "reference" else accumulate_model(v, f.astype(np.int64))


def dev_mesh(v, f):
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    return tv, tf, torch.tensor([len(v), len(f)], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("mode", ["reference", "accumulate"])
@pytest.mark.parametrize("name", ["blob33", "sphere65", "soup"])
def test_normals_bit_for_bit(ops, golden, name, mode):
    v, f = mesh_of(golden, name)
    tv, tf, counts = dev_mesh(v, f)
    out = ops.mesh_normals_raw(tv, tf, counts, mode).cpu().numpy()
    want = expected(golden, name, mode)
    diff = out.view(np.uint32) != want.view(np.uint32)
    print("%s %s: %d of %d components differ in bits" % (name, mode, int(diff.sum()), diff.size))
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))  # bits: -0.0 and +0.0 are told apart
    assert not np.isnan(out).any()
    assert np.array_equal(tv.cpu().numpy(), v) and np.array_equal(tf.cpu().numpy(), f)


@pytest.mark.parametrize("mode", ["reference", "accumulate"])
def test_drop_in_on_device_tensors(ops, golden, mode):
    from monoport_amd import mesh_util
    v, f = mesh_of(golden, "blob33")
    tv, tf, _ = dev_mesh(v, f)
    out = mesh_util.compute_normal(tv, tf, mode)
    assert torch.is_tensor(out) and out.device == tv.device and out.dtype == torch.float32
    assert np.array_equal(out.cpu().numpy(), expected(golden, "blob33", mode))
    # faces as int64 / numpy, the reference's default mode
    assert np.array_equal(mesh_util.compute_normal(tv, f.astype(np.int64)).cpu().numpy(), golden["blob33_ref32"])
    # float64 on the device: the numpy definitions, returned where the input lives
    out64 = mesh_util.compute_normal(tv.double(), tf, "reference")
    assert out64.device == tv.device and np.array_equal(out64.cpu().numpy(), golden["blob33_ref64"])


@pytest.mark.parametrize("mode", ["reference", "accumulate"])
def test_counts_below_the_capacities(ops, golden, mode):
    """Rows beyond counts[0] stay untouched; faces beyond counts[1] (garbage indices) are never read as faces."""
    v, f = mesh_of(golden, "soup")
    nv, nf = len(v), len(f)
    vbuf = torch.full((nv + 300, 3), float("nan"), device=DEV)
    vbuf[:nv] = torch.from_numpy(v).to(DEV)
    fbuf = torch.full((nf + 500, 3), 2 ** 30, dtype=torch.int32, device=DEV)
    fbuf[:nf] = torch.from_numpy(f).to(DEV)
    fbuf[nf + 1] = torch.tensor([0, 1, 2], dtype=torch.int32)  # a valid face beyond the count must not contribute
    counts = torch.tensor([nv, nf], dtype=torch.int32, device=DEV)
    out = torch.full((nv + 300, 3), SENTINEL, device=DEV)
    res = ops.mesh_normals_raw(vbuf, fbuf, counts, mode, out=out)
    assert res is out
    got = out.cpu().numpy()
    assert np.array_equal(got[:nv], expected(golden, "soup", mode))
    assert (got[nv:] == SENTINEL).all()
    pts, count = ops.mesh_points_raw(vbuf, counts)
    assert pts.shape == (3, nv + 300) and int(count.item()) == nv
    assert np.array_equal(pts.cpu().numpy()[:, :nv], v.T) and (pts[:, nv:] == 0).all()


@pytest.mark.parametrize("mode", ["reference", "accumulate"])
@pytest.mark.parametrize("cap_v", [10, 30])
def test_counts_above_the_capacities(ops, golden, mode, cap_v):
    """A truncated marching cubes (10 or 30 vertices, 10 faces kept of thousands): only the capacities are read
    and written, faces that name vertices beyond the capacity are skipped (all ten of them at 10 vertices, four
    at 30), and the call succeeds."""
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    verts, faces, counts = ops.marching_cubes_raw(vol, 0.5, BMIN, BMAX, max_verts=cap_v, max_faces=10)
    assert counts.cpu().tolist() == [len(golden["blob33_verts"]), len(golden["blob33_faces"])]
    guard = 64
    big = torch.full((cap_v + 2 * guard, 3), SENTINEL, device=DEV)
    out = big[guard:guard + cap_v]
    ops.mesh_normals_raw(verts, faces, counts, mode, out=out)
    torch.cuda.synchronize()
    assert (big[:guard] == SENTINEL).all() and (big[guard + cap_v:] == SENTINEL).all()
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    assert np.array_equal(f, golden["blob33_faces"][:10])
    keep = f[(f < cap_v).all(1)]
    assert len(keep) == (0 if cap_v == 10 else 6)  # the other faces name later vertices
    from monoport_amd import mesh_util
    assert np.array_equal(out.cpu().numpy(), mesh_util.compute_normal(v, keep, mode))
    pbig = torch.full((3 * cap_v + 2 * guard,), SENTINEL, device=DEV)
    ctx = ops.get_context(verts.device)
    count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    pts = pbig[guard:guard + 3 * cap_v]
    ctx.check(ctx.lib.mp_mesh_points(ctx.handle, ops._ptr(verts), cap_v, ops._ptr(counts), ops._ptr(pts), ops._ptr(count),
                                     ops._stream(verts)), "mp_mesh_points")
    assert int(count.item()) == cap_v and np.array_equal(pts.view(3, cap_v).cpu().numpy(), v.T)
    assert (pbig[:guard] == SENTINEL).all() and (pbig[guard + 3 * cap_v:] == SENTINEL).all()


def test_accumulate_mode_is_the_same_bits_on_a_second_run(ops, golden):
    """The corner lists are filled in arrival order; the sum must not depend on it.  Two runs, on the mesh with
    the highest valence of the marching-cubes cases and on the 200-face fan."""
    for name in ("blob33", "soup"):
        v, f = mesh_of(golden, name)
        tv, tf, counts = dev_mesh(v, f)
        a = ops.mesh_normals_raw(tv, tf, counts, "accumulate").clone()
        b = ops.mesh_normals_raw(tv, tf, counts, "accumulate")
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    _, f, centre = syn.normals_soup_mesh()
    assert np.bincount(f.reshape(-1))[centre] >= 200


def test_bad_arguments(ops, golden):
    from monoport_amd._lib import MonoportError
    tv, tf, counts = dev_mesh(*mesh_of(golden, "blob33"))
    with pytest.raises(MonoportError):
        ops.mesh_normals_raw(tv, tf, counts, mode=7)
    with pytest.raises(ValueError):
        ops.mesh_normals_raw(tv, tf, counts, mode="area")
    with pytest.raises(ValueError):
        ops.mesh_normals_raw(tv.double(), tf, counts)
    with pytest.raises(ValueError):
        ops.mesh_normals_raw(tv, tf.long(), counts)
    ctx = ops.get_context(tv.device)
    rc = ctx.lib.mp_mesh_normals(ctx.handle, ops._ptr(tv), -1, ops._ptr(tf), tf.shape[0], ops._ptr(counts), 0,
                                 ops._ptr(tv), ops._stream(tv))
    assert rc == -1  # MP_ERR_ARG
    rc = ctx.lib.mp_mesh_normals(ctx.handle, None, tv.shape[0], ops._ptr(tf), tf.shape[0], ops._ptr(counts), 0,
                                 ops._ptr(tv), ops._stream(tv))
    assert rc == -1
    rc = ctx.lib.mp_mesh_points(ctx.handle, ops._ptr(tv), tv.shape[0], None, ops._ptr(tv), ops._ptr(counts),
                                ops._stream(tv))
    assert rc == -1
    # an empty mesh is fine
    e = ops.mesh_normals_raw(tv[:0], tf[:0], torch.zeros(2, dtype=torch.int32, device=DEV))
    assert e.shape == (0, 3)
    z = ops.mesh_normals_raw(tv, tf[:0], torch.tensor([tv.shape[0], 0], dtype=torch.int32, device=DEV))
    assert (z == 0).all()


# ---- the chain at the benchmark's size --------------------------------------------------------------------------

def _seeded_netC(v_n=1):
    from monoport_amd.modeling import PIFuNetC, heads
    netC = PIFuNetC()
    if v_n > 1:
        netC.surface_classifier = heads.SurfaceClassifier(heads.PIFuNetCMLP().filter_channels, v_n, False, "tanh")
    with torch.no_grad():
        for i, (w, b) in enumerate(syn.rand_mlp("C", 61, 2.0)):
            netC.surface_classifier.filters[i].weight.copy_(torch.from_numpy(w)[:, :, None])
            netC.surface_classifier.filters[i].bias.copy_(torch.from_numpy(b))
    netC.surface_classifier.to(DEV)
    return netC.eval()


@pytest.fixture(scope="module")
def body257(ops, oracle):
    """The `body` fixture of tests/test_recon_gpu.py reconstructed at 17..257 (the benchmark's resolutions)."""
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    fh = ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2))[None].to(DEV))
    cal = torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(30))).to(DEV)
    vol, status = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, [17, 33, 65, 129, 257])
    assert int(status[0].item()) == 1
    netC = _seeded_netC()
    feat_C = [[torch.from_numpy(syn.rand_feat(512, 128, 128, 62))[None].to(DEV)]]
    calib = torch.eye(4, device=DEV)[None]
    return dict(vol=vol[None, None], netC=netC, feat_C=feat_C, calib=calib)


def test_reconstruct_mesh_end_to_end(ops, body257, monkeypatch):
    from monoport_amd import mesh_util
    from monoport_amd.recon import Mesh, marching_cubes, reconstruct_mesh
    b = body257
    verts, faces = marching_cubes(b["vol"], 0.5, BMIN, BMAX)
    assert verts.shape[0] > 50000
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    mesh = reconstruct_mesh(b["vol"], 0.5, BMIN, BMAX, netC=b["netC"], feat_tensor_C=b["feat_C"],
                            calib_tensor=b["calib"])
    assert isinstance(mesh, Mesh)
    assert torch.equal(mesh.verts, verts) and torch.equal(mesh.faces, faces) and mesh.faces.dtype == torch.int32
    # the default is the intended behaviour (accumulate); both modes equal the numpy path on the downloaded mesh
    assert np.array_equal(mesh.normals.cpu().numpy(), mesh_util.compute_normal(v, f, "accumulate"))
    ref = reconstruct_mesh(b["vol"], 0.5, BMIN, BMAX, normals="reference")
    assert ref.colors is None and torch.equal(ref.verts, verts) and torch.equal(ref.faces, faces)
    assert np.array_equal(ref.normals.cpu().numpy(), mesh_util.compute_normal(v, f, "reference"))
    assert not torch.equal(ref.normals, mesh.normals)
    # colours: mesh_util.vertex_colors (netC.query -> mp_query) and the chain (mp_query_counted) both launch
    # pifu_query_kernel<512, 3> on the same points, so the colours are the same bits
    colors = mesh_util.vertex_colors(b["netC"], b["feat_C"], verts, b["calib"])
    assert mesh.colors.shape == verts.shape and mesh.colors.is_contiguous()
    assert float(mesh.colors.min()) >= 0 and float(mesh.colors.max()) <= 1
    print("colours: max |chain - vertex_colors| = %.3g" % float((mesh.colors - colors).abs().max()))
    assert torch.equal(mesh.colors, colors)
    none = reconstruct_mesh(b["vol"], 0.5, BMIN, BMAX, normals=None, netC=b["netC"], feat_tensor_C=b["feat_C"],
                            calib_tensor=b["calib"])
    assert none.normals is None and torch.equal(none.colors, colors) and torch.equal(none.verts, verts)

    # a forced short capacity: the same mesh through the retry
    real, calls = ops.marching_cubes_raw_batch, []

    def short(volumes, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1), max_verts=None, max_faces=None, **kw):
        calls.append((max_verts, max_faces))
        if max_verts is None:
            max_verts, max_faces = 1000, 1500
        return real(volumes, level, b_min, b_max, max_verts=max_verts, max_faces=max_faces, **kw)

    monkeypatch.setattr(ops, "marching_cubes_raw_batch", short)
    again = reconstruct_mesh(b["vol"], 0.5, BMIN, BMAX, netC=b["netC"], feat_tensor_C=b["feat_C"],
                             calib_tensor=b["calib"])
    monkeypatch.undo()
    assert calls == [(None, None), (verts.shape[0], faces.shape[0])]
    for got, want in zip(again, mesh):
        assert torch.equal(got, want)


def test_reconstruct_mesh_none_and_multi_view(ops, body257):
    from monoport_amd.recon import reconstruct_mesh
    assert reconstruct_mesh(None) is None
    with pytest.raises(ValueError):
        reconstruct_mesh(body257["vol"], normals="area")
    net2 = _seeded_netC(v_n=2)
    with pytest.raises(NotImplementedError, match="vertex_colors"):
        reconstruct_mesh(body257["vol"], 0.5, BMIN, BMAX, netC=net2, feat_tensor_C=body257["feat_C"],
                         calib_tensor=body257["calib"])


def test_perspective_netC_colours(ops, body257):
    """A perspective netC takes the counted launch with its projection mode, as recon.colorization does."""
    from monoport_amd import mesh_util
    from monoport_amd.modeling import geometry
    from monoport_amd.recon import reconstruct_mesh
    b = body257
    net = _seeded_netC()
    net.projection = geometry.perspective
    calib = torch.tensor([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 1.0, 3.0], [0, 0, 0, 1.0]], device=DEV)[None]
    mesh = reconstruct_mesh(b["vol"], 0.5, BMIN, BMAX, normals=None, netC=net, feat_tensor_C=b["feat_C"],
                            calib_tensor=calib)
    colors = mesh_util.vertex_colors(net, b["feat_C"], mesh.verts, calib)
    print("perspective colours: max |chain - vertex_colors| = %.3g" % float((mesh.colors - colors).abs().max()))
    assert torch.equal(mesh.colors, colors)
    assert not torch.equal(mesh.colors, mesh_util.vertex_colors(b["netC"], b["feat_C"], mesh.verts, b["calib"]))


def test_raw_chain_needs_no_host_value(ops, body257):
    """marching_cubes_raw -> mesh_normals_raw -> mesh_points_raw -> query_counted with `counts` never leaving the
    device equals the Python-level call."""
    from monoport_amd.recon import reconstruct_mesh
    b = body257
    mesh = reconstruct_mesh(b["vol"], 0.5, BMIN, BMAX, netC=b["netC"], feat_tensor_C=b["feat_C"],
                            calib_tensor=b["calib"])
    verts, faces, counts = ops.marching_cubes_raw(b["vol"], 0.5, BMIN, BMAX)
    normals = ops.mesh_normals_raw(verts, faces, counts, "accumulate")
    pts, count = ops.mesh_points_raw(verts, counts)
    binding = b["netC"].bind(b["feat_C"], b["calib"])
    preds = ops.query_counted(binding.mlp, binding.feat_hwc, pts, count, binding.calib, binding.z_scale)
    nv, nf = counts.cpu().tolist()  # the one host read, after everything is enqueued
    assert (nv, nf) == (mesh.verts.shape[0], mesh.faces.shape[0]) and int(count.item()) == nv
    assert torch.equal(verts[:nv], mesh.verts) and torch.equal(faces[:nf], mesh.faces)
    assert torch.equal(normals[:nv], mesh.normals)
    assert torch.equal((preds * 0.5 + 0.5).t()[:nv], mesh.colors)
    assert torch.equal(pts[:, :nv], mesh.verts.t()) and (pts[:, nv:] == 0).all()
