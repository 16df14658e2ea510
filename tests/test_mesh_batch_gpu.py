"""mp_marching_cubes_batch / mp_mesh_normals_batch / mp_mesh_points_batch (csrc/mcubes.hip, csrc/mesh.hip),
recon.reconstruct_mesh_many and FrameSlot(mesh=...) on the GPU.  The contract of every layer is the same: frame f of
a batched call equals the per-frame call on frame f's inputs bit for bit, truncation included, and touches nothing of
the other frames.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
SENTINEL = 12345.0
ISENTINEL = -777
MODES = ("reference", "accumulate")
MP_ERR_ARG = -1


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def vols33():
    """Unequal vertex / face counts, and one empty mesh."""
    return [torch.from_numpy(v).to(DEV) for v in (syn.blob_volume(33, 5), syn.sphere_volume(33), syn.blob_volume(33, 7),
                                                  np.zeros((33, 33, 33), np.float32))]


def _single(ops, vol, max_verts=None, max_faces=None):
    """The per-frame calls on one volume: the reference of everything below."""
    verts, faces, counts = ops.marching_cubes_raw(vol, 0.5, BMIN, BMAX, max_verts=max_verts, max_faces=max_faces)
    nrm = {m: ops.mesh_normals_raw(verts, faces, counts, m, out=torch.full_like(verts, SENTINEL)) for m in MODES}
    pts, count = ops.mesh_points_raw(verts, counts)
    nv, nf = counts.cpu().tolist()
    return dict(verts=verts, faces=faces, counts=counts, normals=nrm, points=pts, count=count,
                nv=min(nv, verts.shape[0]), nf=min(nf, faces.shape[0]), need=(nv, nf))


@pytest.fixture(scope="module")
def singles33(ops, vols33):
    return [_single(ops, v) for v in vols33]


def _sentinel_out(n, cap_v, cap_f, guard=1):
    """Sentinel-filled (verts, faces, counts) of n frames cut out of larger tensors, with the larger tensors: the
    frames are adjacent, so an overrun of frame f shows up in frame f + 1 (or in the guard frames)."""
    big = (torch.full((n + 2 * guard, cap_v, 3), SENTINEL, device=DEV),
           torch.full((n + 2 * guard, cap_f, 3), ISENTINEL, dtype=torch.int32, device=DEV),
           torch.full((n + 2 * guard, 2), ISENTINEL, dtype=torch.int32, device=DEV))
    return tuple(b[guard:guard + n] for b in big), big


def _bits(t):
    return t.view(torch.int32)


def _check_frame(ops, got, want, normals=None, points=None, what=""):
    """One frame of a batch against ``_single``: counts, the rows present, and the rows beyond them untouched."""
    verts, faces, counts = got
    nv, nf = want["nv"], want["nf"]
    assert counts.cpu().tolist() == list(want["need"]), what
    assert torch.equal(_bits(verts[:nv]), _bits(want["verts"][:nv])), what
    assert torch.equal(faces[:nf], want["faces"][:nf]), what
    assert (verts[nv:] == SENTINEL).all() and (faces[nf:] == ISENTINEL).all(), what
    for mode, nrm in (normals or {}).items():
        assert torch.equal(_bits(nrm[:nv]), _bits(want["normals"][mode][:nv])), (what, mode)
        assert (nrm[nv:] == SENTINEL).all(), (what, mode)
    if points is not None:
        pts, count = points
        assert int(count.item()) == int(want["count"].item()) == nv, what
        assert torch.equal(_bits(pts[:, :nv]), _bits(want["points"][:, :nv])), what
        assert (pts[:, nv:] == SENTINEL).all(), what


def _batch(ops, vols, cap_v, cap_f, gates=None):
    """The three batched calls into sentinel-filled buffers -> (per-frame raws, normals per mode, points, guards)."""
    n = len(vols)
    out, big = _sentinel_out(n, cap_v, cap_f)
    raws = ops.marching_cubes_raw_batch(vols, 0.5, BMIN, BMAX, gates=gates, out=out)
    verts, faces, counts = ([r[k] for r in raws] for k in range(3))
    nbig = {m: torch.full((n + 2, cap_v, 3), SENTINEL, device=DEV) for m in MODES}
    normals = {m: ops.mesh_normals_raw_batch(verts, faces, counts, m, out=nbig[m][1:n + 1]) for m in MODES}
    pbig = torch.full((n + 2, 3, cap_v), SENTINEL, device=DEV)
    cbig = torch.full((n + 2, 1), ISENTINEL, dtype=torch.int32, device=DEV)
    points = ops.mesh_points_raw_batch(verts, counts, out=(pbig[1:n + 1], cbig[1:n + 1]))
    guards = list(big) + list(nbig.values()) + [pbig, cbig]
    return raws, normals, points, guards


def _guards_untouched(guards):
    for g in guards:
        s = SENTINEL if g.dtype == torch.float32 else ISENTINEL
        assert (g[0] == s).all() and (g[-1] == s).all()


def test_per_frame_equality_at_33(ops, vols33, singles33):
    cap_v, cap_f = singles33[0]["verts"].shape[0], singles33[0]["faces"].shape[0]
    raws, normals, points, guards = _batch(ops, vols33, cap_v, cap_f)
    needs = [s["need"] for s in singles33]
    print("33^3 batch: (vertices, faces) per frame %s" % needs)
    assert len(set(needs)) == 4 and needs[3] == (0, 0) and all(n[0] > 0 for n in needs[:3])
    for f in range(4):
        _check_frame(ops, raws[f], singles33[f], {m: normals[m][f] for m in MODES}, points[f], "frame %d" % f)
    _guards_untouched(guards)
    gold = load_golden("mesh_normals")
    nv, nf = needs[0]
    assert np.array_equal(raws[0][0][:nv].cpu().numpy(), gold["blob33_verts"])
    assert np.array_equal(raws[0][1][:nf].cpu().numpy(), gold["blob33_faces"])
    # without caller's buffers: the default capacities, points beyond the counts start as zeros (mesh_points_raw)
    plain = ops.marching_cubes_raw_batch(vols33, 0.5, BMIN, BMAX)
    assert plain[0][0].shape == (cap_v, 3) and plain[0][1].shape == (cap_f, 3)
    pts = ops.mesh_points_raw_batch([p[0] for p in plain], [p[2] for p in plain])
    nrm = ops.mesh_normals_raw_batch([p[0] for p in plain], [p[1] for p in plain], [p[2] for p in plain])
    for f in range(4):
        nv = singles33[f]["nv"]
        assert torch.equal(plain[f][2], singles33[f]["counts"])
        assert torch.equal(pts[f][0][:, :nv], singles33[f]["points"][:, :nv]) and (pts[f][0][:, nv:] == 0).all()
        assert torch.equal(_bits(nrm[f][:nv]), _bits(singles33[f]["normals"]["accumulate"][:nv]))


def test_scan_carry_at_129(ops):
    """129^3 = 2,097 blocks of 1,024 nodes per frame: the scan's 1,024-block loop carries twice."""
    assert (129 ** 3 + 1023) // 1024 == 2097
    vols = [torch.from_numpy(v).to(DEV) for v in (syn.sphere_volume(129), syn.blob_volume(129, 3))]
    want = [_single(ops, v) for v in vols]
    cap_v, cap_f = want[0]["verts"].shape[0], want[0]["faces"].shape[0]
    raws, normals, points, guards = _batch(ops, vols, cap_v, cap_f)
    print("129^3 batch: (vertices, faces) per frame %s" % [w["need"] for w in want])
    assert all(0 < w["need"][0] < cap_v and 0 < w["need"][1] < cap_f for w in want)
    for f in range(2):
        _check_frame(ops, raws[f], want[f], {m: normals[m][f] for m in MODES}, points[f], "frame %d" % f)
    _guards_untouched(guards)


def test_gate(ops, vols33, singles33):
    """Frame 1 (a volume of noise: read, it would give thousands of vertices) has its gate at 0."""
    noise = torch.from_numpy(syn.rand_feat(33, 33, 33, 9)).to(DEV)
    vols = [vols33[0], noise, vols33[2]]
    want = [singles33[0], None, singles33[2]]
    cap_v, cap_f = singles33[0]["verts"].shape[0], singles33[0]["faces"].shape[0]
    assert ops.marching_cubes_raw(noise, 0.5, BMIN, BMAX)[2].cpu().tolist()[0] > 1000
    off = torch.zeros(1, dtype=torch.int32, device=DEV)
    on = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    for gates in ([on, off, on], [None, off, None]):  # a NULL entry of the gate array = frame on
        raws, normals, points, guards = _batch(ops, vols, cap_v, cap_f, gates=gates)
        verts, faces, counts = raws[1]
        assert counts.cpu().tolist() == [0, 0]
        assert (verts == SENTINEL).all() and (faces == ISENTINEL).all()
        assert all((normals[m][1] == SENTINEL).all() for m in MODES)
        assert int(points[1][1].item()) == 0 and (points[1][0] == SENTINEL).all()
        for f in (0, 2):
            _check_frame(ops, raws[f], want[f], {m: normals[m][f] for m in MODES}, points[f], "frame %d" % f)
        _guards_untouched(guards)
    # no gate array at all, and every gate open: the noise is meshed like any volume
    for gates in (None, [on, on, on]):
        raws = ops.marching_cubes_raw_batch(vols, 0.5, BMIN, BMAX, gates=gates)
        assert torch.equal(raws[1][2], ops.marching_cubes_raw(noise, 0.5, BMIN, BMAX)[2])


def test_truncation_and_isolation(ops, vols33, singles33):
    """30 vertices and 10 faces kept of thousands: counts report what is needed, only the capacities are written,
    the normals skip the faces that name a vertex beyond the capacity, and no frame writes into its neighbour."""
    want = [_single(ops, v, max_verts=30, max_faces=10) for v in vols33]
    raws, normals, points, guards = _batch(ops, vols33, 30, 10)
    for f in range(4):
        assert want[f]["need"] == singles33[f]["need"]
        assert (want[f]["nv"], want[f]["nf"]) == ((30, 10) if f < 3 else (0, 0))
        _check_frame(ops, raws[f], want[f], {m: normals[m][f] for m in MODES}, points[f], "frame %d" % f)
    _guards_untouched(guards)
    # the empty frame sits behind a truncated one: all of its rows still hold the sentinel (checked above per row
    # range); the same with the empty frame in the middle
    order = [0, 3, 1]
    raws, normals, points, guards = _batch(ops, [vols33[i] for i in order], 30, 10)
    for f, i in enumerate(order):
        _check_frame(ops, raws[f], want[i], {m: normals[m][f] for m in MODES}, points[f], "frame %d" % f)
    _guards_untouched(guards)


def test_chunking_and_frame_count_limits(ops, vols33, singles33):
    cap_v, cap_f = singles33[0]["verts"].shape[0], singles33[0]["faces"].shape[0]
    raws, normals, points, guards = _batch(ops, vols33[:1], cap_v, cap_f)
    _check_frame(ops, raws[0], singles33[0], {m: normals[m][0] for m in MODES}, points[0], "n = 1")
    _guards_untouched(guards)
    n = ops.MAX_FRAMES + 1  # 33 frames: two calls per stage
    raws, normals, points, guards = _batch(ops, [vols33[f % 4] for f in range(n)], cap_v, cap_f)
    for f in range(n):
        _check_frame(ops, raws[f], singles33[f % 4], {m: normals[m][f] for m in MODES}, points[f], "frame %d" % f)
    _guards_untouched(guards)
    # the raw binding: 0 and mp_max_frames() + 1 frames are refused with a message
    ctx = ops.get_context(torch.device(DEV))
    lib, st = ctx.lib, ops._stream(vols33[0])
    assert lib.mp_max_frames() == ops.MAX_FRAMES
    verts, faces, counts = ([r[k] for r in raws] for k in range(3))
    vols = [vols33[f % 4] for f in range(n)]
    outs = [normals["accumulate"][f] for f in range(n)]
    pts, cnt = [p[0] for p in points], [p[1] for p in points]
    before = counts[0].clone()
    for bad in (0, n):
        calls = {
            "mp_marching_cubes_batch": lambda: lib.mp_marching_cubes_batch(
                ctx.handle, bad, ops._ptr_array(vols), 33, 0.5, ops._float3(BMIN), ops._float3(BMAX),
                ops._ptr_array(verts), cap_v, ops._ptr_array(faces), cap_f, ops._ptr_array(counts), None, st),
            "mp_mesh_normals_batch": lambda: lib.mp_mesh_normals_batch(
                ctx.handle, bad, ops._ptr_array(verts), cap_v, ops._ptr_array(faces), cap_f, ops._ptr_array(counts), 1,
                ops._ptr_array(outs), st),
            "mp_mesh_points_batch": lambda: lib.mp_mesh_points_batch(
                ctx.handle, bad, ops._ptr_array(verts), cap_v, ops._ptr_array(counts), ops._ptr_array(pts),
                ops._ptr_array(cnt), st)}
        for name, call in calls.items():
            assert call() == MP_ERR_ARG, (name, bad)
            msg = lib.mp_last_error(ctx.handle).decode()
            assert name in msg and "1..%d frames" % ops.MAX_FRAMES in msg and str(bad) in msg, msg
    # the other refusals of the per-mesh calls: a null buffer of one frame, a bad mode, capacities beyond 2^31 / 3
    holes = list(verts[:2])
    holes[1] = None
    assert lib.mp_mesh_normals_batch(ctx.handle, 2, ops._ptr_array(holes), cap_v, ops._ptr_array(faces[:2]), cap_f,
                                     ops._ptr_array(counts[:2]), 1, ops._ptr_array(outs[:2]), st) == MP_ERR_ARG
    assert "frame 1" in lib.mp_last_error(ctx.handle).decode()
    assert lib.mp_mesh_normals_batch(ctx.handle, 2, ops._ptr_array(verts[:2]), cap_v, ops._ptr_array(faces[:2]), cap_f,
                                     ops._ptr_array(counts[:2]), 7, ops._ptr_array(outs[:2]), st) == MP_ERR_ARG
    assert lib.mp_mesh_normals_batch(ctx.handle, 2, ops._ptr_array(verts[:2]), 2 ** 31 // 3 + 1,
                                     ops._ptr_array(faces[:2]), cap_f, ops._ptr_array(counts[:2]), 1,
                                     ops._ptr_array(outs[:2]), st) == -3  # MP_ERR_UNSUPPORTED
    assert "2^31 / 3" in lib.mp_last_error(ctx.handle).decode()
    odd = (ctypes.c_void_p * 2)(verts[0].data_ptr() + 2, verts[1].data_ptr())
    assert lib.mp_mesh_points_batch(ctx.handle, 2, odd, cap_v, ops._ptr_array(counts[:2]), ops._ptr_array(pts[:2]),
                                    ops._ptr_array(cnt[:2]), st) == MP_ERR_ARG
    assert "misaligned" in lib.mp_last_error(ctx.handle).decode()
    torch.cuda.synchronize()
    assert torch.equal(counts[0], before)  # a refused call enqueues nothing


def test_accumulate_mode_is_the_same_bits_on_a_second_run(ops, vols33):
    raws = ops.marching_cubes_raw_batch(vols33, 0.5, BMIN, BMAX)
    verts, faces, counts = ([r[k] for r in raws] for k in range(3))
    out_a = torch.full((4,) + tuple(verts[0].shape), SENTINEL, device=DEV)
    out_b = torch.full((4,) + tuple(verts[0].shape), SENTINEL, device=DEV)
    ops.mesh_normals_raw_batch(verts, faces, counts, "accumulate", out=out_a)
    ops.mesh_normals_raw_batch(verts, faces, counts, "accumulate", out=out_b)
    assert torch.equal(_bits(out_a), _bits(out_b))
    assert (out_a != SENTINEL).any()


# ---- recon.reconstruct_mesh_many --------------------------------------------------------------------------------

def _seeded_netC():
    from monoport_amd.modeling import PIFuNetC
    netC = PIFuNetC()
    with torch.no_grad():
        for i, (w, b) in enumerate(syn.rand_mlp("C", 61, 2.0)):
            netC.surface_classifier.filters[i].weight.copy_(torch.from_numpy(w)[:, :, None])
            netC.surface_classifier.filters[i].bias.copy_(torch.from_numpy(b))
    netC.surface_classifier.to(DEV)
    return netC.eval()


@pytest.fixture(scope="module")
def colour():
    feat_C = [[torch.from_numpy(syn.rand_feat(512, 128, 128, 62))[None].to(DEV)]]
    return dict(netC=_seeded_netC(), feat_C=feat_C)


def _same_mesh(got, want, what=""):
    from monoport_amd.recon import Mesh
    assert isinstance(got, Mesh) and isinstance(want, Mesh), what
    for name, a, b in zip(Mesh._fields, got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() == b.is_contiguous(), (what, name)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, name)


@pytest.mark.parametrize("projection", ["orthogonal", "perspective"])
def test_reconstruct_mesh_many(ops, vols33, colour, projection, monkeypatch):
    from monoport_amd.modeling import geometry
    from monoport_amd.recon import reconstruct_mesh, reconstruct_mesh_many
    net = colour["netC"] if projection == "orthogonal" else _seeded_netC()
    if projection == "perspective":
        net.projection = geometry.perspective
        calibs = [torch.tensor([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 1.0, 3.0], [0, 0, 0, 1.0]], device=DEV)[None],
                  None,
                  torch.tensor([[1.5, 0, 0, 0.1], [0, 1.5, 0, 0], [0, 0, 1.0, 2.5], [0, 0, 0, 1.0]], device=DEV)[None]]
    else:  # every frame its own camera
        calibs = [torch.eye(4, device=DEV)[None], None, (torch.eye(4, device=DEV) * 0.9)[None].contiguous()]
    sdfs = [vols33[0][None, None], None, vols33[1]]
    feats = [colour["feat_C"], None, colour["feat_C"]]
    want = [None if s is None else reconstruct_mesh(s, 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feats[i],
                                                    calib_tensor=calibs[i]) for i, s in enumerate(sdfs)]
    got = reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, netC=net, feat_tensors_C=feats, calib_tensors=calibs)
    assert len(got) == 3 and got[1] is None
    for i in (0, 2):
        _same_mesh(got[i], want[i], "frame %d" % i)
        assert got[i].colors.shape == got[i].verts.shape and got[i].verts.shape[0] > 100
    assert not torch.equal(got[0].colors, reconstruct_mesh(sdfs[0], 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feats[0],
                                                           calib_tensor=calibs[2]).colors)  # the cameras matter
    # the other normals settings, no colours
    for normals in ("reference", None):
        got_n = reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, normals=normals)
        for i in (0, 2):
            _same_mesh(got_n[i], reconstruct_mesh(sdfs[i], 0.5, BMIN, BMAX, normals=normals), "normals=%s" % normals)
    # a capacity guess of 100 vertices: every frame is re-run alone with exact capacities
    real, calls = ops.marching_cubes_raw_batch, []

    def short(volumes, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1), max_verts=None, max_faces=None, **kw):
        calls.append(max_verts)
        return real(volumes, level, b_min, b_max, max_verts=100 if max_verts is None else max_verts,
                    max_faces=max_faces, **kw)

    monkeypatch.setattr(ops, "marching_cubes_raw_batch", short)
    again = reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, netC=net, feat_tensors_C=feats, calib_tensors=calibs)
    monkeypatch.undo()
    # one call for all volumes at the default guess, then each live volume alone at what it needs
    assert calls == [None, want[0].verts.shape[0], want[2].verts.shape[0]] and again[1] is None
    for i in (0, 2):
        _same_mesh(again[i], want[i], "re-run, frame %d" % i)


def _body_floater():
    """A sphere of radius 0.5 about the origin and a small blob at (0.75, 0.75, 0.75)."""
    g = ((np.arange(33) + 0.5) / 33) * 2 - 1
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    body = np.sqrt(x * x + y * y + z * z) < 0.5
    blob = np.sqrt((x - 0.75) ** 2 + (y - 0.75) ** 2 + (z - 0.75) ** 2) < 0.12
    return np.where(body | blob, 0.9, 0.1).astype(np.float32)


THREE = dict(iterations=3, lam=0.5, mu=-0.53, pin_border=True)


def _by_hand(ops, vol, binding, clean=None, simplify=None, smooth=None):
    """reconstruct_mesh(vol, normals="accumulate", netC=...) composed from the raw per-frame calls -> (Mesh, the
    capacity-sized vertices before and after smoothing, marching cubes' counts).  An orthogonal binding is queried by
    the per-frame counted call, a perspective one by the batched call of one frame."""
    from monoport_amd.recon import Mesh
    if clean is not None:
        vol = ops.keep_largest_raw(vol, 0.5, clean, 0.0)[0]
    verts, faces, counts = ops.marching_cubes_raw(vol, 0.5, BMIN, BMAX)
    mc_counts = counts
    if simplify is not None:
        verts, faces, counts, _ = ops.mesh_simplify_raw(verts, faces, counts, simplify, BMIN, BMAX)
    moved = verts if smooth is None else ops.mesh_smooth_raw(verts, faces, counts, **smooth)
    nrm = ops.mesh_normals_raw(moved, faces, counts, "accumulate")
    pts, count = ops.mesh_points_raw(verts, counts)
    if binding.projection == ops.PROJECTIONS["orthogonal"]:
        col = ops.query_counted(binding.mlp, binding.feat_hwc, pts, count, binding.calib, binding.z_scale)
    else:
        col = ops.query_counted_batch(binding.mlp, [binding.feat_hwc], [pts], [count], [binding.calib], binding.z_scale,
                                      projections=[binding.projection])[0]
    nv, nf = counts.cpu().tolist()
    mesh = Mesh(moved[:nv], faces[:nf], nrm[:nv], (col * 0.5 + 0.5).t()[:nv].contiguous())
    return mesh, verts, moved, mc_counts.cpu().tolist()


def _count_queries(ops, monkeypatch):
    """-> the list that every counted colour query from now on appends its kind to."""
    kinds = []
    for kind in ("query_counted", "query_counted_batch"):
        def counted(*args, _real=getattr(ops, kind), _kind=kind, **kw):
            kinds.append(_kind)
            return _real(*args, **kw)

        monkeypatch.setattr(ops, kind, counted)
    return kinds


def _short_guess(ops, monkeypatch):
    """Marching cubes with a capacity guess of 100 vertices / 150 faces where the caller names none."""
    real = ops.marching_cubes_raw_batch
    monkeypatch.setattr(ops, "marching_cubes_raw_batch",
                        lambda s, level, lo, hi, max_verts=None, max_faces=None, **kw: real(
                            s, level, lo, hi, max_verts=max_verts or 100, max_faces=max_faces or 150, **kw))


def test_every_option_at_once(ops, colour):
    """clean, simplify, smooth, normals and colours in one chain: the only combination nothing else composes."""
    from monoport_amd import recon
    net, feat = colour["netC"], colour["feat_C"]
    calib = torch.eye(4, device=DEV)[None]
    vol = torch.from_numpy(_body_floater()).to(DEV)
    zeros = torch.zeros((33, 33, 33), device=DEV)
    before = vol.clone()
    binding = recon._bind_netC("test", net, [(feat, calib, vol.device)])[0]
    want, on_surface, moved, mc_counts = _by_hand(ops, vol, binding, clean=6, simplify=16, smooth=THREE)
    nv = want.verts.shape[0]
    print("33^3 body + floater, every option: %s from marching cubes, %d vertices kept" % (mc_counts, nv))
    # every stage did something: the floater is gone, the clustering shrank the mesh, the smoothing moved it
    assert 50 < nv < mc_counts[0] and float(want.verts.abs().max()) < 0.6
    assert mc_counts[0] < ops.marching_cubes_raw(vol, 0.5, BMIN, BMAX)[2][0].item()
    assert not torch.equal(moved[:nv], on_surface[:nv])
    opts = dict(normals="accumulate", clean=6, simplify=16, smooth=3)
    got = recon.reconstruct_mesh(vol[None, None], 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feat, calib_tensor=calib,
                                 **opts)
    _same_mesh(got, want, "reconstruct_mesh")
    many = recon.reconstruct_mesh_many([vol, None, zeros], 0.5, BMIN, BMAX, netC=net, feat_tensors_C=[feat, None, feat],
                                       calib_tensors=[calib, None, calib], **opts)
    assert len(many) == 3 and many[1] is None
    _same_mesh(many[0], want, "reconstruct_mesh_many, frame 0")
    _same_mesh(many[2], _by_hand(ops, zeros, binding, clean=6, simplify=16, smooth=THREE)[0], "frame 2")
    assert many[2].verts.shape == (0, 3) and many[2].faces.shape == (0, 3) and many[2].colors.shape == (0, 3)
    assert torch.equal(vol, before)


@pytest.mark.parametrize("simplify", [None, 16])
def test_one_live_volume_in_a_list(ops, vols33, colour, simplify, monkeypatch):
    """reconstruct_mesh_many is defined against reconstruct_mesh: with one live orthogonal volume it issues that
    call's per-frame counted query, on the first run and on the re-run with exact capacities alike."""
    from monoport_amd import recon
    net, feat = colour["netC"], colour["feat_C"]
    calib = (torch.eye(4, device=DEV) * 0.9)[None].contiguous()
    vol = vols33[0]
    want = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feat, calib_tensor=calib,
                                  simplify=simplify)
    assert want.verts.shape[0] == (1562 if simplify is None else 285) and want.colors.shape == want.verts.shape
    kinds = _count_queries(ops, monkeypatch)
    kw = dict(netC=net, feat_tensors_C=[None, feat], calib_tensors=[None, calib], simplify=simplify)
    got = recon.reconstruct_mesh_many([None, vol], 0.5, BMIN, BMAX, **kw)
    assert got[0] is None and kinds == ["query_counted"]
    _same_mesh(got[1], want, "one live volume")
    _short_guess(ops, monkeypatch)
    again = recon.reconstruct_mesh_many([None, vol], 0.5, BMIN, BMAX, **kw)
    assert again[0] is None and kinds == ["query_counted"] * 3
    _same_mesh(again[1], want, "one live volume, re-run")


def test_perspective_binding_on_one_volume(ops, vols33, colour, monkeypatch):
    """The other side of the rule: one frame under a perspective camera goes through the batched counted query."""
    from monoport_amd import recon
    from monoport_amd.modeling import geometry
    net = _seeded_netC()
    net.projection = geometry.perspective
    feat = colour["feat_C"]
    calib = torch.tensor([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 1.0, 3.0], [0, 0, 0, 1.0]], device=DEV)[None]
    vol = vols33[0]
    binding = recon._bind_netC("test", net, [(feat, calib, vol.device)])[0]
    assert binding.projection == ops.PROJECTIONS["perspective"]
    want = _by_hand(ops, vol, binding)[0]
    kinds = _count_queries(ops, monkeypatch)
    got = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feat, calib_tensor=calib)
    assert kinds == ["query_counted_batch"]
    _same_mesh(got, want, "perspective")
    ortho = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, netC=colour["netC"], feat_tensor_C=feat, calib_tensor=calib)
    assert kinds == ["query_counted_batch", "query_counted"]
    assert torch.equal(got.verts, ortho.verts) and not torch.equal(got.colors, ortho.colors)  # the projection matters


def test_reconstruct_mesh_many_multi_view_head(colour):
    from monoport_amd.modeling import PIFuNetC, heads
    from monoport_amd.recon import reconstruct_mesh_many
    net2 = PIFuNetC()
    net2.surface_classifier = heads.SurfaceClassifier(heads.PIFuNetCMLP().filter_channels, 2, False, "tanh")
    with pytest.raises(NotImplementedError, match="vertex_colors"):
        reconstruct_mesh_many([None], netC=net2.eval(), feat_tensors_C=[None], calib_tensors=[None])


# ---- FrameSlot(mesh=...) ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    import bench
    dev = torch.device(DEV)
    return bench.build_netg(dev)[0], bench.build_netc(dev)


def _body_hook():
    """bench.make_pipeline's synthetic-data hook: channels 0 / 1 of netG's map are the body's depth planes."""
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(DEV)
    planes_hwc = planes.permute(1, 2, 0).contiguous()

    def hook(feat):
        feat[:, 0:2].copy_(planes[None].expand(feat.shape[0], -1, -1, -1))

    def hook_hwc(feat_hwc):
        feat_hwc[..., 0:2].copy_(planes_hwc[None].expand(feat_hwc.shape[0], -1, -1, -1))

    hook.hwc = hook_hwc
    return hook


def _slot(nets, batch, resolutions, **kw):
    from monoport_amd.pipeline import FrameSlot
    netg, netc = nets
    return FrameSlot(netg, torch.device(DEV), netC=netc, batch=batch, resolutions=resolutions, b_min=BMIN, b_max=BMAX,
                     feature_hook=_body_hook(), **kw)


def _vertices_equal(a, b):
    ca, cb = int(a[4].item()), int(b[4].item())
    return ca == cb and all(torch.equal(a[k][:ca], b[k][:cb]) for k in range(4))


def test_slot_meshes(nets):
    """Frame 0: a synthetic body.  Frame 1: a camera that looks past the box (every query point projects outside the
    image, so netG answers exactly 0 everywhere): its coarsest level is empty and its volume unspecified."""
    from monoport_amd.modeling.MonoPortNet import QueryBinding
    from monoport_amd.recon import Mesh, _finish_mesh, _mesh_chains, mesh_options, pifu_calib
    images = torch.stack([torch.from_numpy(syn.synthetic_image(0)), torch.zeros(3, 512, 512)]).to(DEV)
    away = torch.eye(4, device=DEV)[None]
    away[0, 0, 3] = 5.0
    calibs = [pifu_calib(*syn.scene_camera(0), device=DEV), away]
    slot = _slot(nets, 2, (17, 33, 65), mesh={"normals": "accumulate"})
    plain = _slot(nets, 2, (17, 33, 65))
    try:
        assert tuple(slot.mesh[:3]) == ("accumulate", 0.5, True) and plain.mesh is None and not hasattr(plain, "mesh_buffers")
        with pytest.raises(RuntimeError):
            plain.meshes()
        slot.submit(images, calibs)
        slot.wait()
        status = slot.status.cpu()
        assert status[0, 0].item() == 1 and status[1, 0].item() == 0  # the precondition, from the slot's own status
        meshes = slot.meshes()
        assert len(meshes) == 2 and isinstance(meshes[0], Mesh) and meshes[1] is None
        m = meshes[0]
        print("slot mesh at 65^3: %d vertices, %d faces" % (m.verts.shape[0], m.faces.shape[0]))
        assert m.verts.shape[0] > 500 and m.verts.data_ptr() == slot.mesh_buffers["verts"].data_ptr()
        assert slot.mesh_buffers["counts"][1].cpu().tolist() == [0, 0]
        binding = QueryBinding(nets[1], nets[1].surface_classifier.packed(), slot.feats_hwc_c[0], slot.calib[0:1],
                               syn.Z_SCALE)
        chain = _mesh_chains([slot.volumes[0]], BMIN, BMAX, mesh_options("accumulate", 0.5, True), [binding])[0]
        nv, nf = chain.counts.cpu().tolist()
        _same_mesh(m, _finish_mesh(chain, nv, nf), "slot frame 0")
        assert float(m.colors.min()) >= 0 and float(m.colors.max()) <= 1 and not (m.normals == 0).all()
        first = Mesh(*[t.clone() for t in m])
        # the same submission on a slot without mesh output
        plain.submit(images, calibs)
        plain.wait()
        assert torch.equal(plain.status, slot.status)
        assert torch.equal(plain.volumes[0], slot.volumes[0])
        # (frame 1's volume is unspecified, and with it everything made from it)
        assert torch.equal(plain.renders[0], slot.renders[0]) and torch.equal(plain.renders_tex[0], slot.renders_tex[0])
        assert _vertices_equal(plain.vertices[0], slot.vertices[0])
        # a second submission reproduces the first
        slot.submit(images, calibs)
        again = slot.meshes()  # waits itself
        assert again[1] is None
        _same_mesh(again[0], first, "second submit")
        # a short submission: one frame
        slot.submit(images[:1], calibs[:1])
        short = slot.meshes()
        assert len(short) == 1
        _same_mesh(short[0], first, "short submit")
    finally:
        slot.close()
        plain.close()


@pytest.mark.parametrize("normals,colors,mesh_batch", [("accumulate", True, None), ("accumulate", True, 2),
                                                       ("reference", False, 1), (None, False, 4)])
def test_slot_mesh_chain_chunks(ops, nets, vols33, singles33, normals, colors, mesh_batch, monkeypatch):
    """Five frames with MONOPORT_MESH_BATCH at its default and at 1, 2 and 4 frames per set of launches (chunks of
    2 + 2 + 1 and 4 + 1), the slot's volumes filled in by hand (four meshes of
    unequal size and an empty one; frame 2 switched off by its status): the slot's chunked chain = the per-frame
    chain; and a frame that overflows the slot's capacity is re-run alone."""
    from monoport_amd import pipeline
    from monoport_amd.modeling.MonoPortNet import QueryBinding
    from monoport_amd.recon import Mesh, _finish_mesh, _mesh_chains, mesh_options
    if mesh_batch is not None:
        monkeypatch.setattr(pipeline, "MESH_BATCH", mesh_batch)
    slot = _slot(nets, 5, (17, 33), mesh={"normals": normals, "colors": colors, "level": 0.5})
    try:
        order = [0, 1, 2, 3, 2]
        with torch.cuda.stream(slot.stream):
            for b, i in enumerate(order):
                slot.volumes[b].copy_(vols33[i])
                slot.feats_hwc_c[b].copy_(torch.from_numpy(syn.rand_feat(128, 128 * 512, 1, 70 + b)).to(DEV).view(128, 128, 512))
            slot.status.zero_()
            slot.status[:, 0] = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32)
            slot.calib[1] *= 0.9
            slot.n_active = 5
            slot._mesh_chain(5)
        slot._busy = True
        got = slot.meshes()
        assert [g is None for g in got] == [False, False, True, False, False]
        mlp_c = nets[1].surface_classifier.packed()
        for b, i in enumerate(order):
            if got[b] is None:
                continue
            binding = QueryBinding(nets[1], mlp_c, slot.feats_hwc_c[b], slot.calib[b:b + 1], syn.Z_SCALE) if colors else None
            chain = _mesh_chains([slot.volumes[b]], BMIN, BMAX, mesh_options(normals, 0.5, colors),
                                 [binding] if colors else None)[0]
            nv, nf = chain.counts.cpu().tolist()
            assert (nv, nf) == singles33[i]["need"]
            _same_mesh(got[b], _finish_mesh(chain, nv, nf), "frame %d" % b)
        assert got[3].verts.shape == (0, 3) and got[3].faces.shape == (0, 3)
        if colors:
            assert not torch.equal(got[0].colors[:50], got[1].colors[:50])
        # the slot's capacity cut to 100 vertices / 200 faces: every non-empty frame comes from the re-run (the meshes
        # above are views of the slot's buffers, which the next chain overwrites: keep copies)
        got = [g if g is None else Mesh(*[t if t is None else t.clone() for t in g]) for g in got]
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        if colors:
            slot.mesh_buffers["points"] = torch.zeros((5, 3, 100), device=DEV)
            slot.mesh_buffers["preds"] = torch.zeros((5, 3, 100), device=DEV)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(5)
        slot._busy = True
        again = slot.meshes()
        for b in range(5):
            if got[b] is None:
                assert again[b] is None
            else:
                _same_mesh(again[b], got[b], "re-run, frame %d" % b)
    finally:
        slot.close()
    print("MESH_BATCH = %d" % pipeline.MESH_BATCH)
