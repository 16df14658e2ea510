"""mp_mesh_smooth / mp_mesh_smooth_batch (csrc/smooth.hip) through ctypes, ops.mesh_smooth_raw[_batch],
recon.smooth_mesh and the ``smooth`` option of recon.reconstruct_mesh, recon.reconstruct_mesh_many and
FrameSlot(mesh=...), on the GPU.  The kernels are held to the definition's numpy restatement (tests/mesh_smooth_ref.py,
itself held to a loop implementation in tests/test_mesh_smooth_ref_cpu.py): verts_out bit for bit (as uint32) wherever
the restatement is not NaN and NaN for NaN elsewhere (the sign of a NaN that an operation produces differs between the
host and the GPU), ring exactly, rows beyond the counts untouched.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import mesh_smooth_ref as sm
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED = 0, -1, -3
PIN = 1  # MP_SMOOTH_PIN_BORDER
LAM, MU = 0.5, -0.53
POISON = -12345.0
IPOISON = -777


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def abi(ops):
    """(library, context handle, stream) of the C-ABI."""
    ctx = ops.get_context(torch.device(DEV))
    return ctx.lib, ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _pp(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _mesh_on_device(verts, faces, counts=None):
    """numpy (verts, faces) -> device (verts, faces, counts = their sizes unless given)."""
    v = torch.from_numpy(np.array(verts, np.float32).reshape(-1, 3)).to(DEV)  # a copy: the fixtures are read-only
    f = torch.from_numpy(np.array(faces, np.int32).reshape(-1, 3)).to(DEV)
    c = torch.tensor([v.shape[0], f.shape[0]] if counts is None else counts, dtype=torch.int32, device=DEV)
    return v, f, c


def _outs(max_v, ring=True):
    return (torch.full((max_v, 3), POISON, device=DEV),
            torch.full((max_v,), IPOISON, dtype=torch.int32, device=DEV) if ring else None)


def _single(abi, mesh, iterations, flags=PIN, lam=LAM, mu=MU, ring=True, max_v=None, max_f=None):
    """One mp_mesh_smooth call into poisoned buffers -> (verts_out, ring)."""
    lib, h, st = abi
    v, f, c = mesh
    max_v = v.shape[0] if max_v is None else max_v
    max_f = f.shape[0] if max_f is None else max_f
    outs = _outs(max_v, ring)
    rc = lib.mp_mesh_smooth(h, _p(v), max_v, _p(f) if max_f else None, max_f, _p(c), iterations, lam, mu, flags,
                            _p(outs[0]), _p(outs[1]), st)
    assert rc == MP_OK, lib.mp_last_error(h).decode()
    return outs


def _check(outs, mesh, iterations, flags=PIN, lam=LAM, mu=MU, what="", want=None):
    """The outputs of a call against the restatement on the rows of ``mesh`` that the call may read -> the
    restatement's (verts, ring), to be handed in again as ``want`` where the same result is expected."""
    v, f, c = mesh
    vo, ro = outs
    nv, nf = (max(0, min(int(x), cap)) for x, cap in zip(c.cpu().tolist(), (vo.shape[0], f.shape[0])))
    if want is None:
        hv, hf = v[:nv].cpu().numpy(), f[:nf].cpu().numpy()
        want = sm.smooth_ref(hv, hf, iterations, lam, mu, bool(flags & PIN)), sm.ring_ref(hv, hf)
    assert want[0].shape == (nv, 3)
    assert sm.same_bits(vo[:nv].cpu().numpy(), want[0]), what
    assert (vo[nv:] == POISON).all(), what
    if ro is not None:
        assert np.array_equal(ro[:nv].cpu().numpy(), want[1]) and (ro[nv:] == IPOISON).all(), what
    return want


@pytest.fixture(scope="module")
def device_meshes(ops):
    """The device's own marching-cubes meshes at the capacities of ops.marching_cubes_raw (counts below them)."""
    vols = {"blob33_5": syn.blob_volume(33, 5), "blob17_3": syn.blob_volume(17, 3)}
    return {k: ops.marching_cubes_raw(torch.from_numpy(v).to(DEV), 0.5, BMIN, BMAX) for k, v in vols.items()}


@pytest.mark.parametrize("name", ["blob33_5", "blob17_3"])
def test_device_meshes_against_the_definition(abi, device_meshes, name):
    """Several blocks of vertices and faces (1,562 and 3,124 at 33^3), capacities above the counts, one to 128 passes.
    A closed mesh has no border vertex: both flag values give the same bits."""
    mesh = device_meshes[name]
    before = [t.clone() for t in mesh]
    for iterations in (1, 2, 10, 64):
        want = _check(_single(abi, mesh, iterations, PIN), mesh, iterations, PIN, what="%s x %d" % (name, iterations))
        _check(_single(abi, mesh, iterations, 0), mesh, iterations, 0, what="%s x %d, free" % (name, iterations),
               want=want)
        assert (want[1] >= 3).all() and np.isfinite(want[0]).all()
    assert all(torch.equal(a, b) for a, b in zip(mesh, before))  # the inputs are only read
    if name == "blob33_5":
        assert mesh[2].cpu().tolist() == [1562, 3124]
        gold_v, gold_f = sm.oracle_mesh("blob33_5")  # the device's mesh is the oracle's
        assert np.array_equal(_bits(mesh[0][:1562]), gold_v.view(np.uint32))
        assert np.array_equal(mesh[1][:3124].cpu().numpy(), gold_f)


@pytest.mark.parametrize("flags", [PIN, 0])
def test_open_mesh(abi, flags):
    v, f = sm.open_mesh()
    mesh = _mesh_on_device(v, f)
    outs = _single(abi, mesh, 3, flags)
    want_v, ring = _check(outs, mesh, 3, flags, what="open mesh, flags %d" % flags)
    border = ring < 0
    assert border.sum() == 227
    moved = (_bits(outs[0]) != v.view(np.uint32)).any(1)
    assert moved[~border].all() and (not moved[border].any() if flags else moved[border].all())


@pytest.mark.parametrize("flags", [PIN, 0])
def test_soup(abi, flags):
    """Degenerate faces, unreferenced vertices, a fan of 200 faces, coordinates whose sums overflow."""
    v, f = sm.soup()
    mesh = _mesh_on_device(v, f)
    for iterations in (1, 2):
        want_v, ring = _check(_single(abi, mesh, iterations, flags), mesh, iterations, flags, what="soup")
    assert (ring == 0).sum() >= 4 and np.abs(ring).max() >= 200
    assert np.array_equal(_bits(mesh[0]), v.view(np.uint32)) and np.array_equal(mesh[1].cpu().numpy(), f)  # only read


def test_repeatable_under_contention(abi):
    """2,000 faces on one edge (every face writes into the segments of vertices 0 and 1), twice: the same bits, and
    the definition's."""
    v, f = sm.book(2000)
    mesh = _mesh_on_device(v, f)
    first, second = _single(abi, mesh, 2, 0), _single(abi, mesh, 2, 0)
    want_v, ring = _check(first, mesh, 2, 0, what="book")
    assert ring[0] == ring[1] == -2001 and (ring[2:] == -2).all()
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(first, second))
    pinned = _single(abi, mesh, 2, PIN)  # every vertex lies on an open edge
    assert np.array_equal(_bits(pinned[0]), v.view(np.uint32))


def test_zero_factors_return_the_input_bits(abi, device_meshes):
    mesh = device_meshes["blob33_5"]
    nv = int(mesh[2][0])
    outs = _single(abi, mesh, 5, PIN, 0.0, 0.0)
    assert np.array_equal(_bits(outs[0][:nv]), _bits(mesh[0][:nv])) and (outs[0][nv:] == POISON).all()
    _check(outs, mesh, 5, PIN, 0.0, 0.0, what="zero factors")


def test_counts_and_capacities(abi, device_meshes):
    v, f, c = device_meshes["blob33_5"]
    nv, nf = c.cpu().tolist()
    # the counts exceed the capacities: only the capacities are read, a face that names a vertex beyond them is no
    # face, and the hole it leaves has a border
    for flags in (PIN, 0):
        outs = _single(abi, (v, f, c), 3, flags, max_v=nv - 30, max_f=nf - 10)
        short = (v[:nv - 30], f[:nf - 10], c)
        want = _check(outs, short, 3, flags, what="short capacities")
        assert (want[1] < 0).any() and want[0].shape == (nv - 30, 3)
    # no mesh (a gated-off frame), and counts below zero: nothing is touched
    for counts in ([0, 0], [-5, -7]):
        outs = _single(abi, (v, f, torch.tensor(counts, dtype=torch.int32, device=DEV)), 3)
        assert (outs[0] == POISON).all() and (outs[1] == IPOISON).all()
    # vertices without faces: all fixed
    outs = _single(abi, (v, f, torch.tensor([nv, 0], dtype=torch.int32, device=DEV)), 3)
    assert np.array_equal(_bits(outs[0][:nv]), _bits(v[:nv])) and (outs[1][:nv] == 0).all()
    # without a ring: the same vertices
    a, b = _single(abi, (v, f, c), 3, ring=False), _single(abi, (v, f, c), 3)
    assert a[1] is None and np.array_equal(_bits(a[0]), _bits(b[0]))
    # a capacity of 0 faces: NULL rows, the vertices are copied; a capacity of 0 vertices: MP_OK, no buffer needed
    outs = _single(abi, (v, f, c), 3, max_f=0)
    assert np.array_equal(_bits(outs[0][:nv]), _bits(v[:nv])) and (outs[0][nv:] == POISON).all()
    lib, h, st = abi
    assert lib.mp_mesh_smooth(h, None, 0, None, 0, _p(c), 3, LAM, MU, PIN, None, None, st) == MP_OK
    assert lib.mp_mesh_smooth(h, None, 0, _p(f), f.shape[0], _p(c), 3, LAM, MU, PIN, None, None, st) == MP_OK


def _batch(abi, meshes, iterations=3, lam=LAM, mu=MU, flags=PIN, n_frames=None, max_v=None, max_f=None, outs=None,
           ring=True):
    lib, h, st = abi
    max_v = meshes[0][0].shape[0] if max_v is None else max_v
    max_f = meshes[0][1].shape[0] if max_f is None else max_f
    if outs is None:
        outs = [_outs(meshes[0][0].shape[0]) for _ in meshes]
    rc = lib.mp_mesh_smooth_batch(h, len(meshes) if n_frames is None else n_frames, _pp([m[0] for m in meshes]), max_v,
                                  _pp([m[1] for m in meshes]), max_f, _pp([m[2] for m in meshes]), iterations, lam, mu,
                                  flags, _pp([o[0] for o in outs]), _pp([o[1] for o in outs]) if ring else None, st)
    return rc, outs, lib.mp_last_error(h).decode()


def test_batch_equals_single_calls(abi, ops):
    """Unequal meshes of one capacity, one of them switched off, in one call; then 33 frames through the wrapper."""
    vols = [syn.blob_volume(33, 5), syn.sphere_volume(33), syn.blob_volume(33, 7), np.zeros((33, 33, 33), np.float32)]
    on, off = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    meshes = ops.marching_cubes_raw_batch([torch.from_numpy(v).to(DEV) for v in vols], 0.5, BMIN, BMAX,
                                          gates=[on, None, off, on])
    assert [m[2].cpu().tolist()[0] > 0 for m in meshes] == [True, True, False, False]
    for iterations in (1, 4):
        rc, outs, msg = _batch(abi, meshes, iterations)
        assert rc == MP_OK, msg
        for k, (m, o) in enumerate(zip(meshes, outs)):
            want = _single(abi, m, iterations)
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(o, want)), (iterations, k)
            _check(o, m, iterations, what="frame %d" % k)
        assert (outs[2][0] == POISON).all() and (outs[3][1] == IPOISON).all()
    # a ring for some frames only
    some = [_outs(meshes[0][0].shape[0], ring=k % 2 == 0) for k in range(4)]
    rc, _, msg = _batch(abi, meshes, 4, outs=some)
    assert rc == MP_OK, msg
    assert all(np.array_equal(_bits(a[0]), _bits(b[0])) for a, b in zip(some, outs))
    assert np.array_equal(_bits(some[0][1]), _bits(outs[0][1]))
    many = [meshes[k % 2] for k in range(33)]
    got = ops.mesh_smooth_raw_batch([m[0] for m in many], [m[1] for m in many], [m[2] for m in many], 3, ring=True)
    singles = [ops.mesh_smooth_raw(*meshes[k], 3, ring=True) for k in range(2)]
    assert len(got) == 33
    for k, (gv, gr) in enumerate(got):
        nv = int(meshes[k % 2][2][0])
        assert nv > 0 and np.array_equal(_bits(gv[:nv]), _bits(singles[k % 2][0][:nv])), k
        assert torch.equal(gr[:nv], singles[k % 2][1][:nv]), k
    nv = int(meshes[0][2][0])
    want = sm.smooth_ref(meshes[0][0][:nv].cpu().numpy(), meshes[0][1][:int(meshes[0][2][1])].cpu().numpy(), 3)
    assert np.array_equal(_bits(singles[0][0][:nv]), want.view(np.uint32))
    # the wrapper writes into a caller's buffers too; without ``ring`` it returns the vertices alone
    out = torch.empty_like(torch.stack([m[0] for m in meshes]))
    rings = torch.empty((4, meshes[0][0].shape[0]), dtype=torch.int32, device=DEV)
    mine = ops.mesh_smooth_raw_batch([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes], 3, out=out,
                                     ring=rings)
    assert mine[1][0].data_ptr() == out[1].data_ptr() and mine[1][1].data_ptr() == rings[1].data_ptr()
    alone = ops.mesh_smooth_raw(*meshes[0], 3, lam=LAM, mu=MU, pin_border=False)
    assert torch.is_tensor(alone) and np.array_equal(_bits(alone[:nv]), _bits(out[0][:nv]))  # closed: nothing pinned
    for bad in (dict(iterations=0), dict(iterations=65), dict(iterations=3.0), dict(iterations=True),
                dict(iterations=3, lam=float("nan")), dict(iterations=3, mu=float("inf")), dict(iterations=3, mu=1e39),
                dict(iterations=3, pin_border=1), dict(iterations=3, lam="0.5")):
        with pytest.raises(ValueError):
            ops.mesh_smooth_raw(*meshes[0], **bad)


def test_refusals(abi, device_meshes):
    lib, h, st = abi
    mesh = device_meshes["blob17_3"]
    most = lib.mp_max_frames()

    def refused(code, text, meshes=None, **kw):
        meshes = [mesh] if meshes is None else meshes
        outs = kw.pop("outs", None) or [_outs(mesh[0].shape[0]) for _ in meshes]
        before = [[None if t is None else t.clone() for t in o] for o in outs]
        rc, outs, msg = _batch(abi, meshes, outs=outs, **kw)
        assert rc == code and text in msg and msg, (rc, msg)
        for o, b in zip(outs, before):  # nothing was written
            assert all(t is None or torch.equal(t, u) for t, u in zip(o, b))

    refused(MP_ERR_ARG, "1..64 iterations", iterations=0)
    refused(MP_ERR_ARG, "1..64 iterations", iterations=65)
    refused(MP_ERR_ARG, "1..64 iterations", iterations=-1)
    refused(MP_ERR_ARG, "finite", lam=float("nan"))
    refused(MP_ERR_ARG, "finite", lam=float("inf"))
    refused(MP_ERR_ARG, "finite", mu=float("-inf"))
    refused(MP_ERR_ARG, "finite", mu=float("nan"))
    refused(MP_ERR_ARG, "unknown flags", flags=2)
    refused(MP_ERR_ARG, "unknown flags", flags=PIN | 4)
    refused(MP_ERR_ARG, "unknown flags", flags=-1)
    refused(MP_ERR_ARG, "1..%d frames per call, got %d" % (most, most + 1), meshes=[mesh] * (most + 1))
    refused(MP_ERR_ARG, "frames per call, got 0", n_frames=0)
    refused(MP_ERR_UNSUPPORTED, "2^31 / 6", max_f=2 ** 31 // 6 + 1)
    refused(MP_ERR_ARG, "bad argument", max_v=-1)
    good = _outs(mesh[0].shape[0])
    refused(MP_ERR_ARG, "null buffer for frame 0", outs=[(None, good[1])])
    refused(MP_ERR_ARG, "null buffer for frame 1", meshes=[mesh, (mesh[0], None, mesh[2])])
    refused(MP_ERR_ARG, "null buffer for frame 1", meshes=[mesh, (None, mesh[1], mesh[2])])
    refused(MP_ERR_ARG, "null buffer for frame 0", meshes=[(mesh[0], mesh[1], None)])
    raw = torch.full((mesh[0].numel() * 4 + 8,), 0, dtype=torch.uint8, device=DEV)
    odd = raw[2:2 + mesh[0].numel() * 4]
    assert odd.data_ptr() % 4 == 2
    refused(MP_ERR_ARG, "misaligned buffer for frame 0", meshes=[(odd, mesh[1], mesh[2])], outs=[good],
            max_v=mesh[0].shape[0])
    refused(MP_ERR_ARG, "misaligned buffer for frame 0", outs=[(good[0], odd)])
    refused(MP_ERR_ARG, "misaligned buffer for frame 0", outs=[(odd, good[1])])
    # aliasing: an output on an input of the same frame, on one of another frame, and overlapping one in part
    refused(MP_ERR_ARG, "aliases", outs=[(mesh[0], good[1])], ring=False)
    as_ring = mesh[1].view(-1)[:mesh[0].shape[0]]
    refused(MP_ERR_ARG, "aliases", meshes=[mesh, (good[0].clone(), mesh[1], mesh[2])],
            outs=[(good[0], as_ring), _outs(mesh[0].shape[0])])
    refused(MP_ERR_ARG, "aliases", meshes=[mesh, (good[0], mesh[1], mesh[2])],
            outs=[(good[0], good[1]), _outs(mesh[0].shape[0])])
    cap = mesh[0].shape[0]
    long = torch.full((2 * cap, 3), POISON, device=DEV)
    refused(MP_ERR_ARG, "aliases", meshes=[(long[:cap], mesh[1], mesh[2])], outs=[(long[cap // 2:cap // 2 + cap], good[1])])
    # the per-mesh call shares the checks and names itself
    for iterations, lam, flags, cap_f, code in ((0, LAM, PIN, 10, MP_ERR_ARG), (3, float("nan"), PIN, 10, MP_ERR_ARG),
                                                (3, LAM, 8, 10, MP_ERR_ARG),
                                                (3, LAM, PIN, 2 ** 31 // 6 + 1, MP_ERR_UNSUPPORTED)):
        rc = lib.mp_mesh_smooth(h, _p(mesh[0]), 10, _p(mesh[1]), cap_f, _p(mesh[2]), iterations, lam, MU, flags,
                                _p(good[0]), _p(good[1]), st)
        assert rc == code and lib.mp_last_error(h).decode().startswith("mp_mesh_smooth:")
    assert lib.mp_mesh_smooth(h, _p(mesh[0]), 10, _p(mesh[1]), 10, None, 3, LAM, MU, PIN, _p(good[0]), None,
                              st) == MP_ERR_ARG
    assert lib.mp_mesh_smooth(h, _p(mesh[0]), 10, _p(mesh[1]), 10, _p(mesh[2]), 3, LAM, MU, PIN, _p(mesh[0]), None,
                              st) == MP_ERR_ARG
    assert all((t == (POISON if t.dtype == torch.float32 else IPOISON)).all() for t in good)


# ---- Python layers ------------------------------------------------------------------------------------------------

def _same_mesh(a, b, what=""):
    assert (a is None) == (b is None), what
    if a is None:
        return
    for name, x, y in zip(a._fields, a, b):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape)
            assert np.array_equal(_bits(x) if x.dtype == torch.float32 else x.cpu().numpy(),
                                  _bits(y) if y.dtype == torch.float32 else y.cpu().numpy()), (what, name)


@pytest.fixture(scope="module")
def colour():
    """A netC with seeded weights, one feature map and camera per volume (the recipe of tools/mesh_timing.py)."""
    from monoport_amd.modeling import PIFuNetC
    net = PIFuNetC()
    with torch.no_grad():
        for i, (w, b) in enumerate(syn.rand_mlp("C", 61, 2.0)):
            net.surface_classifier.filters[i].weight.copy_(torch.from_numpy(w)[:, :, None])
            net.surface_classifier.filters[i].bias.copy_(torch.from_numpy(b))
    net.surface_classifier.to(DEV)
    net.eval()
    feats = [[[torch.from_numpy(syn.rand_feat(512, 128, 128, 62 + k))[None].to(DEV)]] for k in range(3)]
    calibs = [torch.eye(4, device=DEV)[None] for _ in range(3)]
    return net, feats, calibs


def _by_hand(ops, vol, smooth, normals, binding, clean=None, simplify=None):
    """The chain of reconstruct_mesh(..., smooth=...) composed from the raw calls: the colours are queried at the
    vertices before smoothing."""
    from monoport_amd.recon import Mesh
    if clean is not None:
        vol = ops.keep_largest_raw(vol, 0.5, clean, 0.0)[0]
    verts, faces, counts = ops.marching_cubes_raw(vol, 0.5, BMIN, BMAX)
    if simplify is not None:
        verts, faces, counts, _ = ops.mesh_simplify_raw(verts, faces, counts, simplify, BMIN, BMAX)
    moved = ops.mesh_smooth_raw(verts, faces, counts, **smooth)
    nrm = ops.mesh_normals_raw(moved, faces, counts, normals) if normals is not None else None
    col = None
    if binding is not None:
        pts, count = ops.mesh_points_raw(verts, counts)
        col = ops.query_counted(binding.mlp, binding.feat_hwc, pts, count, binding.calib, binding.z_scale)
    nv, nf = counts.cpu().tolist()
    assert not torch.equal(moved[:nv], verts[:nv])
    return Mesh(moved[:nv], faces[:nf], None if nrm is None else nrm[:nv],
                None if col is None else (col * 0.5 + 0.5).t()[:nv].contiguous())


def _body_floater():
    """A sphere of radius 0.5 about the origin and a small blob at (0.75, 0.75, 0.75)."""
    g = ((np.arange(33) + 0.5) / 33) * 2 - 1
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    body = np.sqrt(x * x + y * y + z * z) < 0.5
    blob = np.sqrt((x - 0.75) ** 2 + (y - 0.75) ** 2 + (z - 0.75) ** 2) < 0.12
    return np.where(body | blob, 0.9, 0.1).astype(np.float32)


THREE = dict(iterations=3, lam=0.5, mu=-0.53, pin_border=True)


def test_reconstruct_mesh_smooth(ops, colour):
    from monoport_amd import recon
    net, feats, calibs = colour
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    before = vol.clone()
    binding = recon._bind_netC("test", net, [(feats[0], calibs[0], vol.device)])[0]
    kw = dict(netC=net, feat_tensor_C=feats[0], calib_tensor=calibs[0])
    plain = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, **kw)
    got = recon.reconstruct_mesh(vol[None, None], 0.5, BMIN, BMAX, smooth=3, **kw)
    _same_mesh(got, _by_hand(ops, vol, THREE, "accumulate", binding), "with netC")
    assert got.verts.shape == (1562, 3) and torch.equal(got.faces, plain.faces)
    assert torch.equal(got.colors, plain.colors)  # queried on the iso-surface: the bits of smooth=None
    assert not torch.equal(got.verts, plain.verts) and not torch.equal(got.normals, plain.normals)
    # the definition, through every layer
    want = sm.smooth_ref(plain.verts.cpu().numpy(), plain.faces.cpu().numpy(), 3)
    assert np.array_equal(_bits(got.verts), want.view(np.uint32))
    _same_mesh(recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, normals="reference", smooth=3),
               _by_hand(ops, vol, THREE, "reference", None), "without netC")
    other = dict(iterations=2, lam=0.3, mu=-0.31, pin_border=False)
    _same_mesh(recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, normals=None, smooth=other),
               _by_hand(ops, vol, other, None, None), "a dict, no normals")
    _same_mesh(recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, smooth={"iterations": 3}),
               recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, smooth=3), "a dict of the defaults")
    both = torch.from_numpy(_body_floater()).to(DEV)
    cleaned = recon.reconstruct_mesh(both, 0.5, BMIN, BMAX, clean=6, smooth=3, **kw)
    _same_mesh(cleaned, _by_hand(ops, both, THREE, "accumulate", binding, clean=6), "clean=6")
    assert float(cleaned.verts.abs().max()) < 0.6 < float(recon.reconstruct_mesh(both, 0.5, BMIN, BMAX, smooth=3).verts.max())
    small = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, simplify=16, smooth=3, **kw)
    _same_mesh(small, _by_hand(ops, vol, THREE, "accumulate", binding, simplify=16), "simplify=16")
    assert small.verts.shape == (285, 3)
    assert torch.equal(small.colors, recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, simplify=16, **kw).colors)
    assert torch.equal(vol, before)
    # the default leaves the call alone; bad values are refused before anything runs
    _same_mesh(plain, recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, smooth=None, **kw), "smooth=None")
    for bad in (0, 65, -1, 3.0, "3", True, {}, {"lam": 0.5}, {"iterations": 3, "lambda": 0.5},
                {"iterations": 3, "mu": float("nan")}, {"iterations": 3, "pin_border": "yes"}):
        with pytest.raises(ValueError):
            recon.reconstruct_mesh(vol, smooth=bad)
        with pytest.raises(ValueError):
            recon.reconstruct_mesh_many([vol], smooth=bad)
    assert recon.reconstruct_mesh(None, smooth=3) is None
    # a capacity guess that is short: the whole chain runs again with exact capacities
    real = ops.marching_cubes_raw_batch
    try:
        ops.marching_cubes_raw_batch = lambda s, level, lo, hi, max_verts=None, max_faces=None, **kw: real(
            s, level, lo, hi, max_verts=max_verts or 100, max_faces=max_faces or 150, **kw)
        _same_mesh(recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, smooth=3, **kw), got, "short capacities")
    finally:
        ops.marching_cubes_raw_batch = real


def test_reconstruct_mesh_many_smooth(colour):
    from monoport_amd import recon
    net, feats, calibs = colour
    sdfs = [torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)[None, None], None,
            torch.from_numpy(syn.sphere_volume(33)).to(DEV), torch.zeros((33, 33, 33), device=DEV)]
    feats4, calibs4 = [feats[0], None, feats[1], feats[2]], [calibs[0], None, calibs[1], calibs[2]]
    for simplify in (None, 16):
        got = recon.reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, netC=net, feat_tensors_C=feats4, calib_tensors=calibs4,
                                          simplify=simplify, smooth=3)
        assert got[1] is None and got[3].verts.shape == (0, 3) and got[3].faces.shape == (0, 3)
        for i in (0, 2, 3):
            _same_mesh(got[i], recon.reconstruct_mesh(sdfs[i], 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feats4[i],
                                                      calib_tensor=calibs4[i], simplify=simplify, smooth=3),
                       "frame %d" % i)
    plain = recon.reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, normals=None, simplify=16)
    assert torch.equal(got[0].faces, plain[0].faces) and not torch.equal(got[0].verts, plain[0].verts)
    assert recon.reconstruct_mesh_many([None, None], smooth=3) == [None, None]


def test_smooth_mesh_and_render(ops, colour):
    """recon.smooth_mesh on a finished mesh equals smoothing inside the chain, colours included, and the rasteriser
    takes the result (the pieces connect)."""
    from monoport_amd import recon
    net, feats, calibs = colour
    kw = dict(netC=net, feat_tensor_C=feats[0], calib_tensor=calibs[0])
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    full = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, **kw)
    fair = recon.smooth_mesh(full, 3)
    _same_mesh(fair, recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, smooth=3, **kw), "smooth_mesh")
    assert fair.colors is full.colors and fair.normals.shape == fair.verts.shape
    want = sm.smooth_ref(full.verts.cpu().numpy(), full.faces.cpu().numpy(), 10, 0.4, -0.42, False)
    pair = recon.smooth_mesh((full.verts, full.faces), lam=0.4, mu=-0.42, pin_border=False, normals=None)
    assert pair.normals is None and pair.colors is None and np.array_equal(_bits(pair.verts), want.view(np.uint32))
    assert recon.smooth_mesh(None) is None
    empty = recon.smooth_mesh((full.verts[:0], full.faces[:0]), 3)
    assert empty.verts.shape == (0, 3) and empty.faces.shape == (0, 3)
    with pytest.raises(ValueError):
        recon.smooth_mesh(full, 0)
    shot = recon.render_mesh(fair, torch.eye(4, device=DEV), res=65, shade="normals")
    covered = int((shot.face >= 0).sum())
    print("smoothed blob at 65 x 65: %d pixels covered" % covered)
    assert covered >= 1 and int(shot.face.max()) < fair.faces.shape[0]


# ---- FrameSlot(mesh={"smooth": ...}) ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    import bench
    dev = torch.device(DEV)
    return bench.build_netg(dev)[0], bench.build_netc(dev)


@pytest.mark.parametrize("mesh_batch", [None, 2])
def test_slot_smooth(nets, mesh_batch, monkeypatch):
    """The slot's smallest admissible frames, the volumes filled in by hand (two bodies, a frame switched off by its
    status whose volume is NaN, an empty volume, a body with a floater), in one chunk and in chunks of 2 + 2 + 1."""
    from monoport_amd import pipeline, recon
    from monoport_amd.modeling.MonoPortNet import QueryBinding
    from monoport_amd.pipeline import FrameSlot
    if mesh_batch is not None:
        monkeypatch.setattr(pipeline, "MESH_BATCH", mesh_batch)
    netg, netc = nets
    vols = [torch.from_numpy(syn.blob_volume(33, 5)).to(DEV), torch.from_numpy(syn.sphere_volume(33)).to(DEV),
            torch.full((33, 33, 33), float("nan"), device=DEV), torch.zeros((33, 33, 33), device=DEV),
            torch.from_numpy(_body_floater()).to(DEV)]

    def make(**mesh):
        return FrameSlot(netg, torch.device(DEV), netC=netc, batch=5, resolutions=(17, 33), b_min=BMIN, b_max=BMAX, mesh=mesh)

    plain, slot = make(normals="accumulate", simplify=16), make(normals="accumulate", smooth=3, simplify=16)
    try:
        assert slot.mesh._replace(smooth=None) == plain.mesh and slot.mesh.smooth == THREE and plain.mesh.smooth is None
        assert "smooth_verts" not in plain.mesh_buffers
        assert slot.mesh_buffers["smooth_verts"].shape == slot.mesh_buffers["verts"].shape
        with pytest.raises(ValueError):
            make(smooth=0)
        with pytest.raises(ValueError):
            make(smoth=3)
        for s in (plain, slot):
            torch.cuda.synchronize()
            with torch.cuda.stream(s.stream):
                for b, v in enumerate(vols):
                    s.volumes[b].copy_(v)
                    s.feats_hwc_c[b].copy_(torch.from_numpy(syn.rand_feat(128, 128 * 512, 1, 80 + b)).to(DEV).view(128, 128, 512))
                s.status.zero_()
                s.status[:, 0] = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32)
                s.n_active = 5
                s._mesh_chain(5)
            s._busy = True
        got, rough = slot.meshes(), plain.meshes()
        assert [g is None for g in got] == [False, False, True, False, False]
        assert got[3].verts.shape == (0, 3) and got[3].faces.shape == (0, 3)
        assert got[0].verts.data_ptr() == slot.mesh_buffers["smooth_verts"].data_ptr()
        mlp_c = netc.surface_classifier.packed()
        for b in (0, 1, 3, 4):
            binding = QueryBinding(netc, mlp_c, slot.feats_hwc_c[b], slot.calib[b:b + 1], syn.Z_SCALE)
            opts = recon.mesh_options("accumulate", 0.5, True, simplify=16, smooth=THREE)
            chain = recon._mesh_chains([slot.volumes[b]], BMIN, BMAX, opts, [binding])[0]
            nv, nf = chain.counts.cpu().tolist()
            _same_mesh(got[b], recon._finish_mesh(chain, nv, nf), "frame %d" % b)
            # geometry and normals: the public per-volume call on the slot's volume
            want = recon.reconstruct_mesh(slot.volumes[b], 0.5, BMIN, BMAX, simplify=16, smooth=3)
            _same_mesh(got[b]._replace(colors=None), want, "frame %d, reconstruct_mesh" % b)
            # the same faces and colours as without the option, other vertices
            assert torch.equal(got[b].faces, rough[b].faces) and torch.equal(got[b].colors, rough[b].colors)
            assert nv == 0 or not torch.equal(got[b].verts, rough[b].verts)
            # the clustered mesh stays in the slot beside the smoothed one
            assert torch.equal(slot.mesh_buffers["simple_verts"][b, :nv], rough[b].verts)
        assert got[0].verts.shape == (285, 3) and got[0].colors.shape == (285, 3)
    finally:
        slot.close()
        plain.close()
