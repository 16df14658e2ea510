"""mp_mesh_simplify / mp_mesh_simplify_batch (csrc/simplify.hip) through ctypes, ops.mesh_simplify_raw[_batch],
recon.simplify_mesh and the ``simplify`` option of recon.reconstruct_mesh, recon.reconstruct_mesh_many and
FrameSlot(mesh=...), on the GPU.  The kernels are held to the definition's numpy restatement
(tests/mesh_simplify_ref.py, itself held to a slow implementation in tests/test_mesh_simplify_ref_cpu.py): verts_out bit
for bit (as uint32), faces_out, vmap and counts_out exactly, rows beyond the counts untouched.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import mesh_simplify_ref as ms
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED = 0, -1, -3
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


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _mesh_on_device(verts, faces, counts=None):
    """numpy (verts, faces) -> device (verts, faces, counts = their sizes unless given)."""
    v = torch.from_numpy(np.array(verts, np.float32).reshape(-1, 3)).to(DEV)  # a copy: the fixtures are read-only
    f = torch.from_numpy(np.array(faces, np.int32).reshape(-1, 3)).to(DEV)
    c = torch.tensor([v.shape[0], f.shape[0]] if counts is None else counts, dtype=torch.int32, device=DEV)
    return v, f, c


def _outs(max_v, max_f, vmap=True):
    return (torch.full((max_v, 3), POISON, device=DEV), torch.full((max_f, 3), IPOISON, dtype=torch.int32, device=DEV),
            torch.full((2,), IPOISON, dtype=torch.int32, device=DEV),
            torch.full((max_v,), IPOISON, dtype=torch.int32, device=DEV) if vmap else None)


def _single(abi, mesh, n, b_min=BMIN, b_max=BMAX, vmap=True, max_v=None, max_f=None):
    """One mp_mesh_simplify call into poisoned buffers -> (verts_out, faces_out, counts_out, vmap)."""
    lib, h, st = abi
    v, f, c = mesh
    max_v = v.shape[0] if max_v is None else max_v
    max_f = f.shape[0] if max_f is None else max_f
    outs = _outs(max_v, max_f, vmap)
    rc = lib.mp_mesh_simplify(h, _p(v), max_v, _p(f) if max_f else None, max_f, _p(c), _f3(b_min), _f3(b_max), n,
                              _p(outs[0]), _p(outs[1]) if max_f else None, _p(outs[2]), _p(outs[3]), st)
    assert rc == MP_OK, lib.mp_last_error(h).decode()
    return outs


def _check(outs, mesh, n, b_min=BMIN, b_max=BMAX, what=""):
    """The outputs of a call against the restatement on the rows of ``mesh`` that the call may read."""
    v, f, c = mesh
    vo, fo, co, vm = outs
    nv, nf = (min(int(x), cap) for x, cap in zip(c.cpu().tolist(), (vo.shape[0], fo.shape[0])))
    want_v, want_f, want_map = ms.simplify_ref(v[:nv].cpu().numpy(), f[:nf].cpu().numpy(), n, b_min, b_max)
    assert co.cpu().tolist() == [len(want_v), len(want_f)], (what, co.cpu().tolist(), len(want_v), len(want_f))
    assert np.array_equal(_bits(vo[:len(want_v)]), want_v.view(np.uint32)), what
    assert np.array_equal(fo[:len(want_f)].cpu().numpy(), want_f), what
    assert (vo[len(want_v):] == POISON).all() and (fo[len(want_f):] == IPOISON).all(), what
    if vm is not None:
        assert np.array_equal(vm[:nv].cpu().numpy(), want_map) and (vm[nv:] == IPOISON).all(), what
    return len(want_v), len(want_f)


@pytest.fixture(scope="module")
def device_meshes(ops):
    """The device's own marching-cubes meshes at the capacities of ops.marching_cubes_raw (counts below them)."""
    vols = {"blob33_5": syn.blob_volume(33, 5), "blob17_3": syn.blob_volume(17, 3)}
    return {k: ops.marching_cubes_raw(torch.from_numpy(v).to(DEV), 0.5, BMIN, BMAX) for k, v in vols.items()}


@pytest.mark.parametrize("name", ["blob33_5", "blob17_3"])
def test_device_meshes_against_the_definition(abi, device_meshes, name):
    """Scan tails, several blocks of faces (3,124 at 33^3), cell tables that are no multiple of the block (n = 3, 33,
    66) and larger than one block of block sums' worth of cells."""
    mesh = device_meshes[name]
    sizes = {}
    for n in (1, 2, 3, 8, 16, 33, 66):
        sizes[n] = _check(_single(abi, mesh, n), mesh, n, what="%s n = %d" % (name, n))
    print("%s %s -> %s" % (name, mesh[2].cpu().tolist(), sizes))
    assert sizes[1] == (1, 0)
    if name == "blob33_5":
        assert mesh[2].cpu().tolist() == [1562, 3124]
        assert (sizes[16], sizes[33], sizes[66]) == ((285, 576), (848, 1710), (1372, 2746))
        gold_v, gold_f = ms.oracle_mesh("blob33_5")  # the device's mesh is the oracle's
        assert np.array_equal(_bits(mesh[0][:1562]), gold_v.view(np.uint32))
        assert np.array_equal(mesh[1][:3124].cpu().numpy(), gold_f)


def test_512_cells_per_axis(abi, device_meshes):
    """131,072 block sums: the one-block scan takes 128 steps."""
    mesh = device_meshes["blob17_3"]
    nv, nf = _check(_single(abi, mesh, 512), mesh, 512, what="n = 512")
    assert nv <= mesh[2][0].item() and nv > 0.9 * mesh[2][0].item()


def test_soup(abi):
    v, f = ms.soup()
    mesh = _mesh_on_device(v, f)
    outs = _single(abi, mesh, ms.SOUP_CELLS, ms.SOUP_BMIN, ms.SOUP_BMAX)
    nv, nf = _check(outs, mesh, ms.SOUP_CELLS, ms.SOUP_BMIN, ms.SOUP_BMAX, "soup")
    assert (outs[3][-6:] == -1).all() and 0 < nf < len(f)
    assert np.array_equal(_bits(mesh[0]), v.view(np.uint32)) and np.array_equal(mesh[1].cpu().numpy(), f)  # only read


def test_a_cell_of_300000_members(abi):
    """Sums beyond 2^53: the int64 -> double conversion rounds to nearest-even.  No faces: a capacity of 0, NULL rows."""
    mesh = _mesh_on_device(ms.crowd(), np.zeros((0, 3), np.int32))
    outs = _single(abi, mesh, ms.CROWD_CELLS, ms.CROWD_BMIN, ms.CROWD_BMAX)
    assert _check(outs, mesh, ms.CROWD_CELLS, ms.CROWD_BMIN, ms.CROWD_BMAX, "crowd") == (1, 0)
    assert (outs[3] == 0).all()


def test_counts_and_capacities(abi, device_meshes):
    v, f, c = device_meshes["blob33_5"]
    nv, nf = c.cpu().tolist()
    # the counts exceed the capacities: only the capacities are read, a face that names a vertex beyond them is dropped
    outs = _single(abi, (v, f, c), 16, max_v=nv - 30, max_f=nf - 10)
    got = _check(outs, (v, f, c), 16, what="short capacities")
    assert 0 < got[0] <= 285 and 0 < got[1] <= 576
    # no mesh (a gated-off frame): the counts, nothing else
    zero = torch.zeros(2, dtype=torch.int32, device=DEV)
    outs = _single(abi, (v, f, zero), 16)
    assert outs[2].cpu().tolist() == [0, 0]
    assert (outs[0] == POISON).all() and (outs[1] == IPOISON).all() and (outs[3] == IPOISON).all()
    # without a vmap: the same mesh
    a, b = _single(abi, (v, f, c), 16, vmap=False), _single(abi, (v, f, c), 16)
    assert _check(a, (v, f, c), 16, what="no vmap") == (285, 576)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:3], b[:3]))
    # a capacity of 0 vertices: MP_OK, counts zeroed, no buffer needed
    lib, h, st = abi
    co = torch.full((2,), IPOISON, dtype=torch.int32, device=DEV)
    assert lib.mp_mesh_simplify(h, None, 0, None, 0, _p(c), _f3(BMIN), _f3(BMAX), 4, None, None, _p(co), None, st) == MP_OK
    assert co.cpu().tolist() == [0, 0]


def test_repeatable_under_contention(abi):
    """2,000 vertices in one cell (every add lands on one row), twice: the same bits, and the definition's."""
    rng = np.random.RandomState(23)
    v = (0.3 + 0.2 * rng.rand(2000, 3)).astype(np.float32)  # cell (1, 1, 1) of 2^3
    f = rng.randint(0, 2000, (500, 3)).astype(np.int32)
    mesh = _mesh_on_device(v, f)
    first, second = _single(abi, mesh, 2), _single(abi, mesh, 2)
    assert _check(first, mesh, 2, what="one cell") == (1, 0)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(first, second))


def _batch(abi, meshes, n, b_min=BMIN, b_max=BMAX, n_frames=None, max_v=None, max_f=None, outs=None, vmap=True):
    lib, h, st = abi
    max_v = meshes[0][0].shape[0] if max_v is None else max_v
    max_f = meshes[0][1].shape[0] if max_f is None else max_f
    if outs is None:
        outs = [_outs(meshes[0][0].shape[0], meshes[0][1].shape[0]) for _ in meshes]
    rc = lib.mp_mesh_simplify_batch(h, len(meshes) if n_frames is None else n_frames, _pp([m[0] for m in meshes]), max_v,
                                    _pp([m[1] for m in meshes]), max_f, _pp([m[2] for m in meshes]), _f3(b_min),
                                    _f3(b_max), n, _pp([o[0] for o in outs]), _pp([o[1] for o in outs]),
                                    _pp([o[2] for o in outs]), _pp([o[3] for o in outs]) if vmap else None, st)
    return rc, outs, lib.mp_last_error(h).decode()


def test_batch_equals_single_calls(abi, ops):
    """Unequal meshes of one capacity, one of them switched off, in one call; then 33 frames through the wrapper."""
    vols = [syn.blob_volume(33, 5), syn.sphere_volume(33), syn.blob_volume(33, 7), np.zeros((33, 33, 33), np.float32)]
    on, off = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    meshes = ops.marching_cubes_raw_batch([torch.from_numpy(v).to(DEV) for v in vols], 0.5, BMIN, BMAX,
                                          gates=[on, None, off, on])
    assert [m[2].cpu().tolist()[0] > 0 for m in meshes] == [True, True, False, False]
    for n in (16, 33):
        rc, outs, msg = _batch(abi, meshes, n)
        assert rc == MP_OK, msg
        for k, (m, o) in enumerate(zip(meshes, outs)):
            want = _single(abi, m, n)
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(o, want)), (n, k)
            _check(o, m, n, what="frame %d" % k)
        assert outs[2][2].cpu().tolist() == [0, 0] and outs[3][2].cpu().tolist() == [0, 0]
    many = [meshes[k % 2] for k in range(33)]
    got = ops.mesh_simplify_raw_batch([m[0] for m in many], [m[1] for m in many], [m[2] for m in many], 16, BMIN, BMAX)
    singles = [ops.mesh_simplify_raw(*meshes[k], 16, BMIN, BMAX) for k in range(2)]
    assert len(got) == 33
    for k, g in enumerate(got):
        nv, nf = g[2].cpu().tolist()
        assert (nv, nf) == tuple(singles[k % 2][2].cpu().tolist()) and nv > 0
        want = singles[k % 2]
        assert np.array_equal(_bits(g[0][:nv]), _bits(want[0][:nv])) and torch.equal(g[1][:nf], want[1][:nf]), k
        old = int(meshes[k % 2][2][0])
        assert torch.equal(g[3][:old], want[3][:old]), k
    # the wrapper writes into a caller's buffers too
    out = (torch.empty_like(torch.stack([m[0] for m in meshes])), torch.empty_like(torch.stack([m[1] for m in meshes])),
           torch.empty((4, 2), dtype=torch.int32, device=DEV), torch.empty((4, meshes[0][0].shape[0]), dtype=torch.int32, device=DEV))
    mine = ops.mesh_simplify_raw_batch([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes], 16, out=out)
    assert mine[1][0].data_ptr() == out[0][1].data_ptr() and out[2].cpu().tolist()[0] == singles[0][2].cpu().tolist()
    with pytest.raises(ValueError):
        ops.mesh_simplify_raw(*meshes[0], 0)
    with pytest.raises(ValueError):
        ops.mesh_simplify_raw(*meshes[0], 513)
    with pytest.raises(ValueError):
        ops.mesh_simplify_raw(*meshes[0], 16.0)


def test_refusals(abi, device_meshes):
    lib, h, st = abi
    mesh = device_meshes["blob17_3"]
    most = lib.mp_max_frames()

    def refused(code, text, meshes=None, **kw):
        meshes = [mesh] if meshes is None else meshes
        n = kw.pop("n", 8)
        rc, outs, msg = _batch(abi, meshes, n, **kw)
        assert rc == code and text in msg and msg, (rc, msg)
        for o in outs:
            assert all(t is None or (t == (POISON if t.dtype == torch.float32 else IPOISON)).all() for t in o)

    refused(MP_ERR_ARG, "1..512 cells", n=0)
    refused(MP_ERR_ARG, "1..512 cells", n=513)
    refused(MP_ERR_ARG, "b_max > b_min", b_max=[1.0, -1.0, 1.0])
    refused(MP_ERR_ARG, "b_max > b_min", b_min=[-1.0, -1.0, -2.0], b_max=[1.0, 1.0, -3.0])
    refused(MP_ERR_ARG, "finite", b_min=[float("nan"), -1.0, -1.0])
    refused(MP_ERR_ARG, "finite", b_max=[1.0, float("inf"), 1.0])
    refused(MP_ERR_ARG, "too thin", b_min=[0.0, -1.0, -1.0], b_max=[1e-44, 1.0, 1.0])
    refused(MP_ERR_ARG, "1..%d frames per call, got %d" % (most, most + 1), meshes=[mesh] * (most + 1))
    refused(MP_ERR_ARG, "frames per call, got 0", n_frames=0)
    refused(MP_ERR_UNSUPPORTED, "2^27", max_v=2 ** 27 + 1)
    refused(MP_ERR_UNSUPPORTED, "2^31 / 3", max_f=2 ** 31 // 3 + 1)
    good = _outs(mesh[0].shape[0], mesh[1].shape[0])
    for k in range(3):  # a NULL output; vmap may only be NULL as a whole
        outs = list(good)
        outs[k] = None
        refused(MP_ERR_ARG, "null buffer for frame 0", outs=[tuple(outs)])
    refused(MP_ERR_ARG, "null buffer for frame 1", meshes=[mesh, (mesh[0], None, mesh[2])])
    raw = torch.full((mesh[0].numel() * 4 + 8,), 0, dtype=torch.uint8, device=DEV)
    odd = raw[2:2 + mesh[0].numel() * 4]
    assert odd.data_ptr() % 4 == 2
    refused(MP_ERR_ARG, "misaligned buffer for frame 0", meshes=[(odd, mesh[1], mesh[2])], outs=[good],
            max_v=mesh[0].shape[0])
    # aliasing: an output on an input of the same frame, on one of another frame, and overlapping one in part
    refused(MP_ERR_ARG, "aliases", meshes=[(good[0], mesh[1], mesh[2])], outs=[good])
    refused(MP_ERR_ARG, "aliases", meshes=[mesh, (mesh[0], good[1], mesh[2])],
            outs=[good, _outs(mesh[0].shape[0], mesh[1].shape[0])])
    cap = mesh[0].shape[0]
    long = torch.full((2 * cap, 3), POISON, device=DEV)
    refused(MP_ERR_ARG, "aliases", meshes=[(long[:cap], mesh[1], mesh[2])],
            outs=[(long[cap // 2:cap // 2 + cap], good[1], good[2], good[3])])
    # the per-mesh call shares the checks and names itself
    for n, lo, hi, cap_v, code in ((0, BMIN, BMAX, 10, MP_ERR_ARG), (8, BMAX, BMIN, 10, MP_ERR_ARG),
                                   (8, BMIN, BMAX, 2 ** 27 + 1, MP_ERR_UNSUPPORTED)):
        rc = lib.mp_mesh_simplify(h, _p(mesh[0]), cap_v, _p(mesh[1]), 10, _p(mesh[2]), _f3(lo), _f3(hi), n, _p(good[0]),
                                  _p(good[1]), _p(good[2]), None, st)
        assert rc == code and lib.mp_last_error(h).decode().startswith("mp_mesh_simplify:")
    assert lib.mp_mesh_simplify(h, _p(mesh[0]), 10, _p(mesh[1]), 10, None, _f3(BMIN), _f3(BMAX), 8, _p(good[0]),
                                _p(good[1]), _p(good[2]), None, st) == MP_ERR_ARG
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


def _by_hand(ops, vol, cells, normals, binding, clean=None):
    """The chain of reconstruct_mesh(..., simplify=cells) composed from the raw calls."""
    from monoport_amd.recon import Mesh
    if clean is not None:
        vol = ops.keep_largest_raw(vol, 0.5, clean, 0.0)[0]
    verts, faces, counts = ops.marching_cubes_raw(vol, 0.5, BMIN, BMAX)
    sv, sf, sc, _ = ops.mesh_simplify_raw(verts, faces, counts, cells, BMIN, BMAX)
    nrm = ops.mesh_normals_raw(sv, sf, sc, normals) if normals is not None else None
    col = None
    if binding is not None:
        pts, count = ops.mesh_points_raw(sv, sc)
        col = ops.query_counted(binding.mlp, binding.feat_hwc, pts, count, binding.calib, binding.z_scale)
    nv, nf = sc.cpu().tolist()
    assert (nv, nf) != tuple(counts.cpu().tolist()) and nv <= counts[0].item()
    return Mesh(sv[:nv], sf[:nf], None if nrm is None else nrm[:nv],
                None if col is None else (col * 0.5 + 0.5).t()[:nv].contiguous())


def test_reconstruct_mesh_simplify(ops, colour):
    from monoport_amd import recon
    net, feats, calibs = colour
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    before = vol.clone()
    binding = recon._bind_netC("test", net, [(feats[0], calibs[0], vol.device)])[0]
    kw = dict(netC=net, feat_tensor_C=feats[0], calib_tensor=calibs[0])
    got = recon.reconstruct_mesh(vol[None, None], 0.5, BMIN, BMAX, simplify=16, **kw)
    _same_mesh(got, _by_hand(ops, vol, 16, "accumulate", binding), "with netC")
    assert got.verts.shape == (285, 3) and got.faces.shape == (576, 3) and got.colors.shape == (285, 3)
    assert float(got.colors.min()) >= 0 and float(got.colors.max()) <= 1 and not (got.normals == 0).all()
    _same_mesh(recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, normals="reference", simplify=16),
               _by_hand(ops, vol, 16, "reference", None), "without netC")
    _same_mesh(recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, normals=None, simplify=33),
               _by_hand(ops, vol, 33, None, None), "no normals")
    both = torch.from_numpy(_body_floater()).to(DEV)
    cleaned = recon.reconstruct_mesh(both, 0.5, BMIN, BMAX, clean=6, simplify=16, **kw)
    _same_mesh(cleaned, _by_hand(ops, both, 16, "accumulate", binding, clean=6), "clean=6")
    assert float(cleaned.verts.abs().max()) < 0.6
    assert float(recon.reconstruct_mesh(both, 0.5, BMIN, BMAX, simplify=16).verts.max()) > 0.7
    assert torch.equal(vol, before)
    # the default leaves the call alone; bad values are refused before anything runs
    plain = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, **kw)
    _same_mesh(plain, recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, simplify=None, **kw), "simplify=None")
    assert plain.verts.shape == (1562, 3)
    for bad in (0, 513, -1, 16.0, "16", True):
        with pytest.raises(ValueError):
            recon.reconstruct_mesh(vol, simplify=bad)
        with pytest.raises(ValueError):
            recon.reconstruct_mesh_many([vol], simplify=bad)
        with pytest.raises(ValueError):
            recon.simplify_mesh(plain, bad)
    assert recon.reconstruct_mesh(None, simplify=16) is None
    # a capacity guess that is short: the whole chain runs again with exact capacities
    real = ops.marching_cubes_raw_batch
    try:
        ops.marching_cubes_raw_batch = lambda s, level, lo, hi, max_verts=None, max_faces=None, **kw: real(
            s, level, lo, hi, max_verts=max_verts or 100, max_faces=max_faces or 150, **kw)
        _same_mesh(recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, simplify=16, **kw), got, "short capacities")
    finally:
        ops.marching_cubes_raw_batch = real


def _body_floater():
    """A sphere of radius 0.5 about the origin and a small blob at (0.75, 0.75, 0.75)."""
    g = ((np.arange(33) + 0.5) / 33) * 2 - 1
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    body = np.sqrt(x * x + y * y + z * z) < 0.5
    blob = np.sqrt((x - 0.75) ** 2 + (y - 0.75) ** 2 + (z - 0.75) ** 2) < 0.12
    return np.where(body | blob, 0.9, 0.1).astype(np.float32)


def test_reconstruct_mesh_many_simplify(colour):
    from monoport_amd import recon
    net, feats, calibs = colour
    sdfs = [torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)[None, None], None,
            torch.from_numpy(syn.sphere_volume(33)).to(DEV), torch.zeros((33, 33, 33), device=DEV)]
    feats4, calibs4 = [feats[0], None, feats[1], feats[2]], [calibs[0], None, calibs[1], calibs[2]]
    for clean in (None, 26):
        got = recon.reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, netC=net, feat_tensors_C=feats4, calib_tensors=calibs4,
                                          clean=clean, simplify=16)
        assert got[1] is None and got[3].verts.shape == (0, 3) and got[3].faces.shape == (0, 3)
        for i in (0, 2, 3):
            _same_mesh(got[i], recon.reconstruct_mesh(sdfs[i], 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feats4[i],
                                                      calib_tensor=calibs4[i], clean=clean, simplify=16), "frame %d" % i)
    plain = recon.reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, normals=None)
    assert got[0].verts.shape[0] == 285 < plain[0].verts.shape[0] and 0 < got[2].verts.shape[0] < plain[2].verts.shape[0]
    assert recon.reconstruct_mesh_many([None, None], simplify=16) == [None, None]


def test_simplify_mesh_and_render(ops):
    """recon.simplify_mesh on a finished mesh, its vmap, and the rasteriser on the result (the pieces connect)."""
    from monoport_amd import recon
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    full = recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX)
    small, vmap = recon.simplify_mesh(full, 16, BMIN, BMAX)
    _same_mesh(small, recon.reconstruct_mesh(vol, 0.5, BMIN, BMAX, simplify=16), "simplify_mesh")
    want = ms.simplify_ref(full.verts.cpu().numpy(), full.faces.cpu().numpy(), 16)
    assert np.array_equal(vmap.cpu().numpy(), want[2]) and np.array_equal(_bits(small.verts), want[0].view(np.uint32))
    assert small.colors is None and small.normals.shape == small.verts.shape
    pair, vmap2 = recon.simplify_mesh((full.verts, full.faces), 16, normals=None)
    assert pair.normals is None and torch.equal(pair.faces, small.faces) and torch.equal(vmap2, vmap)
    assert recon.simplify_mesh(None, 16) == (None, None)
    empty, emap = recon.simplify_mesh((full.verts[:0], full.faces[:0]), 16)
    assert empty.verts.shape == (0, 3) and empty.faces.shape == (0, 3) and emap.shape == (0,)
    shot = recon.render_mesh(small, torch.eye(4, device=DEV), res=65, shade="normals")
    covered = int((shot.face >= 0).sum())
    print("simplified blob at 65 x 65: %d pixels covered" % covered)
    assert covered >= 1 and int(shot.face.max()) < small.faces.shape[0]


# ---- FrameSlot(mesh={"simplify": ...}) -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    import bench
    dev = torch.device(DEV)
    return bench.build_netg(dev)[0], bench.build_netc(dev)


@pytest.mark.parametrize("mesh_batch", [None, 2])
def test_slot_simplify(nets, mesh_batch, monkeypatch):
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

    plain, slot = make(normals="accumulate"), make(normals="accumulate", simplify=16, clean=6)
    try:
        assert slot.mesh._replace(simplify=None, clean=None) == plain.mesh
        assert slot.mesh.simplify == 16 and slot.mesh.clean == 6 and plain.mesh.simplify is None
        assert not any(k.startswith("simple_") for k in plain.mesh_buffers)
        assert slot.mesh_buffers["simple_verts"].shape == slot.mesh_buffers["verts"].shape
        with pytest.raises(ValueError):
            make(simplify=0)
        with pytest.raises(ValueError):
            make(simplfy=16)
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
        got, full = slot.meshes(), plain.meshes()
        assert [g is None for g in got] == [False, False, True, False, False]
        assert got[3].verts.shape == (0, 3) and got[3].faces.shape == (0, 3)
        assert slot.mesh_buffers["simple_counts"][2].cpu().tolist() == [0, 0]
        assert got[0].verts.data_ptr() == slot.mesh_buffers["simple_verts"].data_ptr()
        mlp_c = netc.surface_classifier.packed()
        for b in (0, 1, 3, 4):
            binding = QueryBinding(netc, mlp_c, slot.feats_hwc_c[b], slot.calib[b:b + 1], syn.Z_SCALE)
            opts = recon.mesh_options("accumulate", 0.5, True, clean=6, simplify=16)
            chain = recon._mesh_chains([slot.volumes[b]], BMIN, BMAX, opts, [binding])[0]
            nv, nf = chain.counts.cpu().tolist()
            _same_mesh(got[b], recon._finish_mesh(chain, nv, nf), "frame %d" % b)
            # geometry and normals: the public per-volume call on the slot's volume
            want = recon.reconstruct_mesh(slot.volumes[b], 0.5, BMIN, BMAX, clean=6, simplify=16)
            _same_mesh(got[b]._replace(colors=None), want, "frame %d, reconstruct_mesh" % b)
            assert got[b].verts.shape[0] <= full[b].verts.shape[0]
            # marching cubes' own mesh stays in the slot beside the simplified one
            assert slot.mesh_buffers["counts"][b, 0].item() >= got[b].verts.shape[0]
        assert got[0].verts.shape == (285, 3) and full[0].verts.shape == (1562, 3)
        assert float(got[4].verts.abs().max()) < 0.6 < float(full[4].verts.max())
        assert got[0].colors.shape == (285, 3) and not torch.equal(got[0].colors[:50], got[1].colors[:50])
        # the slot's capacities cut below the meshes: every non-empty frame comes from the re-run
        got = [g if g is None else type(g)(*[t.clone() for t in g]) for g in got]
        cut = {"verts": 100, "normals": 100, "simple_verts": 100, "faces": 200, "simple_faces": 200}
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = v[:, :cut[k]] if k in cut else v
        slot.mesh_buffers["simple_vmap"] = torch.zeros((5, 100), dtype=torch.int32, device=DEV)
        slot.mesh_buffers["points"] = torch.zeros((5, 3, 100), device=DEV)
        slot.mesh_buffers["preds"] = torch.zeros((5, 3, 100), device=DEV)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(5)
        slot._busy = True
        again = slot.meshes()
        for b in range(5):
            _same_mesh(again[b], got[b], "re-run, frame %d" % b)
    finally:
        slot.close()
        plain.close()
