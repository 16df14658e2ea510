"""mp_volume_keep_largest / mp_volume_keep_largest_batch (csrc/components.hip) through ctypes, and the ``clean``
option of recon.reconstruct_mesh, recon.reconstruct_mesh_many and FrameSlot(mesh=...), on the GPU.  The kernels are
held to the definition's numpy restatement (tests/keep_largest_ref.py, itself held to scipy in
tests/test_keep_largest_cpu.py): ``out`` bit for bit (as uint32, so NaNs compare), ``stats`` exactly.  Needs an
MI355X."""
import ctypes

import numpy as np
import pytest

import keep_largest_ref as kl
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
    from monoport_amd import _lib
    assert (_lib.load().mp_max_frames(), MP_ERR_ARG, MP_ERR_UNSUPPORTED) == (ops.MAX_FRAMES, _err("MP_ERR_ARG"),
                                                                             _err("MP_ERR_UNSUPPORTED"))
    ctx = ops.get_context(torch.device(DEV))
    return ctx.lib, ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _err(name):
    """The value of an MP_ERR_* code in include/monoport_hip.h."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "monoport_hip.h")).read()
    return int(re.search(r"\b%s\s*=\s*(-?\d+)" % name, text).group(1))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _pp(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _dev(vol):
    return torch.from_numpy(np.array(vol)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _single(abi, vol, connectivity, fill=0.0, level=kl.LEVEL, in_place=False):
    """One mp_volume_keep_largest call on a device volume -> (out tensor, stats list)."""
    lib, h, st = abi
    r = vol.shape[0]
    out = vol if in_place else torch.full_like(vol, POISON)
    stats = torch.full((4,), IPOISON, dtype=torch.int32, device=DEV)
    rc = lib.mp_volume_keep_largest(h, _p(vol), r, level, connectivity, fill, _p(out), _p(stats), st)
    assert rc == MP_OK, lib.mp_last_error(h).decode()
    return out, stats.cpu().tolist()


def _check_case(abi, name, connectivity, fill=0.0):
    vol = kl.volume(name)
    want, want_stats = kl.reference(name, connectivity, fill)
    src = _dev(vol)
    out, stats = _single(abi, src, connectivity, fill)
    print("%s, connectivity %d: stats %s (reference %s)" % (name, connectivity, stats, want_stats))
    assert stats == want_stats
    assert np.array_equal(_bits(out), want.view(np.uint32))
    assert np.array_equal(_bits(src), vol.view(np.uint32))  # the input is only read
    return out, stats


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", ["spheres33", "serpentine33", "equal_cubes17", "nan_bridge17", "empty17", "full17",
                                  "noise65", "body129"])
def test_against_the_definition(abi, name, connectivity):
    out, stats = _check_case(abi, name, connectivity)
    vol = kl.volume(name)
    if name in ("empty17", "full17"):
        assert np.array_equal(_bits(out), vol.view(np.uint32))
        assert stats == ([0, 0, 0, -1] if name == "empty17" else [17 ** 3, 1, 17 ** 3, 0])
    if name == "spheres33":  # the small sphere is filled, every other voxel keeps its bits
        changed = _bits(out) != vol.view(np.uint32)
        assert changed.sum() == stats[0] - stats[2] > 0 and (out.cpu().numpy()[changed] == 0.0).all()
        assert changed[24:31, 24:31, 24:31].sum() == changed.sum()
    if name == "equal_cubes17":
        assert stats[3] == (2 * 17 + 2) * 17 + 2
    if name == "serpentine33":
        assert stats[2] == 6935


@pytest.mark.parametrize("kind,directions", [("edge", kl.EDGE_DIRECTIONS), ("corner", kl.CORNER_DIRECTIONS),
                                             ("face", [(0, 0, 1), (0, -1, 0), (1, 0, 0)])])
def test_touching_cubes(abi, kind, directions):
    """Every direction two cubes can touch in: apart under 6 unless they share a face, one body under 26."""
    for d in directions:
        for connectivity in (6, 26):
            _, stats = _check_case(abi, d, connectivity)
            joined = kind == "face" or connectivity == 26
            assert stats[:3] == ([91, 1, 91] if joined else [91, 2, 64]), (d, connectivity)


def test_fill_value_and_level(abi):
    """A fill other than 0 (negative, and exactly the level), and a level other than 0.5."""
    for fill in (-1.5, kl.LEVEL):
        _check_case(abi, "spheres33", 6, fill)
    vol = kl.volume("body_floater33")
    want, want_stats = kl.keep_largest_ref(vol, 0.25, 26, 0.125)
    out, stats = _single(abi, _dev(vol), 26, 0.125, level=0.25)
    assert stats == want_stats and np.array_equal(_bits(out), want.view(np.uint32))


@pytest.mark.parametrize("name,connectivity", [("spheres33", 6), ("noise65", 26), ("empty17", 6)])
def test_in_place(abi, name, connectivity):
    want, want_stats = kl.reference(name, connectivity)
    src = _dev(kl.volume(name))
    out, stats = _single(abi, src, connectivity, in_place=True)
    assert out.data_ptr() == src.data_ptr() and stats == want_stats
    assert np.array_equal(_bits(src), want.view(np.uint32))


def test_unaligned_volume(abi):
    """Volumes that start 4 bytes past a 16-byte boundary take the scalar path of the vector kernels."""
    vol = kl.volume("spheres33")
    want, want_stats = kl.reference("spheres33", 6)
    n = vol.size
    src = torch.zeros(n + 4, device=DEV)
    dst = torch.full((n + 8,), POISON, device=DEV)
    src[1:n + 1] = _dev(vol).reshape(-1)
    lib, h, st = abi
    stats = torch.zeros(4, dtype=torch.int32, device=DEV)
    a, b = src[1:n + 1], dst[3:n + 3]
    assert a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 12
    assert lib.mp_volume_keep_largest(h, _p(a), 33, kl.LEVEL, 6, 0.0, _p(b), _p(stats), st) == MP_OK
    assert stats.cpu().tolist() == want_stats and np.array_equal(_bits(b), want.view(np.uint32).reshape(-1))
    assert (dst[:3] == POISON).all() and (dst[n + 3:] == POISON).all()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_repeatable(abi, connectivity):
    src = _dev(kl.volume("noise65"))
    first, stats1 = _single(abi, src, connectivity)
    second, stats2 = _single(abi, src, connectivity)
    assert stats1 == stats2 == kl.reference("noise65", connectivity)[1]
    assert np.array_equal(_bits(first), _bits(second))


def _batch(abi, vols, connectivity, gates=None, n=None, r=None, level=kl.LEVEL, fill=0.0, outs=None, stats=None):
    lib, h, st = abi
    n = len(vols) if n is None else n
    r = vols[0].shape[0] if r is None else r
    if outs is None:
        outs = [torch.full_like(v, POISON) for v in vols]
    if stats is None:
        stats = [torch.full((4,), IPOISON, dtype=torch.int32, device=DEV) for _ in vols]
    rc = lib.mp_volume_keep_largest_batch(h, n, _pp(vols), r, level, connectivity, fill, _pp(outs), _pp(stats),
                                          None if gates is None else _pp(gates), st)
    return rc, outs, stats, lib.mp_last_error(h).decode()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_batch_equals_single_calls(abi, connectivity):
    """Floaters / gated off (its output poisoned before: it must stay poisoned, and its volume is never read) /
    empty / a second body, with gates given as NULL, 1 and 0."""
    names = ["spheres33", "serpentine33", None, "body_floater33"]
    vols = [_dev(kl.volume(n)) if n else torch.zeros((33, 33, 33), device=DEV) for n in names]
    vols[1] = torch.full((33, 33, 33), float("nan"), device=DEV)  # "unspecified": gated off below
    on, off = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    rc, outs, stats, msg = _batch(abi, vols, connectivity, gates=[None, off, on, on])
    assert rc == MP_OK, msg
    for f in (0, 2, 3):
        want, want_stats = _single(abi, vols[f], connectivity)
        assert stats[f].cpu().tolist() == want_stats, f
        assert np.array_equal(_bits(outs[f]), _bits(want)), f
    assert stats[1].cpu().tolist() == [0, 0, 0, -1] and (outs[1] == POISON).all()
    assert stats[2].cpu().tolist() == [0, 0, 0, -1] and np.array_equal(_bits(outs[2]), _bits(vols[2]))
    assert stats[0].cpu().tolist() == kl.reference("spheres33", connectivity)[1]
    # without gates every frame is on
    rc, outs2, stats2, msg = _batch(abi, vols, connectivity)
    assert rc == MP_OK, msg
    assert stats2[1].cpu().tolist() == [0, 0, 0, -1] and np.array_equal(_bits(outs2[1]), _bits(vols[1]))
    assert np.array_equal(_bits(outs2[3]), _bits(outs[3]))


def test_refusals(abi, ops):
    lib, h, st = abi
    vols = [_dev(kl.volume("equal_cubes17"))]
    most = lib.mp_max_frames()
    many = vols * (most + 1)

    def refused(code, text, **kw):
        args = dict(vols=vols, connectivity=6)
        args.update(kw)
        rc, outs, stats, msg = _batch(abi, **args)
        assert rc == code and text in msg and msg, (rc, msg)
        assert all((o == POISON).all() for o in outs if o is not None) and all((s == IPOISON).all() for s in stats)

    refused(MP_ERR_ARG, "1..%d frames per call, got %d" % (most, most + 1), vols=many)
    refused(MP_ERR_ARG, "frames per call, got 0", n=0)
    refused(MP_ERR_ARG, "connectivity", connectivity=18)
    refused(MP_ERR_ARG, "fill", fill=0.75)
    refused(MP_ERR_ARG, "fill", fill=float("nan"))
    refused(MP_ERR_UNSUPPORTED, "64-bit", r=1291)
    two = vols * 2
    good = [torch.full_like(vols[0], POISON) for _ in two]
    refused(MP_ERR_ARG, "null buffer for frame 1", vols=two, outs=[good[0], None])
    refused(MP_ERR_ARG, "null buffer for frame 1", vols=[vols[0], None], outs=good)
    bytes_ = torch.zeros(17 ** 3 * 4 + 8, dtype=torch.uint8, device=DEV)
    odd = bytes_[2:2 + 17 ** 3 * 4]
    assert odd.data_ptr() % 4 == 2
    refused(MP_ERR_ARG, "misaligned buffer for frame 1", vols=[vols[0], odd], outs=good)
    gate_bytes = torch.zeros(8, dtype=torch.uint8, device=DEV)
    refused(MP_ERR_ARG, "misaligned buffer for frame 0", gates=[gate_bytes[1:5]])
    # the single call shares the checks
    stats = torch.full((4,), IPOISON, dtype=torch.int32, device=DEV)
    out = torch.full_like(vols[0], POISON)
    for conn, fill, r, code in ((5, 0.0, 17, MP_ERR_ARG), (6, 1.0, 17, MP_ERR_ARG), (26, float("nan"), 17, MP_ERR_ARG),
                                (6, 0.0, 1291, MP_ERR_UNSUPPORTED)):
        assert lib.mp_volume_keep_largest(h, _p(vols[0]), r, kl.LEVEL, conn, fill, _p(out), _p(stats), st) == code
        assert lib.mp_last_error(h).decode()
    assert lib.mp_volume_keep_largest(h, None, 17, kl.LEVEL, 6, 0.0, _p(out), _p(stats), st) == MP_ERR_ARG
    assert (out == POISON).all() and (stats == IPOISON).all()
    # the wrappers refuse the same before they call
    for kw in (dict(connectivity=18), dict(fill=0.75), dict(fill=float("nan"))):
        with pytest.raises(ValueError):
            ops.keep_largest_raw(vols[0], kl.LEVEL, **kw)


# ---- Python layers ------------------------------------------------------------------------------------------------

def test_ops_and_recon_wrappers(abi, ops):
    from monoport_amd import recon
    vols = [_dev(kl.volume(n)) for n in ("spheres33", "body_floater33")]
    for connectivity in (6, 26):
        singles = [_single(abi, v, connectivity) for v in vols]
        for v, (want, want_stats) in zip(vols, singles):
            out, stats = ops.keep_largest_raw(v, kl.LEVEL, connectivity, 0.0)
            assert stats.cpu().tolist() == want_stats and np.array_equal(_bits(out), _bits(want))
            got = recon.keep_largest(v[None, None], connectivity=connectivity)
            assert got.shape == (1, 1, 33, 33, 33) and np.array_equal(_bits(got[0, 0]), _bits(want))
            assert recon.keep_largest(v, connectivity=connectivity).shape == (33, 33, 33)
        on, off = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        batch = ops.keep_largest_raw_batch(vols, kl.LEVEL, connectivity, 0.0, gates=[on, None])
        for (out, stats), (want, want_stats) in zip(batch, singles):
            assert stats.cpu().tolist() == want_stats and np.array_equal(_bits(out), _bits(want))
        assert ops.keep_largest_raw_batch(vols, gates=[off, on])[0][1].cpu().tolist() == [0, 0, 0, -1]
        many = recon.keep_largest_many([vols[0][None, None], None, vols[1]], connectivity=connectivity)
        assert many[1] is None and many[0].shape == (1, 1, 33, 33, 33) and many[2].shape == (33, 33, 33)
        assert np.array_equal(_bits(many[0][0, 0]), _bits(singles[0][0]))
        assert np.array_equal(_bits(many[2]), _bits(singles[1][0]))
    assert recon.keep_largest(None) is None and recon.keep_largest_many([None]) == [None]
    src = vols[0].clone()
    out, _ = ops.keep_largest_raw(src, out=src)
    assert out.data_ptr() == src.data_ptr() and np.array_equal(_bits(src), kl.reference("spheres33", 6)[0].view(np.uint32))


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


def test_reconstruct_mesh_clean(colour):
    from monoport_amd import recon
    net, feats, calibs = colour
    both = _dev(kl.volume("body_floater33"))[None, None]
    before = both.clone()
    one = _dev(syn.sphere_volume(33))[None, None]
    kw = dict(netC=net, feat_tensor_C=feats[0], calib_tensor=calibs[0])
    for clean in (6, 26):
        got = recon.reconstruct_mesh(both, 0.5, BMIN, BMAX, clean=clean, **kw)
        _same_mesh(got, recon.reconstruct_mesh(recon.keep_largest(both, 0.5, clean), 0.5, BMIN, BMAX, **kw), "clean")
        assert torch.equal(both, before)  # the caller's volume is not modified
        # one body: nothing to drop
        _same_mesh(recon.reconstruct_mesh(one, 0.5, BMIN, BMAX, clean=clean, **kw),
                   recon.reconstruct_mesh(one, 0.5, BMIN, BMAX, **kw), "single component")
    dirty = recon.reconstruct_mesh(both, 0.5, BMIN, BMAX, **kw)
    print("33^3 body + floater: %d vertices, %d with clean=6" % (dirty.verts.shape[0], got.verts.shape[0]))
    assert 100 < got.verts.shape[0] < dirty.verts.shape[0] and got.faces.shape[0] < dirty.faces.shape[0]
    # the body is the sphere of radius 0.5 about the origin: no vertex of the floater at (0.75, 0.75, 0.75) is left
    assert float(got.verts.abs().max()) < 0.6 and float(dirty.verts.max()) > 0.7
    assert got.colors.shape == got.verts.shape and got.normals.shape == got.verts.shape
    _same_mesh(recon.reconstruct_mesh(both, 0.5, BMIN, BMAX, normals=None, clean=6),
               recon.reconstruct_mesh(recon.keep_largest(both), 0.5, BMIN, BMAX, normals=None), "no colours")
    for bad in (dict(clean=6, level=0), dict(clean=6, level=-0.5), dict(clean=5), dict(clean=True)):
        with pytest.raises(ValueError):
            recon.reconstruct_mesh(both, **{"level": 0.5, **bad})
        with pytest.raises(ValueError):
            recon.reconstruct_mesh_many([both], **{"level": 0.5, **bad})
    assert recon.reconstruct_mesh(None, clean=6) is None


def test_reconstruct_mesh_many_clean(colour):
    from monoport_amd import recon
    net, feats, calibs = colour
    sdfs = [_dev(kl.volume("body_floater33"))[None, None], None, _dev(syn.blob_volume(33, 5)),
            torch.zeros((33, 33, 33), device=DEV)]
    feats4, calibs4 = [feats[0], None, feats[1], feats[2]], [calibs[0], None, calibs[1], calibs[2]]
    for clean in (6, 26):
        got = recon.reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, netC=net, feat_tensors_C=feats4,
                                          calib_tensors=calibs4, clean=clean)
        assert got[1] is None and got[3].verts.shape[0] == 0
        for i in (0, 2, 3):
            _same_mesh(got[i], recon.reconstruct_mesh(sdfs[i], 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feats4[i],
                                                      calib_tensor=calibs4[i], clean=clean), "frame %d" % i)
    plain = recon.reconstruct_mesh_many(sdfs, 0.5, BMIN, BMAX, normals="reference")
    assert got[0].verts.shape[0] < plain[0].verts.shape[0]


# ---- FrameSlot(mesh={"clean": ...}) --------------------------------------------------------------------------------

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


def _binding(nets, slot, b):
    from monoport_amd.modeling.MonoPortNet import QueryBinding
    return QueryBinding(nets[1], nets[1].surface_classifier.packed(), slot.feats_hwc_c[b], slot.calib[b:b + 1],
                        syn.Z_SCALE)


def test_slot_clean(nets, ops):
    """Two frames of the synthetic body from two cameras, and a third whose camera looks past the box (its coarsest
    level is empty, its volume unspecified: gated off on the device)."""
    from monoport_amd.recon import _finish_mesh, _mesh_chains, mesh_options, pifu_calib
    images = torch.stack([torch.from_numpy(syn.synthetic_image(k)) for k in range(3)]).to(DEV)
    away = torch.eye(4, device=DEV)[None]
    away[0, 0, 3] = 5.0
    calibs = [pifu_calib(*syn.scene_camera(0), device=DEV), pifu_calib(*syn.scene_camera(40), device=DEV), away]
    plain = _slot(nets, 3, (17, 33, 65), mesh={"normals": "accumulate"})
    slot = _slot(nets, 3, (17, 33, 65), mesh={"normals": "accumulate", "clean": 6})
    try:
        # the option is a field of the slot's record; without it nothing is allocated
        assert slot.mesh._replace(clean=None) == plain.mesh and tuple(plain.mesh[:3]) == ("accumulate", 0.5, True)
        assert slot.mesh.clean == 6 and plain.mesh.clean is None
        assert "cleaned" not in plain.mesh_buffers and "clean_stats" not in plain.mesh_buffers
        assert slot.mesh_buffers["cleaned"].shape == (3, 65, 65, 65)
        for s in (plain, slot):
            s.submit(images, calibs)
        got, want_plain = slot.meshes(), plain.meshes()
        assert slot.status[:, 0].cpu().tolist() == [1, 1, 0] and got[2] is None and want_plain[2] is None
        # every other consumer sees the unchanged volume
        for b in range(2):
            assert torch.equal(_bits_t(slot.volumes[b]), _bits_t(plain.volumes[b]))
            assert torch.equal(slot.renders[b], plain.renders[b]) and torch.equal(slot.renders_tex[b], plain.renders_tex[b])
        assert slot.mesh_buffers["clean_stats"][2].cpu().tolist() == [0, 0, 0, -1]
        for b in range(2):
            chain = _mesh_chains([slot.volumes[b]], BMIN, BMAX, mesh_options("accumulate", 0.5, True, clean=6),
                                 [_binding(nets, slot, b)])[0]
            nv, nf = chain.counts.cpu().tolist()
            _same_mesh(got[b], _finish_mesh(chain, nv, nf), "frame %d" % b)
            stats = slot.mesh_buffers["clean_stats"][b].cpu().tolist()
            assert stats == ops.keep_largest_raw(slot.volumes[b], 0.5, 6, 0.0)[1].cpu().tolist() and stats[2] > 1000
            if stats[1] == 1:  # one body: the mesh of the slot without the option
                _same_mesh(got[b], want_plain[b], "frame %d, one component" % b)
        # a floater planted into frame 0's volume: the chain on the slot's buffers drops it, the plain chain meshes it
        stats0 = slot.mesh_buffers["clean_stats"][0].cpu().tolist()
        got = [g if g is None else type(g)(*[t.clone() for t in g]) for g in got]  # views of the slot's buffers
        for s in (plain, slot):
            with torch.cuda.stream(s.stream):
                s.volumes[0][2:5, 2:5, 2:5] = 0.9
                s._mesh_chain(3)
            s._busy = True
        got2, plain2 = slot.meshes(), plain.meshes()
        _same_mesh(got2[0], got[0], "floater dropped")
        _same_mesh(got2[1], got[1], "frame 1 again")
        assert plain2[0].verts.shape[0] > got2[0].verts.shape[0] and float(plain2[0].verts.min()) < -0.85
        assert float(slot.volumes[0][3, 3, 3]) == np.float32(0.9)
        assert slot.mesh_buffers["clean_stats"][0].cpu().tolist() == [stats0[0] + 27, stats0[1] + 1] + stats0[2:]
    finally:
        slot.close()
        plain.close()


def _bits_t(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("mesh_batch", [2, None])
def test_slot_clean_chunks(nets, ops, mesh_batch, monkeypatch):
    """Five frames, the volumes filled in by hand (a floater, one body, a gated-off frame of NaNs, an empty volume,
    noise), in chunks of 2 + 2 + 1 frames and in one: the cleaned copies live in ONE chunk's buffer."""
    from monoport_amd import pipeline
    from monoport_amd.recon import _finish_mesh, _mesh_chains, mesh_options
    if mesh_batch is not None:
        monkeypatch.setattr(pipeline, "MESH_BATCH", mesh_batch)
    vols = [_dev(kl.volume("body_floater33")), _dev(syn.sphere_volume(33)), torch.full((33, 33, 33), float("nan"), device=DEV),
            torch.zeros((33, 33, 33), device=DEV), _dev(kl.volume("spheres33"))]
    slot = _slot(nets, 5, (17, 33), mesh={"normals": "reference", "colors": False, "clean": 26})
    try:
        assert slot.mesh_buffers["cleaned"].shape[0] == (5 if mesh_batch is None else mesh_batch)
        torch.cuda.synchronize()
        with torch.cuda.stream(slot.stream):
            for b, v in enumerate(vols):
                slot.volumes[b].copy_(v)
            slot.status.zero_()
            slot.status[:, 0] = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32)
            slot.n_active = 5
            slot._mesh_chain(5)
        slot._busy = True
        got = slot.meshes()
        assert got[2] is None and got[3].verts.shape[0] == 0
        for b in (0, 1, 3, 4):
            chain = _mesh_chains([vols[b]], BMIN, BMAX, mesh_options("reference", 0.5, clean=26))[0]
            nv, nf = chain.counts.cpu().tolist()
            _same_mesh(got[b], _finish_mesh(chain, nv, nf), "frame %d" % b)
            assert torch.equal(_bits_t(slot.volumes[b]), _bits_t(vols[b]))
        assert [slot.mesh_buffers["clean_stats"][b].cpu().tolist() for b in (0, 2, 3)] == [
            kl.reference("body_floater33", 26)[1], [0, 0, 0, -1], [0, 0, 0, -1]]
    finally:
        slot.close()
