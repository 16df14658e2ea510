"""Every stage that takes temporary memory from the per-stream scratch arena (ensure_scratch, csrc/api.hip), run on a
DIRTY arena.  In production the stages run back to back on one stream, so each starts on the bytes another stage left;
a test that calls one stage sees a fresh hipMalloc or the residue of whatever test ran before it, and the arena pointer
never leaves the library.  mp_scratch_fill (a test hook) fills the whole block with one byte first; DESIGN.md section
4.8.6 lists, region by region, what establishes every word before it is read -- these tests confirm that reading.

Per stage and per fill byte (scratch_cases.FILLS):
  (a) the result equals the stage's existing reference -- the numpy restatements, the CPU oracle, float64 -- with the
      comparison and the bar of the stage's own test module (imported from there where it is a function);
  (b) the four fills give the same bits (every stage here is defined bit for bit; of the top-k selection the SET: the
      order of its list is unspecified);
  (c) the outputs go into poisoned buffers and the rows behind the counts keep the poison;
  (d) the call stayed inside the filled block: mp_memory_stats reads the same before and after it.
Each call runs on a private stream, released afterwards, so the arenas of the rest of the suite stay as they are.
Needs an MI355X."""
import functools

import numpy as np
import pytest

import elementwise_ref as er
import keep_largest_ref as kl
import mesh_render_ref as render_ref
import mesh_simplify_ref as ms
import mesh_smooth_ref as sm
import octree_ref
import scratch_cases as cases
import surface_cases as sc
import topk_ref
from conftest import load_golden
from monoport_amd import synthetic as syn
from test_box_threshold_cpu import B_MAX, B_MIN
from test_gn_offset_gpu import _consumer_input as gn_input, _gn as gn_module
from test_mesh_gpu import expected as normals_expected, mesh_of as normals_mesh
from test_mesh_render_gpu import PREDS, NORMALS, _cameras, assert_same as render_same, projected, soup as render_soup
from test_mesh_simplify_gpu import _check as simplify_check
from test_mesh_smooth_gpu import _check as smooth_check
from test_recon_views_gpu import _abi_inputs as views_inputs
from test_surface_cases_gpu import capacities, check_mesh, check_rows, cut, oracle_rows
from test_topk_gpu import _reference as topk_reference, _tie_run

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
POISON, IPOISON = -12345.0, -777  # the values the imported checks look for behind the counts
RES = cases.RES
fills = pytest.mark.parametrize("byte", cases.FILLS, ids=cases.FILL_IDS)


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


# ---- the helper every stage goes through ------------------------------------------------------------------------
def on_dirty_arena(ops, byte, op, role="query"):
    """``op()`` on a private stream whose scratch arena (of the ``role`` context) is one block of cases.ARENA_BYTES or
    more, every byte of it ``byte``.  Asserts that the contexts own the same arenas of the same size after ``op`` as
    before it: the stage worked inside the filled block, on the stream that was filled.  Returns ``op``'s result,
    complete (the stream is drained)."""
    dev = torch.device(DEV)
    torch.cuda.synchronize(dev)  # the inputs were made on the default stream
    stream = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(stream):
            block = ops.scratch_fill(dev, cases.ARENA_BYTES, byte, role)
            before = ops.memory_stats(dev)
            out = op()
            after = ops.memory_stats(dev)
        stream.synchronize()
    finally:
        ops.stream_release(stream)
    assert block >= cases.ARENA_BYTES, block
    assert (after["arena_bytes"], after["arenas"]) == (before["arena_bytes"], before["arenas"]), \
        "the stage left the filled block: %s -> %s" % (before, after)
    return out


def _host(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


_FIRST = {}


def agree(key, byte, *outputs):
    """(b): the outputs of this fill (whole buffers, poison included) have the bits of the first fill that ran."""
    got = [_host(t) for t in outputs]
    first_byte, first = _FIRST.setdefault(key, (byte, got))
    for k, (a, b) in enumerate(zip(first, got)):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), \
            "%s: output %d under fill 0x%02X differs from fill 0x%02X" % (key, k, byte, first_byte)


def full(shape, value, dtype=None):
    return torch.full(shape, value, dtype=dtype or torch.float32, device=DEV)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared cases are read-only


def test_fill_reports_the_block_and_refuses(ops):
    """The hook itself: it reports the whole block (which a smaller request does not shrink), refuses what the header
    says it refuses, and the fills of two roles are two arenas."""
    from monoport_amd._lib import MonoportError
    d = torch.device(DEV)
    stream = torch.cuda.Stream(d)
    ops.stream_release(stream)  # torch hands its streams out of a pool: no arena of an earlier user of this one
    try:
        with torch.cuda.stream(stream):
            base = ops.memory_stats(d)
            a = ops.scratch_fill(d, 1 << 20, 0x5A)
            assert a >= 1 << 20 and a % 65536 == 0
            assert ops.scratch_fill(d, 0, 0xFF) == a and ops.scratch_fill(d, 4096, 0) == a
            one = ops.memory_stats(d)
            assert (one["arena_bytes"], one["arenas"]) == (base["arena_bytes"] + a, base["arenas"] + 1)
            b = ops.scratch_fill(d, 4096, 0x7F, role="encoder")
            two = ops.memory_stats(d)
            assert (two["arena_bytes"], two["arenas"]) == (one["arena_bytes"] + b, one["arenas"] + 1)
            for bad in ((-1, 0), (16, -1), (16, 256)):
                with pytest.raises(MonoportError, match="mp_scratch_fill"):
                    ops.scratch_fill(d, *bad)
            with pytest.raises(ValueError):
                ops.scratch_fill(d, 16, 0, role="mesh")
            assert ops.memory_stats(d) == two
    finally:
        ops.stream_release(stream)
    assert ops.memory_stats(d) == base


# ---- the fused reconstruction ----------------------------------------------------------------------------------
def _gpu_query(ops, mlp, fh, cal):
    def gpu_query(pts):  # [3,N] numpy -> [N] numpy through the HIP query kernel
        out = ops.query(mlp, fh, torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV), cal, syn.Z_SCALE)
        return out[0, 0].cpu().numpy()
    return gpu_query


@pytest.fixture(scope="module")
def scene(ops, oracle):
    """The f32 body head of tests/test_recon_gpu.py on three frames with their own maps and cameras; frame 1 looks past
    the box.  ``lossless[f]`` = (volume or None, points per level) of the CPU driver fed by the same HIP query kernel,
    computed once on the default stream."""
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    feats, cals, queries, lossless = [], [], [], []
    for i in range(3):
        feats.append(ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2 + i))[None].to(DEV)))
        calib = oracle.pifu_calib(*syn.scene_camera(30 + 25 * i))
        if i == 1:
            calib[0, 0, 3] = 5.0
        cals.append(torch.from_numpy(calib).to(DEV))
        queries.append(_gpu_query(ops, mlp, feats[i], cals[i]))
        stats = []
        lossless.append((oracle.seg3d_lossless(queries[i], BMIN, BMAX, RES, stats=stats), stats))
    assert lossless[1][0] is None and lossless[0][0] is not None and lossless[2][0] is not None
    assert all(s > 0 for s in lossless[0][1] + lossless[2][1])
    return dict(mlp=mlp, feats=feats, cals=cals, queries=queries, lossless=lossless, topk={})


@fills
@pytest.mark.parametrize("frames", [(0,), (0, 1, 2)], ids=["1frame", "3frames"])
def test_recon_batch(ops, scene, frames, byte):
    """Level volumes, boundary and evaluated bitmaps (r = 9, 17, 33: most bits of a row's last word are padding) and
    the point list, carved per frame out of the dirt; the frame that looks past the box between two live ones."""
    n = len(frames)

    def op():
        volumes = [full((RES[-1],) * 3, POISON) for _ in frames]
        status = full((n, 1 + len(RES)), IPOISON, torch.int32)
        return ops.recon_batch(scene["mlp"], [scene["feats"][f] for f in frames], [scene["cals"][f] for f in frames],
                               syn.Z_SCALE, BMIN, BMAX, RES, volumes=volumes, status=status)

    volumes, status = on_dirty_arena(ops, byte, op)
    st = status.cpu().numpy()
    for k, f in enumerate(frames):
        ref, stats = scene["lossless"][f]
        if ref is None:
            assert st[k].tolist() == [0, RES[0] ** 3, 0, 0], f
        else:
            assert st[k].tolist() == [1] + stats, f
            assert np.array_equal(volumes[k].cpu().numpy(), ref), f
    agree(("recon", frames), byte, status, *volumes)


@fills
def test_recon_topk_batch(ops, scene, byte):
    """The lossless carve of two frames with the top-k header, histograms and tie arrays behind it; budgets of a
    quarter of the lossless counts (tests/test_topk_gpu.py), so every level cuts inside its candidates."""
    frames = (0, 2)
    budgets = [0] + [max(s // 4, 1) for s in scene["lossless"][0][1][1:]]
    for f in frames:
        if f not in scene["topk"]:
            stats = []
            scene["topk"][f] = (topk_ref.seg3d_topk(scene["queries"][f], BMIN, BMAX, RES, budgets, None, stats=stats),
                                stats)

    def op():
        volumes = [full((RES[-1],) * 3, POISON) for _ in frames]
        status = full((len(frames), 1 + len(RES)), IPOISON, torch.int32)
        return ops.recon_topk_batch(scene["mlp"], [scene["feats"][f] for f in frames],
                                    [scene["cals"][f] for f in frames], syn.Z_SCALE, BMIN, BMAX, RES, budgets,
                                    volumes=volumes, status=status)

    volumes, status = on_dirty_arena(ops, byte, op)
    st = status.cpu().numpy()
    for k, f in enumerate(frames):
        ref, stats = scene["topk"][f]
        assert st[k].tolist() == [1] + stats and all(s > 0 for s in stats), (f, st[k].tolist(), stats)
        assert np.array_equal(volumes[k].cpu().numpy().view(np.uint32), ref.view(np.uint32)), f
    agree("recon_topk", byte, status, *volumes)


@functools.lru_cache(maxsize=None)
def _select_case():
    """9 -> 17 on octree_ref.plateau: 40 % of the nodes exactly on the threshold (u == 0: one long run of ties) next to
    nodes one ulp above it.  Budgets: inside the run (the ties are ranked: tie counts and their scan), and more than
    there are candidates (no ranking at all: the tie arrays stay dirt and must stay unread)."""
    prev, ev_prev = octree_ref.plateau(9, 11)
    n_cand, start, end = _tie_run(prev, ev_prev)
    assert end - start > 50 and n_cand + 7 <= 17 ** 3
    ks = ((start + end) // 2, n_cand + 7)
    return prev, ev_prev, ks, [topk_reference(prev, ev_prev, k) for k in ks]


@fills
def test_octree_select_topk(ops, byte):
    prev, ev_prev, ks, wants = _select_case()
    rp, r = 9, 17
    words = r * r * ((r + 63) // 64)
    ctx = ops.get_context(torch.device(DEV))
    d_prev = dev(prev)
    d_evp = torch.from_numpy(octree_ref.pack_bits(ev_prev).view(np.int64)).to(DEV)

    def op():
        outs = []
        for k in ks:
            cur = full((r, r, r), POISON)
            ev_cur = full((words,), IPOISON, torch.int64)
            packed = full((r ** 3,), IPOISON, torch.int32)
            count = full((1,), IPOISON, torch.int32)
            ctx.check(ctx.lib.mp_octree_select_topk(
                ctx.handle, ops._ptr(d_prev), rp, ops._ptr(cur), r, ops._ptr(d_evp), ops._ptr(ev_cur), int(k),
                float("inf"), 0.5, ops._ptr(packed), ops._ptr(count), ops._stream(cur)), "mp_octree_select_topk")
            outs.append((cur, ev_cur, packed, count))
        return outs

    flat = []
    for k, want, (cur, ev_cur, packed, count) in zip(ks, wants, on_dirty_arena(ops, byte, op)):
        n = int(count.item())
        packed = packed.cpu().numpy()
        assert 0 <= n <= r ** 3 and (packed[n:] == IPOISON).all(), k  # nothing is written behind the count
        codes = np.sort(packed[:n].astype(np.int64))
        assert np.array_equal(codes, want[2]), k
        assert np.array_equal(cur.cpu().numpy().view(np.uint32), want[0]), k
        assert np.array_equal(ev_cur.cpu().numpy().view(np.uint64), want[1]), k
        flat += [cur, ev_cur, codes, count]
    assert len(wants[0][2]) == ks[0] and len(wants[1][2]) == ks[1] - 7
    agree("select_topk", byte, *flat)


@pytest.fixture(scope="module")
def views(ops):
    """Two views of the multi-view body scene of tests/test_recon_views_gpu.py and the level-at-a-time engine's volume
    and counts on them (ops.recon_generic keeps its bitmaps in tensors of its own, not in the arena)."""
    mlp, fh, calibs = views_inputs(ops, 2)

    def query_func(points):
        pts = points[0].t()[None].expand(2, 3, points.shape[1])
        return ops.query_views(mlp, fh, pts, calibs, "orthogonal", syn.Z_SCALE)[:1]

    gen, counts = ops.recon_generic(query_func, {}, DEV, BMIN, BMAX, RES)
    assert gen is not None and counts[-1] > 0
    return dict(mlp=mlp, fh=fh, calibs=calibs, gen=gen, counts=counts)


@fills
def test_recon_views(ops, views, byte):
    vol, st = on_dirty_arena(ops, byte, lambda: ops.recon_views(views["mlp"], views["fh"], views["calibs"], "orthogonal",
                                                                syn.Z_SCALE, BMIN, BMAX, RES))
    assert st.tolist() == [1] + views["counts"]
    assert torch.equal(vol, views["gen"])
    agree("recon_views", byte, st, vol)


# ---- forward_vertices and marching cubes -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _depth33():
    vol = sc.depth_case(33, "smooth")[0]
    vol.setflags(write=False)
    return vol


@fills
def test_forward_vertices_batch(ops, oracle, byte):
    """r = 33 (two scan segments per column, two emit blocks), the four directions back to back, an empty volume as
    frame 1.  The hit map must read kNoHit where no segment found a hit, whatever lay there."""
    vols = [dev(_depth33()), torch.zeros((33, 33, 33), device=DEV)]
    n, r, cap = 2, 33, 33 * 33
    ctx = ops.get_context(torch.device(DEV))

    def op():
        outs = {}
        for direction in sc.DIRECTIONS:
            x, y = full((n, cap), IPOISON, torch.int64), full((n, cap), IPOISON, torch.int64)
            z, nrm = full((n, cap), POISON), full((n, cap, 3), POISON)
            count = full((n, 1), IPOISON, torch.int32)
            ctx.check(ctx.lib.mp_forward_vertices_batch(
                ctx.handle, n, ops._ptr_array(vols), r, ops.DIRECTIONS[direction], ops._ptr_array(x),
                ops._ptr_array(y), ops._ptr_array(z), ops._ptr_array(nrm), ops._ptr_array(count), ops._stream(x)),
                "mp_forward_vertices_batch")
            outs[direction] = (x, y, z, nrm, count)
        return outs

    outs = on_dirty_arena(ops, byte, op)
    for direction, (x, y, z, nrm, count) in outs.items():
        c = check_rows((x[0], y[0], z[0], nrm[0], count[0]), oracle_rows(oracle, _depth33(), direction), direction)
        assert c > 500
        assert (x[0, c:] == IPOISON).all() and (y[0, c:] == IPOISON).all()
        assert (z[0, c:] == POISON).all() and (nrm[0, c:] == POISON).all()
        assert int(count[1].item()) == 0 and (x[1] == IPOISON).all() and (z[1] == POISON).all()
        assert (y[1] == IPOISON).all() and (nrm[1] == POISON).all()
        agree(("forward_vertices", direction), byte, x, y, z, nrm, count)


@functools.lru_cache(maxsize=None)
def _mc_references(oracle):
    quarters = sc.quarters_volume(*sc.QUARTERS)  # r = 17: values in {0, .25, .5, .75, 1}, crossings on every border
    nonfinite = sc.nonfinite_volume(17, sc.NONFINITE[1])
    assert (quarters == np.float32(0.5)).sum() > 900
    assert np.isnan(nonfinite).sum() > 50 and np.isposinf(nonfinite).sum() > 50 and np.isneginf(nonfinite).sum() > 50
    with np.errstate(invalid="ignore", divide="ignore"):
        return (quarters, oracle.marching_cubes(quarters, 0.5, B_MIN, B_MAX),
                nonfinite, oracle.marching_cubes(nonfinite, 0.5, B_MIN, B_MAX))


@fills
def test_marching_cubes_batch(ops, oracle, byte):
    """r = 17, three frames: nodes exactly at the level / gated off (its volume is NaN and never read) / empty; then,
    on what that call left, a volume with NaN and +-inf nodes.  vbase[n] is written for nodes with a crossing flag
    only and read for owners of crossing edges only: no face may name a vertex that is not there."""
    quarters, want_q, nonfinite, want_n = _mc_references(oracle)
    max_v, max_f = capacities(17)
    vols = [dev(quarters), full((17, 17, 17), float("nan")), torch.zeros((17, 17, 17), device=DEV)]
    gates = [None, torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)]
    d_nonfinite = dev(nonfinite)

    def op():
        out3 = (full((3, max_v, 3), POISON), full((3, max_f, 3), IPOISON, torch.int32), full((3, 2), IPOISON, torch.int32))
        out1 = (full((1, max_v, 3), POISON), full((1, max_f, 3), IPOISON, torch.int32), full((1, 2), IPOISON, torch.int32))
        ops.marching_cubes_raw_batch(vols, 0.5, B_MIN, B_MAX, gates=gates, out=out3)
        ops.marching_cubes_raw_batch([d_nonfinite], 0.5, B_MIN, B_MAX, out=out1)
        return out3, out1

    out3, out1 = on_dirty_arena(ops, byte, op)
    for (verts, faces, counts), k, want, what in ((out3, 0, want_q, "quarters17"), (out1, 0, want_n, "nonfinite17")):
        check_mesh(cut((verts[k], faces[k], counts[k])), want, what)
        nv, nf = counts[k].cpu().tolist()
        assert nv > 1000 and nf > 1000, (what, nv, nf)
        f = faces[k, :nf]
        assert bool((f >= 0).all()) and bool((f < nv).all()), what  # every face index < counts[0]
        assert (verts[k, nv:] == POISON).all() and (faces[k, nf:] == IPOISON).all(), what
    for k in (1, 2):  # gated off, empty
        assert out3[2][k].cpu().tolist() == [0, 0], k
        assert (out3[0][k] == POISON).all() and (out3[1][k] == IPOISON).all(), k
    agree("marching_cubes", byte, *out3, *out1)


# ---- the mesh stages ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _normals_case():
    """Two meshes in buffers of one capacity above both: the soup (degenerate faces, a fan of 200) and blob33, vertex
    rows beyond the counts NaN, face rows beyond them out of range, one valid face among those."""
    golden = dict(load_golden("mesh_normals"))
    names = ("soup", "blob33")
    meshes = [normals_mesh(golden, name) for name in names]
    max_v = max(len(v) for v, _ in meshes) + 300
    max_f = max(len(f) for _, f in meshes) + 500
    padded = [cases.padded_mesh(v, f, max_v, max_f) for v, f in meshes]
    want = {mode: [normals_expected(golden, name, mode) for name in names] for mode in ("reference", "accumulate")}
    return padded, want


@fills
@pytest.mark.parametrize("mode", ["reference", "accumulate"])
def test_mesh_normals_batch(ops, mode, byte):
    padded, want = _normals_case()
    verts, faces, counts = ([dev(m[k]) for m in padded] for k in range(3))
    out = on_dirty_arena(ops, byte, lambda: ops.mesh_normals_raw_batch(
        verts, faces, counts, mode, out=full((2,) + tuple(verts[0].shape), POISON)))
    for k in range(2):
        got = out[k].cpu().numpy()
        nv = int(padded[k][2][0])
        assert np.array_equal(got[:nv].view(np.uint32), want[mode][k].view(np.uint32)), k
        assert (got[nv:] == POISON).all(), k
    agree(("mesh_normals", mode), byte, *out)


@functools.lru_cache(maxsize=None)
def _simplify_case():
    """The soup of mesh_simplify_ref (invalid vertices, faces out of range) as it is, and told to be 50 vertices and
    100 faces shorter: its last faces then name vertices at or beyond counts[0]."""
    v, f = ms.soup()
    max_v, max_f = len(v) + 40, len(f) + 60
    return [cases.padded_mesh(v, f, max_v, max_f), cases.padded_mesh(v, f, max_v, max_f, (len(v) - 50, len(f) - 100))]


@fills
def test_mesh_simplify_batch(ops, byte):
    padded = _simplify_case()
    meshes = [tuple(dev(a) for a in m) for m in padded]
    max_v, max_f = meshes[0][0].shape[0], meshes[0][1].shape[0]

    def op():
        out = (full((2, max_v, 3), POISON), full((2, max_f, 3), IPOISON, torch.int32), full((2, 2), IPOISON, torch.int32),
               full((2, max_v), IPOISON, torch.int32))
        ops.mesh_simplify_raw_batch([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes],
                                    ms.SOUP_CELLS, ms.SOUP_BMIN, ms.SOUP_BMAX, out=out)
        return out

    out = on_dirty_arena(ops, byte, op)
    sizes = [simplify_check(tuple(o[k] for o in out), meshes[k], ms.SOUP_CELLS, ms.SOUP_BMIN, ms.SOUP_BMAX,
                            "soup, frame %d" % k) for k in range(2)]
    assert all(nv > 100 and nf > 100 for nv, nf in sizes) and sizes[0] != sizes[1]
    agree("mesh_simplify", byte, *out)


@functools.lru_cache(maxsize=None)
def _smooth_case():
    """The smoothing soup (degenerate faces, unreferenced vertices, a fan of 200) and the open mesh (227 border
    vertices) in buffers of one capacity."""
    meshes = [sm.soup(), sm.open_mesh()]
    max_v = max(len(v) for v, _ in meshes) + 70
    max_f = max(len(f) for _, f in meshes) + 90
    return [cases.padded_mesh(v, f, max_v, max_f) for v, f in meshes]


_SMOOTH_WANT = {}


@fills
def test_mesh_smooth_batch(ops, byte):
    """Two iterations, border vertices pinned and free, one call after the other on the same arena."""
    padded = _smooth_case()
    meshes = [tuple(dev(a) for a in m) for m in padded]
    max_v = meshes[0][0].shape[0]

    def op():
        outs = {}
        for pin in (True, False):
            out, ring = full((2, max_v, 3), POISON), full((2, max_v), IPOISON, torch.int32)
            ops.mesh_smooth_raw_batch([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes], 2,
                                      pin_border=pin, out=out, ring=ring)
            outs[pin] = (out, ring)
        return outs

    outs = on_dirty_arena(ops, byte, op)
    for pin, (out, ring) in outs.items():
        for k in range(2):
            with np.errstate(all="ignore"):
                _SMOOTH_WANT[pin, k] = smooth_check((out[k], ring[k]), meshes[k], 2, int(pin), what="frame %d" % k,
                                                    want=_SMOOTH_WANT.get((pin, k)))
        agree(("mesh_smooth", pin), byte, out, ring)
    assert (_SMOOTH_WANT[True, 1][1] < 0).sum() == 227
    assert not sm.same_bits(_SMOOTH_WANT[True, 1][0], _SMOOTH_WANT[False, 1][0])


@functools.lru_cache(maxsize=None)
def _render_meshes():
    xyz, faces, attr, _ = render_soup()  # two triangles across the whole picture, small ones, faces that are skipped
    xyz2, attr2 = cases.mirrored(xyz, attr)
    return [(xyz, faces, attr), (xyz2, faces, attr2)]


_RENDER_WANT = {}


def _render_want(ops, verts, views, nearest):
    """The restatement's picture per (mesh, view), made once on the default stream."""
    meshes = _render_meshes()
    for m in range(2):
        for v in range(2):
            if (m, v, nearest) not in _RENDER_WANT:
                _RENDER_WANT[m, v, nearest] = render_ref.render(
                    projected(ops, verts[m], views[v], "orthogonal"), meshes[m][1], 32, 32, attr=meshes[m][2],
                    nearest=nearest, **PREDS)
    want = _RENDER_WANT[0, 0, nearest]
    assert (want.cover > 2).sum() > 100 and len(np.unique(want.face)) > 30  # the large faces and many small ones
    return _RENDER_WANT


@fills
@pytest.mark.parametrize("nearest", ["max", "min"])
def test_mesh_render_batch(ops, nearest, byte):
    """32 x 32, two meshes x two views: the keys (cleared to 0 = no fragment), the counters and lists of the faces too
    large for one thread (raster_large), the snapped vertices of four image slots.  A stale key would win or lose
    against real fragments; a stale counter would list faces that are not there."""
    meshes = _render_meshes()
    verts = [dev(m[0]) for m in meshes]
    faces = [dev(m[1]) for m in meshes]
    attrs = [dev(m[2]) for m in meshes]
    counts = [torch.tensor([len(m[0]), len(m[1])], dtype=torch.int32, device=DEV) for m in meshes]
    cams = _cameras()
    views = torch.stack([cams["identity"][0], cams["scene"][0]])
    want = _render_want(ops, verts, views, nearest)
    # the two spanning triangles take the list path: their boxes hold the whole picture, far more than one thread walks
    assert sum(int((want[0, 0, nearest].face == f).any()) for f in (0, 1)) >= 1

    def op():
        out = (full((2, 2, 32, 32, 3), POISON), full((2, 2, 32, 32), POISON), full((2, 2, 32, 32), IPOISON, torch.int32))
        ops.mesh_render_raw_batch(verts, faces, counts, attrs, [views] * 2, 32, nearest=nearest, out=out, **PREDS)
        return out

    image, depth, face = on_dirty_arena(ops, byte, op)
    for m in range(2):
        for v in range(2):
            render_same((image[m, v], depth[m, v], face[m, v]), want[m, v, nearest], "mesh %d view %d" % (m, v))
    agree(("mesh_render", nearest), byte, image, depth, face)


@fills
@pytest.mark.parametrize("connectivity", [6, 26])
def test_keep_largest_batch(ops, connectivity, byte):
    """r = 17 (4913 voxels: the last int4 of the labels is partial), three frames: two equal cubes (the tie), gated off
    (its volume NaN, its output must keep the poison), bodies joined over a NaN bridge."""
    names = ["equal_cubes17", None, "nan_bridge17"]
    vols = [full((17, 17, 17), float("nan")) if n is None else dev(np.array(kl.volume(n))) for n in names]
    gates = [None, torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1,), 7, dtype=torch.int32, device=DEV)]

    def op():
        out = (full((3, 17, 17, 17), POISON), full((3, 4), IPOISON, torch.int32))
        ops.keep_largest_raw_batch(vols, kl.LEVEL, connectivity, 0.0, gates=gates, out=out)
        return out

    cleaned, stats = on_dirty_arena(ops, byte, op)
    for k, name in enumerate(names):
        if name is None:
            assert stats[k].cpu().tolist() == [0, 0, 0, -1] and (cleaned[k] == POISON).all()
            continue
        want, want_stats = kl.reference(name, connectivity)
        assert stats[k].cpu().tolist() == want_stats, name
        assert np.array_equal(_host(cleaned[k]), want.view(np.uint32)), name
    agree(("keep_largest", connectivity), byte, cleaned, stats)


# ---- the encoder context -------------------------------------------------------------------------------------------
@fills
def test_group_norm_on_the_encoder_context(ops, byte):
    """n = 2, C = 64, 16 x 16, 32 groups at |mean| / std = 1e3 (tests/test_gn_offset_gpu.py): the per-slice partial
    sums in double are the arena's; the bar is that module's -- twice torch's own f32 error + 1e-6."""
    x = gn_input(2, 64, 16, 16, 21)
    gn = gn_module(64, 22)
    with torch.no_grad():
        ref = er.group_norm(x, 32, gn.weight, gn.bias, gn.eps)
        bar = 2.0 * (gn(x).double() - ref).abs().max().item() + 1e-6
    y = on_dirty_arena(ops, byte, lambda: ops.group_norm(x, 32, gn.weight.detach(), gn.bias.detach(), gn.eps),
                       role="encoder")
    err = (y.double() - ref).abs().max().item()
    print("group_norm under fill 0x%02X: %.3g (bar %.3g)" % (byte, err, bar))
    assert err <= bar
    agree("group_norm", byte, y)


# ---- the chain, once -----------------------------------------------------------------------------------------------
def _chain(ops, scene):
    """recon -> keep_largest -> marching cubes -> normals -> simplify -> smooth -> render, through ops on the current
    stream: each stage starts on what the one before it left in the arena.  Every output goes into a poisoned buffer, so
    whole buffers compare."""
    r = RES[-1]
    max_v, max_f = 12 * r * r, 24 * r * r
    vol, status = ops.recon(scene["mlp"], scene["feats"][0], scene["cals"][0], syn.Z_SCALE, BMIN, BMAX, RES,
                            volume=full((r, r, r), POISON), status=full((1 + len(RES),), IPOISON, torch.int32))
    (clean, stats), = ops.keep_largest_raw_batch([vol], 0.5, 26, 0.0,
                                                 out=(full((1, r, r, r), POISON), full((1, 4), IPOISON, torch.int32)))
    (verts, faces, counts), = ops.marching_cubes_raw_batch(
        [clean], 0.5, BMIN, BMAX, out=(full((1, max_v, 3), POISON), full((1, max_f, 3), IPOISON, torch.int32),
                                       full((1, 2), IPOISON, torch.int32)))
    normals = ops.mesh_normals_raw(verts, faces, counts, "accumulate", out=full((max_v, 3), POISON))
    s_verts, s_faces, s_counts, vmap = ops.mesh_simplify_raw(
        verts, faces, counts, 16, BMIN, BMAX, out=(full((max_v, 3), POISON), full((max_f, 3), IPOISON, torch.int32),
                                                   full((2,), IPOISON, torch.int32), full((max_v,), IPOISON, torch.int32)))
    smooth = ops.mesh_smooth_raw(s_verts, s_faces, s_counts, 2, out=full((max_v, 3), POISON))
    colours = ops.mesh_normals_raw(smooth, s_faces, s_counts, "accumulate", out=full((max_v, 3), POISON))
    cams = _cameras()
    image, depth, face = ops.mesh_render_raw(
        smooth, s_faces, s_counts, colours, torch.stack([cams["identity"][0], cams["scene"][0]]), 32,
        out=(full((2, 32, 32, 3), POISON), full((2, 32, 32), POISON), full((2, 32, 32), IPOISON, torch.int32)), **NORMALS)
    return dict(status=status, vol=vol, clean=clean, stats=stats, verts=verts, faces=faces, counts=counts,
                normals=normals, s_verts=s_verts, s_faces=s_faces, s_counts=s_counts, vmap=vmap, smooth=smooth,
                image=image, depth=depth, face=face)


@pytest.fixture(scope="module")
def clean_chain(ops, scene):
    """The chain on a stream whose arena holds zeros."""
    out = on_dirty_arena(ops, 0x00, lambda: _chain(ops, scene))
    nv, nf = out["counts"].cpu().tolist()
    sv, sf = out["s_counts"].cpu().tolist()
    print("chain: status %s, kept %s, mesh %d / %d, simplified %d / %d, %d pixels covered"
          % (out["status"].cpu().tolist(), out["stats"].cpu().tolist(), nv, nf, sv, sf, int((out["face"] >= 0).sum())))
    assert 0 < sv < nv <= out["verts"].shape[0] and 0 < sf < nf <= out["faces"].shape[0]
    assert int((out["face"][0] >= 0).sum()) > 30 and int((out["face"][1] >= 0).sum()) > 30
    return {k: _host(t) for k, t in out.items()}


@pytest.mark.parametrize("byte", cases.FILLS[1:], ids=cases.FILL_IDS[1:])
def test_the_chain(ops, scene, clean_chain, byte):
    """The final mesh and picture -- and every intermediate buffer -- of the chain on dirt have the bits of the chain
    on zeros."""
    out = on_dirty_arena(ops, byte, lambda: _chain(ops, scene))
    for name in ("smooth", "s_faces", "s_counts", "image", "depth", "face") + tuple(clean_chain):
        got = _host(out[name])
        assert got.shape == clean_chain[name].shape and np.array_equal(got, clean_chain[name]), name
