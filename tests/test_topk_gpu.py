"""The fixed-budget octree refinement on the GPU (csrc/topk.hip): mp_octree_select_topk and mp_recon_topk_batch through
ctypes, ops.recon_topk(_batch), ops.LevelEngine(num_points=...) and Seg3dTopk.  The kernels are held to the numpy
restatement of the header's definition (tests/topk_ref.py): the selected set (``packed[:count]`` compared sorted -- the
order of the list is unspecified), ``cur``, ``ev_cur``, volumes and counts exactly.  Needs an MI355X."""
import ctypes
import warnings

import numpy as np
import pytest

import topk_ref
from octree_ref import codes as _codes, pack_bits as _pack_bits
from monoport_amd import synthetic as syn
from oracle import pifu_oracle as po  # numpy parts only here (upsample2x); the built oracle is the `oracle` fixture

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
MP_OK, MP_ERR_ARG = 0, -1
POISON = -12345.0
IPOISON = -777
INF = float("inf")


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
    return ctypes.c_void_p(t.data_ptr())


def _pp(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _select(abi, prev, ev_prev, k, max_dist=INF, balance=0.5):
    """One mp_octree_select_topk call on poisoned outputs -> (cur bits, ev_cur words, sorted selected codes)."""
    lib, h, st = abi
    rp = prev.shape[0]
    r = 2 * rp - 1
    words = r * r * ((r + 63) // 64)
    d_prev = torch.from_numpy(np.ascontiguousarray(prev)).to(DEV)
    d_evp = torch.from_numpy(_pack_bits(ev_prev).view(np.int64)).to(DEV)
    cur = torch.full((r, r, r), POISON, dtype=torch.float32, device=DEV)
    ev_cur = torch.full((words,), IPOISON, dtype=torch.int64, device=DEV)
    packed = torch.full((r ** 3,), IPOISON, dtype=torch.int32, device=DEV)
    count = torch.full((1,), IPOISON, dtype=torch.int32, device=DEV)
    rc = lib.mp_octree_select_topk(h, _p(d_prev), rp, _p(cur), r, _p(d_evp), _p(ev_cur), int(k), max_dist, balance,
                                   _p(packed), _p(count), st)
    assert rc == MP_OK, lib.mp_last_error(h).decode()
    n = int(count.item())
    packed = packed.cpu().numpy()
    assert 0 <= n <= r ** 3
    assert (packed[n:] == IPOISON).all()  # nothing is written behind the count
    return cur.cpu().numpy().view(np.uint32), ev_cur.cpu().numpy().view(np.uint64), np.sort(packed[:n].astype(np.int64))


def _reference(prev, ev_prev, k, max_dist=INF, balance=0.5):
    cur = po.upsample2x(prev)
    ev = topk_ref.evaluated_image(ev_prev)
    sel = topk_ref.select_topk(cur, ev, k, max_dist, balance)
    ev_after = ev.copy()
    ev_after.reshape(-1)[sel] = True
    return cur.view(np.uint32), _pack_bits(ev_after), _codes(sel, cur.shape[0])


def _check(abi, prev, ev_prev, k, max_dist=INF, balance=0.5):
    got = _select(abi, prev, ev_prev, k, max_dist, balance)
    want = _reference(prev, ev_prev, k, max_dist, balance)
    assert got[2].shape == want[2].shape, (k, got[2].shape, want[2].shape)
    assert np.array_equal(got[2], want[2]), k
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
    return got


def _random_volume(rp, seed):
    """Random field with plateaus of exact ties (values on a coarse grid), NaNs and a random evaluated set."""
    rng = np.random.default_rng(seed)
    prev = rng.random((rp, rp, rp), dtype=np.float32)
    plateau = rng.random((rp, rp, rp)) < 0.35
    prev[plateau] = np.round(prev[plateau] * 8) / 8  # equal values, and equal averages of them one level up
    prev[rng.random((rp, rp, rp)) < 0.01] = np.nan
    prev[rp // 2:, : rp // 3] = 0.25  # a block of one value: a long run of ties in linear index order
    ev_prev = rng.random((rp, rp, rp)) < 0.5
    return prev, ev_prev


def _tie_run(prev, ev_prev, max_dist=INF, balance=0.5):
    """(#candidates, start, end) of the longest run of equal keys in the sorted candidate list."""
    cur = po.upsample2x(prev)
    sel = topk_ref.select_topk(cur, topk_ref.evaluated_image(ev_prev), cur.size, max_dist, balance)
    u = np.abs(cur.reshape(-1)[sel] - np.float32(balance))
    starts = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
    lengths = np.diff(np.r_[starts, u.size])
    i = int(np.argmax(lengths))
    return sel.size, int(starts[i]), int(starts[i] + lengths[i])


@pytest.mark.parametrize("rp,seed", [(17, 1), (33, 2)])
def test_select_random_volume_every_budget(abi, rp, seed):
    """r = 33 and 65 (tail blocks, rows that are no multiple of 64): k = 0, 1, 2, inside a run of tied keys, exactly
    at its end, #candidates and r^3, on a random field with plateaus, NaNs and a random evaluated set."""
    prev, ev_prev = _random_volume(rp, seed)
    n_cand, start, end = _tie_run(prev, ev_prev)
    r = 2 * rp - 1
    assert end - start > 100 and np.isnan(po.upsample2x(prev)).sum() > 0
    for k in (0, 1, 2, start + 1, (start + end) // 2, end - 1, end, n_cand, r ** 3):
        _, _, codes = _check(abi, prev, ev_prev, k)
        assert codes.size == min(k, n_cand)
    # a balance off 0.5 moves every key
    _check(abi, prev, ev_prev, (start + end) // 2, balance=0.3)


def test_select_max_dist_cuts_below_the_budget(abi):
    prev, ev_prev = _random_volume(17, 3)
    n_cand, _, _ = _tie_run(prev, ev_prev)
    n_near, _, _ = _tie_run(prev, ev_prev, max_dist=0.1)
    assert 0 < n_near < n_cand
    _, _, codes = _check(abi, prev, ev_prev, n_cand, max_dist=0.1)
    assert codes.size == n_near
    _check(abi, prev, ev_prev, n_near // 2, max_dist=0.1)
    _, _, codes = _check(abi, prev, ev_prev, n_cand, max_dist=0.0)  # only nodes exactly on the threshold
    assert codes.size == _tie_run(prev, ev_prev, max_dist=0.0)[0]


def _half_zero(rp):
    """An analytic body in one half of the box, exactly 0.0 in the other: u == balance there, a run of hundreds of
    thousands of ties behind every key of the body's half."""
    c = (np.arange(rp, dtype=np.float32) / np.float32(rp - 1) * 2 - 1).astype(np.float32)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    d = np.sqrt(x * x + y * y + z * z).astype(np.float32)
    prev = (1.0 / (1.0 + np.exp(-(np.float32(0.6) - d) * np.float32(6)))).astype(np.float32)
    prev[:, :, rp // 2 + 1:] = 0.0
    return prev


def test_select_129_threshold_inside_a_huge_tie_run(abi):
    """129 from 65: the ties at u == balance straddle the threshold and span thousands of blocks of the tie scan;
    level 0's evaluated set (every node) as in the engine."""
    rp = 65
    prev = _half_zero(rp)
    ev_prev = np.ones((rp, rp, rp), bool)
    n_cand, start, end = _tie_run(prev, ev_prev)
    assert end - start > 300000 and end == n_cand
    for k in (start + 12345, end - 1, start):
        _, _, codes = _check(abi, prev, ev_prev, k)
        assert codes.size == k
    # the same call twice: the same set and the same bits
    a = _select(abi, prev, ev_prev, start + 12345)
    b = _select(abi, prev, ev_prev, start + 12345)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_select_257_tie_scan_over_thousands_of_blocks(abi):
    """257 from 129: a slab of one value crosses every row, so every one of the 5160 blocks holds ties and the tie
    scan runs over several chunks with a carry; the ties lie exactly on max_dist, which keeps the candidates few."""
    rp = 129
    c = (np.arange(rp, dtype=np.float32) / np.float32(rp - 1) * 2 - 1).astype(np.float32)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    prev = (1.0 / (1.0 + np.exp(-(np.float32(0.6) - np.sqrt(x * x + y * y + z * z)) * np.float32(6)))).astype(np.float32)
    prev[:, :, 40:60] = 0.25
    ev_prev = np.ones((rp, rp, rp), bool)
    n_cand, start, end = _tie_run(prev, ev_prev, max_dist=0.25)
    assert end - start > 2000000 and end == n_cand
    _, _, codes = _check(abi, prev, ev_prev, (start + end) // 2, max_dist=0.25)
    assert codes.size == (start + end) // 2


def test_select_equal_keys_on_two_planes(abi):
    """Two nodes with the same smallest u on different z planes, k = 1: the smaller linear index wins."""
    rp = 9
    prev = np.full((rp, rp, rp), 0.9, np.float32)
    prev[5, 1, 2] = prev[2, 3, 4] = 0.5625
    none = np.zeros((rp, rp, rp), bool)
    _, _, codes = _check(abi, prev, none, 1)
    assert list(codes) == [8 | (6 << 10) | (4 << 20)]
    _, _, codes = _check(abi, prev, none, 2)
    assert list(codes) == sorted([8 | (6 << 10) | (4 << 20), 4 | (2 << 10) | (10 << 20)])


def test_select_refusals(abi):
    lib, h, st = abi
    rp, r = 9, 17
    prev = torch.zeros((rp, rp, rp), dtype=torch.float32, device=DEV)
    cur = torch.zeros((r, r, r), dtype=torch.float32, device=DEV)
    evp = torch.zeros((rp * rp,), dtype=torch.int64, device=DEV)
    ev = torch.zeros((r * r + 1,), dtype=torch.int64, device=DEV)
    packed = torch.zeros((r ** 3,), dtype=torch.int32, device=DEV)
    count = torch.zeros((2,), dtype=torch.int32, device=DEV)

    def call(prev=prev, rp=rp, cur=cur, r=r, evp=evp, ev=ev, k=10, max_dist=INF, packed=packed, count=count):
        ptr = lambda t: t if t is None or isinstance(t, ctypes.c_void_p) else _p(t)
        return lib.mp_octree_select_topk(h, ptr(prev), rp, ptr(cur), r, ptr(evp), ptr(ev), k, max_dist, 0.5,
                                         ptr(packed), ptr(count), st)

    assert call() == MP_OK
    assert call(k=r ** 3) == MP_OK and call(k=0) == MP_OK and call(max_dist=0.0) == MP_OK
    for bad in (dict(k=-1), dict(k=r ** 3 + 1), dict(max_dist=float("nan")), dict(max_dist=-0.5), dict(prev=None),
                dict(cur=None), dict(evp=None), dict(ev=None), dict(packed=None), dict(count=None), dict(r=r + 1),
                dict(rp=1, r=1), dict(cur=ctypes.c_void_p(cur.data_ptr() + 2)),
                dict(ev=ctypes.c_void_p(ev.data_ptr() + 4)), dict(count=ctypes.c_void_p(count.data_ptr() + 1))):
        assert call(**bad) == MP_ERR_ARG, bad
        assert b"mp_octree_select_topk" in lib.mp_last_error(h)
    torch.cuda.synchronize()


# ---- the fused engine: mp_recon_topk_batch ------------------------------------------------------------------
def _gpu_query(ops, mlp, fh, cal, projection="orthogonal"):
    def gpu_query(pts):  # [3,N] numpy -> [N] numpy through the HIP query kernel
        out = ops.query(mlp, fh, torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV), cal, syn.Z_SCALE,
                        ops.PROJECTIONS[projection])
        return out[0, 0].cpu().numpy()
    return gpu_query


@pytest.fixture(scope="module")
def body(ops, oracle):
    """The scene of tests/test_recon_gpu.py's ``body`` fixture."""
    layers = syn.body_mlp("G", noise=0.05, seed=1)
    f = syn.body_feat(256, 128, 128, 2)
    calib = oracle.pifu_calib(*syn.scene_camera(30))
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    cal = torch.from_numpy(calib).to(DEV)
    return dict(layers=layers, f=f, calib=calib, mlp=mlp, fh=fh, cal=cal, gpu_query=_gpu_query(ops, mlp, fh, cal))


_LOSSLESS = {}


def _lossless_counts(oracle, body, res):
    """Points per level of the lossless schedule on the body scene (computed once per resolution list)."""
    key = tuple(res)
    if key not in _LOSSLESS:
        stats = []
        oracle.seg3d_lossless(body["gpu_query"], BMIN, BMAX, res, stats=stats)
        _LOSSLESS[key] = stats
    return _LOSSLESS[key]


def _check_fused(ops, body, res, budgets, max_dist=None):
    vol, status = ops.recon_topk(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, BMIN, BMAX, res, budgets, max_dist)
    stats = []
    ref = topk_ref.seg3d_topk(body["gpu_query"], BMIN, BMAX, res, budgets, max_dist, stats=stats)
    status = status.cpu().numpy().tolist()
    print("res %s budgets %s max_dist %s: status %s (restatement %s)" % (res, budgets, max_dist, status, stats))
    assert status == [1] + stats
    assert np.array_equal(vol.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    return ref, stats


@pytest.mark.parametrize("res", [[9, 17, 33], [17, 33, 65], [17, 33, 65, 129]])
def test_recon_topk_bit_exact_vs_restatement(ops, oracle, body, res):
    """Budgets of 1/4 of the lossless counts and one above them: volume and status equal the numpy restatement
    driven by the same HIP query kernel, bit for bit."""
    lossless = _lossless_counts(oracle, body, res)
    quarter = [0] + [max(s // 4, 1) for s in lossless[1:]]
    above = [0] + [min(2 * s, r ** 3) for s, r in zip(lossless[1:], res[1:])]
    _, stats = _check_fused(ops, body, res, quarter)
    assert stats[1:] == quarter[1:]
    _check_fused(ops, body, res, above)


def test_recon_topk_full_budgets_equal_dense_evaluation(ops, oracle, body):
    res = [9, 17, 33]
    ref, stats = _check_fused(ops, body, res, [r ** 3 for r in res])
    assert stats == [9 ** 3, 17 ** 3 - 9 ** 3, 33 ** 3 - 17 ** 3]
    assert np.array_equal(ref, oracle.dense_volume(body["gpu_query"], BMIN, BMAX, 33))


def test_recon_topk_zero_budget_and_bounds(ops, oracle, body):
    res = [9, 17, 33, 65]
    _, stats = _check_fused(ops, body, res, [0, 500, 0, 3000])  # a level that is only upsampled
    assert stats == [9 ** 3, 500, 0, 3000]
    _, stats = _check_fused(ops, body, res, [0, 17 ** 3, 33 ** 3, 65 ** 3], [INF, 0.2, 0.1, 0.05])
    assert all(0 < s < r ** 3 // 2 for s, r in zip(stats[1:], res[1:]))


def _frames(ops, oracle, n, empty=None):
    """n frames with their own feature maps and cameras; frame ``empty`` looks past the box."""
    feats, cals = [], []
    for i in range(n):
        feats.append(ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2 + i))[None].to(DEV)))
        calib = oracle.pifu_calib(*syn.scene_camera(25 * i))
        if i == empty:
            calib[0, 0, 3] = 5.0
        cals.append(torch.from_numpy(calib).to(DEV))
    return feats, cals


def test_recon_topk_batch_equals_single_frames(ops, oracle, body):
    """3 frames with different maps and cameras, one of them empty, volumes poisoned before the call: the live
    frames equal the single-frame calls bit for bit, the empty frame's status is [0, r0^3, 0, ...]; then
    mp_max_frames() frames in one call."""
    mlp = body["mlp"]
    res, budgets, max_dist = [9, 17, 33, 65], [0, 400, 1500, 5000], [INF, INF, 0.3, 0.3]
    feats, cals = _frames(ops, oracle, 3, empty=1)
    singles = [ops.recon_topk(mlp, feats[i], cals[i], syn.Z_SCALE, BMIN, BMAX, res, budgets, max_dist)
               for i in range(3)]
    volumes = [torch.full((65, 65, 65), POISON, dtype=torch.float32, device=DEV) for _ in range(3)]
    vols, status = ops.recon_topk_batch(mlp, feats, cals, syn.Z_SCALE, BMIN, BMAX, res, budgets, max_dist,
                                        volumes=volumes)
    st = status.cpu().numpy()
    print("batch status\n%s" % st)
    assert st[1].tolist() == [0, 9 ** 3, 0, 0, 0]
    for i in (0, 2):
        assert st[i, 0] == 1 and st[i, 2] == 400 and st[i, 3] > 0
        assert np.array_equal(st[i], singles[i][1].cpu().numpy()), i
        assert torch.equal(vols[i].view(torch.int32), singles[i][0].view(torch.int32)), i
    assert np.array_equal(singles[1][1].cpu().numpy(), st[1])
    assert not torch.equal(vols[0], vols[2])
    # frame 2 against the restatement on its own map and camera
    stats = []
    ref = topk_ref.seg3d_topk(_gpu_query(ops, mlp, feats[2], cals[2]), BMIN, BMAX, res, budgets, max_dist, stats=stats)
    assert st[2].tolist() == [1] + stats and np.array_equal(vols[2].cpu().numpy().view(np.uint32), ref.view(np.uint32))
    # the most frames one call takes
    n = ops.MAX_FRAMES
    res, budgets = [9, 17, 33], [0, 300, 1000]
    many, status = ops.recon_topk_batch(mlp, [feats[i % 3] for i in range(n)], [cals[i % 3] for i in range(n)],
                                        syn.Z_SCALE, BMIN, BMAX, res, budgets)
    st = status.cpu().numpy()
    for i in (0, 2):
        v1, s1 = ops.recon_topk(mlp, feats[i], cals[i], syn.Z_SCALE, BMIN, BMAX, res, budgets)
        for j in range(i, n, 3):
            assert np.array_equal(st[j], s1.cpu().numpy()) and torch.equal(many[j], v1), j
    assert all(st[j].tolist() == [0, 9 ** 3, 0, 0] for j in range(1, n, 3))
    with pytest.raises(ValueError):
        ops.recon_topk(mlp, feats[0], cals[0], syn.Z_SCALE, BMIN, BMAX, res, [0, 300])


def test_recon_topk_perspective_frame_with_nan_nodes(ops, oracle, body):
    """A perspective camera at the centre of the box looking along z: the lattice plane z == 0 cuts the body and
    projects to NaN, and so does what the upsample makes of it -- none of those nodes is a candidate, their
    neighbours are selected."""
    calib = np.zeros((1, 4, 4), np.float32)
    calib[0, 0, 0], calib[0, 1, 1], calib[0, 2, 2], calib[0, 3, 3] = 0.05, -0.05, 1.0, 1.0  # z_cam == world z
    cal = torch.from_numpy(calib).to(DEV)
    q = _gpu_query(ops, body["mlp"], body["fh"], cal, "perspective")
    res, budgets = [17, 33, 65], [0, 3000, 20000]
    level0 = oracle.dense_volume(q, BMIN, BMAX, 17, 65)
    print("perspective level 0: %d NaN, %d inside" % (np.isnan(level0).sum(), (level0 > 0.5).sum()))
    assert np.isnan(level0[8]).all() and not np.isnan(level0[[7, 9]]).any() and (level0 > 0.5).sum() > 50
    vol, status = ops.recon_topk(body["mlp"], body["fh"], cal, syn.Z_SCALE, BMIN, BMAX, res, budgets,
                                 projection="perspective")
    stats = []
    ref = topk_ref.seg3d_topk(q, BMIN, BMAX, res, budgets, stats=stats)
    assert status.cpu().numpy().tolist() == [1] + stats == [1, 17 ** 3, 3000, 20000]
    v = vol.cpu().numpy()
    assert np.array_equal(v.view(np.uint32), ref.view(np.uint32))
    nan = np.isnan(v)
    assert nan[29:36].all() and not nan[:29].any() and not nan[36:].any()  # the slab no level may refine
    near = np.abs(po.upsample2x(po.upsample2x(level0)) - 0.5) < 0.4  # where the last level's candidates were
    assert (v[28] != po.upsample2x(po.upsample2x(level0))[28])[near[28]].any()  # evaluated right next to the slab


def _topk_call(abi, body, **over):
    """One mp_recon_topk_batch call on the body scene with arguments replaced by ``over`` -> return code."""
    lib, h, st = abi
    res = over.pop("res", [9, 17, 33])
    n = over.pop("n_frames", 1)
    k = over.pop("num_points", [0, 100, 100])
    md = over.pop("max_dist", None)
    vol = torch.empty((res[-1],) * 3, dtype=torch.float32, device=DEV)
    status = torch.empty((1 + len(res),), dtype=torch.int32, device=DEV)
    a = dict(feat=_pp([body["fh"]] * max(n, 1)), calib=_pp([body["cal"]] * max(n, 1)), volume=_pp([vol] * max(n, 1)),
             status=_pp([status] * max(n, 1)), b_min=(ctypes.c_float * 3)(*BMIN), b_max=(ctypes.c_float * 3)(*BMAX),
             res_arg=(ctypes.c_int * len(res))(*res),
             num_points=None if k is None else (ctypes.c_int64 * len(k))(*k))
    a.update(over)
    hh, ww, c = body["fh"].shape
    rc = lib.mp_recon_topk_batch(h, body["mlp"].id, n, a["feat"], c, hh, ww, a["calib"], None, syn.Z_SCALE, a["b_min"],
                                 a["b_max"], a["res_arg"], len(res), a["num_points"],
                                 None if md is None else (ctypes.c_float * len(md))(*md), 0.5, a["volume"],
                                 a["status"], None, st)
    torch.cuda.synchronize()
    return rc


def test_recon_topk_refusals(abi, ops, body):
    lib, h, _ = abi
    assert _topk_call(abi, body) == MP_OK
    assert _topk_call(abi, body, num_points=[-5, 17 ** 3, 0], max_dist=[-1.0, 0.0, INF]) == MP_OK  # entry 0: ignored
    for bad in (dict(num_points=[0, -1, 100]), dict(num_points=[0, 100, 33 ** 3 + 1]),
                dict(max_dist=[INF, float("nan"), INF]), dict(max_dist=[INF, INF, -0.25]), dict(num_points=None),
                dict(feat=None), dict(calib=None), dict(volume=None), dict(status=None), dict(b_min=None),
                dict(res_arg=None), dict(feat=_pp([None])), dict(volume=_pp([None])), dict(status=_pp([None])),
                dict(feat=(ctypes.c_void_p * 1)(body["fh"].data_ptr() + 4)),
                dict(res=[9, 17, 34]), dict(res=[9, 18, 35]), dict(res=[1, 1, 1]),
                dict(n_frames=0), dict(n_frames=ops.MAX_FRAMES + 1)):
        assert _topk_call(abi, body, **bad) == MP_ERR_ARG, bad
        assert b"mp_recon_topk_batch" in lib.mp_last_error(h), bad


# ---- the Python layers: LevelEngine(num_points=...), recon_generic, Seg3dTopk --------------------------------
@pytest.fixture()
def net(ops, body, monkeypatch):
    """netG with the body head, its feature list, and a plain query_func (RTL/main.py:169-183).  The restatement is
    driven by the plain query kernel: keep netG.query on it too."""
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

    return dict(netG=netG, feats=feats, query_func=query_func)


BOX = dict(b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]))


def test_seg3d_topk_fused_generic_and_restatement(ops, oracle, body, net):
    """Seg3dTopk on a plain netG.query takes the fused call; a query_func that reaches the same kernel without
    MonoPortNet.query (and adds + 0.0) runs level by level: the same volume and counts, which are the restatement's
    and ops.recon_generic's."""
    from monoport_amd.implicit_seg.functional import Seg3dTopk
    res, budgets = [9, 17, 33, 65], [0, 500, 2000, 8000]
    eng = Seg3dTopk(query_func=net["query_func"], resolutions=res, num_points=budgets, **BOX).to(DEV)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sdf = eng(feats=net["feats"], calib=body["cal"])
    assert not [w for w in caught if "Seg3dTopk" in str(w.message)]
    assert eng.last_path == "fused" and sdf.shape == (1, 1, 65, 65, 65)
    stats = []
    ref = topk_ref.seg3d_topk(body["gpu_query"], BMIN, BMAX, res, budgets, stats=stats)
    assert eng.last_status.tolist() == [1] + stats == [1, 9 ** 3] + budgets[1:]
    fused = sdf[0, 0].cpu().numpy()
    assert np.array_equal(fused.view(np.uint32), ref.view(np.uint32))

    def wrapped(points, feats, calib):  # not a MonoPortNet.query call: nothing to bind the fused engine to
        return ops.query(body["mlp"], body["fh"], points.permute(0, 2, 1), calib, syn.Z_SCALE) + 0.0

    gen = Seg3dTopk(query_func=wrapped, resolutions=res, num_points=budgets, **BOX).to(DEV)
    vol = gen(feats=net["feats"], calib=body["cal"])
    assert gen.last_path == "generic" and gen.last_status.tolist() == [1] + stats
    vol = vol[0, 0].cpu().numpy()
    assert np.array_equal(vol > 0.5, fused > 0.5) and np.array_equal(vol, fused)
    v2, counts = ops.recon_generic(wrapped, dict(feats=net["feats"], calib=body["cal"]), DEV, BMIN, BMAX, res,
                                   num_points=budgets)
    assert counts == stats and np.array_equal(v2.cpu().numpy(), fused)
    # a wrapper AROUND netG.query whose values differ is noticed on the coarsest level and honoured
    flipped = Seg3dTopk(query_func=lambda **kw: 1.0 - net["query_func"](**kw), resolutions=res, num_points=budgets,
                        **BOX).to(DEV)
    with pytest.warns(UserWarning, match="Seg3dTopk: query_func is not a plain MonoPortNet.query"):
        out = flipped(feats=net["feats"], calib=body["cal"])
    assert flipped.last_path == "generic"
    ref = topk_ref.seg3d_topk(lambda p: (np.float32(1.0) - body["gpu_query"](p)).astype(np.float32), BMIN, BMAX, res,
                              budgets)
    assert np.array_equal(out[0, 0].cpu().numpy(), ref)


def test_seg3d_topk_clip_mins_none_async_and_many(ops, oracle, body, net):
    from monoport_amd.implicit_seg.functional import Seg3dTopk
    res, budgets = [9, 17, 33], [0, 17 ** 3, 10 ** 9]
    with pytest.warns(UserWarning, match="clamped"):
        eng = Seg3dTopk(query_func=net["query_func"], resolutions=res, num_points=budgets,
                        clip_mins=[None, -0.25, -0.125], validate="first", **BOX).to(DEV)
    assert eng.num_points == [0, 17 ** 3, 33 ** 3]
    stats = []
    ref = topk_ref.seg3d_topk(body["gpu_query"], BMIN, BMAX, res, eng.num_points, [INF, 0.25, 0.125], stats=stats)
    assert 0 < stats[2] < 33 ** 3 - 17 ** 3
    cals = [body["cal"], torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(75))).to(DEV)]
    per_frame = []
    for i in range(eng.VALIDATE_CALLS + 1):  # validated calls, then a trusted one
        sdf = eng(feats=net["feats"], calib=cals[0])
        assert eng.last_path == "fused" and eng.last_status.tolist() == [1] + stats
        assert np.array_equal(sdf[0, 0].cpu().numpy().view(np.uint32), ref.view(np.uint32))
    per_frame = [eng(feats=net["feats"], calib=c) for c in cals]
    assert eng._agreed >= eng.VALIDATE_CALLS
    many = eng.forward_many([dict(feats=net["feats"], calib=c) for c in cals])
    assert eng.last_path == "fused" and len(many) == 2
    assert all(torch.equal(a, b) for a, b in zip(many, per_frame)) and not torch.equal(many[0], many[1])
    vol, status = eng.forward_async(feats=net["feats"], calib=cals[0])
    assert status.cpu().tolist() == [1] + stats and torch.equal(vol, per_frame[0][0, 0])
    # an empty scene: None from the level-at-a-time engine and from the fused one
    empty = Seg3dTopk(query_func=lambda points: torch.zeros(1, 1, points.shape[1], device=DEV), resolutions=res,
                      num_points=[0, 10, 10], **BOX).to(DEV)
    assert empty() is None and empty.last_status.tolist() == [0, 9 ** 3]
    past = oracle.pifu_calib(*syn.scene_camera(0))
    past[0, 0, 3] = 5.0  # the camera looks past the box
    assert eng(feats=net["feats"], calib=torch.from_numpy(past).to(DEV)) is None
    assert eng.last_path == "fused" and eng.last_status.tolist() == [0, 9 ** 3, 0, 0]


def test_seg3d_lossless_unchanged(ops, oracle, body, net):
    """The default engine on the same fixture: still the lossless schedule, bit for bit."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    res = [9, 17, 33, 65]
    for faster, path in ((True, "fused"), (False, "generic")):
        eng = Seg3dLossless(query_func=net["query_func"], resolutions=res, faster=faster, **BOX).to(DEV)
        sdf = eng(feats=net["feats"], calib=body["cal"])
        stats = []
        ref = oracle.seg3d_lossless(body["gpu_query"], BMIN, BMAX, res, stats=stats, faster=faster)
        assert eng.last_path == path and eng.last_status.tolist() == [1] + stats
        assert np.array_equal(sdf[0, 0].cpu().numpy(), ref)
    assert (eng.final_level, eng.fuse_views, eng.view, eng.validate) == ("dilate3", False, 0, "always")
