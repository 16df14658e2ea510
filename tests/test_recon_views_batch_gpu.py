"""n frames x V views in one fused octree call (mp_recon_views_batch, the batched-lattice instantiation of
csrc/query_views.hip): frame f's volume and status against ops.recon_views on frame f's maps and calibrations, bit
for bit.  Needs an MI355X.

The reference is the per-frame call, which tests/test_recon_views_gpu.py holds to the reference's fixtures and to the
level-at-a-time engine.  "Bit for bit" is derivable: both calls run the same housekeeping kernels per frame, and the
batched kernel's tile IS the one-frame kernel's tile once its owner frame is looked up (a tile never spans two
frames), so level 0 agrees, hence the next level's node set, and so on.  What can go wrong is the lookup: tile
boundaries between frames, frames without nodes, the frame-major pointer tables.  So the frames differ in cameras AND
in maps, and the per-level counts are printed and held to differ between frames."""
import ctypes

import numpy as np
import pytest

import test_query_views_gpu as tv
import test_recon_views_gpu as rv
from conftest import load_golden
from monoport_amd import synthetic as syn
from test_box_threshold_cpu import B_MAX, B_MIN
from test_query_batch_persp_gpu import persp_body_mlp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
RES = [17, 33, 65]
FULL = rv.FULL
LO, HI = rv.UNIT_MIN[0], rv.UNIT_MAX[0]
MP_ERR_ARG, MP_ERR_UNSUPPORTED = -1, -3
FRAME_STEP = 7  # degrees of the orbit camera between consecutive frames


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops
    return ops


# ---- inputs -------------------------------------------------------------------------------------------------------
_CACHE = {}


def body_head(ops):
    if "head" not in _CACHE:
        _CACHE["head"] = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=251), syn.LAST_OP["G"])
    return _CACHE["head"]


def packed_body_maps(ops, v_n):
    """The V body maps of test_recon_views_gpu.body_case, channels-last on the device (made once per V)."""
    key = ("maps", v_n)
    if key not in _CACHE:
        _CACHE[key] = tv.pack_views(ops, rv.body_maps(v_n))
    return _CACHE[key]


def body_frames(ops, v_n, n):
    """n frames of V views: frame f sees the body maps in the order rotated by f (so the frames' map tables differ)
    from cameras 6 v + FRAME_STEP f degrees round the orbit -> (maps [n][V], calibs [n,V,4,4] on the device)."""
    m = packed_body_maps(ops, v_n)
    maps = [[m[(v + f) % v_n] for v in range(v_n)] for f in range(n)]
    calibs = np.stack([tv.calibs_of(dict(proj="orthogonal", steps=[6 * v + FRAME_STEP * f for v in range(v_n)]))
                       for f in range(n)])
    return maps, torch.from_numpy(calibs).to(DEV)


def per_frame(ops, mlp, maps, calibs, projection="orthogonal", res=RES, b_min=LO, b_max=HI, **kw):
    """The reference: ops.recon_views frame by frame -> [(volume, status list)]"""
    out = []
    for f in range(len(maps)):
        vol, st = ops.recon_views(mlp, maps[f], calibs[f], projection, syn.Z_SCALE, b_min, b_max, res, **kw)
        out.append((vol.clone(), st.tolist()))
    return out


def batched(ops, mlp, maps, calibs, projection="orthogonal", res=RES, b_min=LO, b_max=HI, **kw):
    vols, st = ops.recon_views_batch(mlp, maps, calibs, projection, syn.Z_SCALE, b_min, b_max, res, **kw)
    return vols, st.tolist()


def assert_frames_equal(vols, status, ref, what, nan_ok=False):
    for f, (rvol, rst) in enumerate(ref):
        assert status[f] == rst, "%s: status of frame %d: %s, per-frame call %s" % (what, f, status[f], rst)
        if rst[0] == 0:
            continue  # an empty coarsest level: the volume is unspecified
        same = rv.same_bits(vols[f], rvol) if nan_ok else torch.equal(vols[f], rvol)
        assert same, "%s: volume of frame %d differs from the per-frame call" % (what, f)


# ---- 1. views and frames ------------------------------------------------------------------------------------------
_REF = {}


def body_reference(ops, v_n, n):
    """Per-frame results of the first n body frames of V views: computed once per frame, shared by the batch sizes."""
    maps, calibs = body_frames(ops, v_n, n)
    have = _REF.setdefault(v_n, [])
    if len(have) < n:
        have += per_frame(ops, body_head(ops), maps[len(have):], calibs[len(have):])
    return maps, calibs, have[:n]


@pytest.mark.parametrize("v_n", [2, 3, 8])
@pytest.mark.parametrize("n", [1, 2, "max"])
def test_views_and_frames(ops, v_n, n):
    n = ops.max_view_frames(v_n) if n == "max" else n
    maps, calibs, ref = body_reference(ops, v_n, n)
    vols, status = batched(ops, body_head(ops), maps, calibs)
    print("V = %d (%d points per tile), %d frames: statuses %s" % (v_n, 64 // v_n, n, status))
    assert len(vols) == n and all(st[0] == 1 and min(st[1:]) > 0 for st in status)
    assert_frames_equal(vols, status, ref, "V=%d n=%d" % (v_n, n))
    if n >= 2:  # tile boundaries between frames at uneven places
        for level in range(1, len(RES)):
            assert len({st[1 + level] for st in status}) >= 2, "every frame has the same count at level %d" % level
    assert bool((vols[-1] > 0.5).any()) and bool((vols[-1] < 0.5).any())


# ---- 2. empty and odd frames ----------------------------------------------------------------------------------------
def odd_frames(ops):
    """(a) live, (b) camera `view` = 0 looks past the box: every value 0, (c) camera 1 looks past the box: live on
    zero-padded samples of that view, (d) = (a)."""
    maps, calibs = body_frames(ops, 3, 4)
    maps[3] = maps[0]
    calibs = calibs.clone()
    calibs[3] = calibs[0]
    calibs[1, 0, 0, 3] = 5.0
    calibs[2, 1, 0, 3] = 5.0
    return maps, calibs


def test_empty_and_odd_frames(ops):
    mlp = body_head(ops)
    maps, calibs = odd_frames(ops)
    ref = per_frame(ops, mlp, maps, calibs)
    vols, status = batched(ops, mlp, maps, calibs)
    print("live / away / other camera away / live again: %s" % status)
    assert status[1] == [0, 17 ** 3, 0, 0]
    assert status[2][0] == 1 and min(status[2][1:]) > 0 and status[2] != status[0]
    assert_frames_equal(vols, status, ref, "odd frames")
    assert status[3] == status[0] and torch.equal(vols[3], vols[0])
    live = [v.clone() for v in vols]

    # the empty frame first
    order = [1, 0, 2, 3]
    vols, status = batched(ops, mlp, [maps[i] for i in order], calibs[order])
    assert_frames_equal(vols, status, [ref[i] for i in order], "empty frame first")
    assert torch.equal(vols[1], live[0]) and torch.equal(vols[2], live[2])

    # nothing but empty frames: the call ends, and no finer level has a node
    vols, status = batched(ops, mlp, [maps[1]] * 3, calibs[[1, 1, 1]])
    torch.cuda.synchronize()
    assert status == [[0, 17 ** 3, 0, 0]] * 3


# ---- 3. variants ------------------------------------------------------------------------------------------------------
def test_variant_box_and_balance(ops):
    mlp = body_head(ops)
    maps, calibs = body_frames(ops, 3, 2)
    kw = dict(b_min=B_MIN, b_max=B_MAX, balance=0.3)
    ref = per_frame(ops, mlp, maps, calibs, **kw)
    vols, status = batched(ops, mlp, maps, calibs, **kw)
    print("off-centre box, balance 0.3: %s" % status)
    assert all(st[0] == 1 and st[-1] > 0 for st in status)
    assert_frames_equal(vols, status, ref, "box B")


def test_variant_perspective(ops):
    mlp = ops.PackedMLP.from_layers(DEV, persp_body_mlp("G", 251, 0.05), syn.LAST_OP["G"])
    m = packed_body_maps(ops, 3)
    maps = [m, [m[1], m[2], m[0]]]
    yaws = [[(s, np.sqrt(1 - s ** 2)) for s in (0.1, 0.0, -0.1)], [(s, np.sqrt(1 - s ** 2)) for s in (0.15, 0.05, -0.05)]]
    calibs = torch.from_numpy(np.stack([tv.calibs_of(dict(proj="perspective", yaws=y)) for y in yaws])).to(DEV)
    ref = per_frame(ops, mlp, maps, calibs, "perspective")
    vols, status = batched(ops, mlp, maps, calibs, "perspective")
    print("perspective: %s, NaN nodes %s" % (status, [int(torch.isnan(v).sum()) for v in vols]))
    assert all(st[0] == 1 and st[-1] > 0 for st in status)
    assert_frames_equal(vols, status, ref, "perspective", nan_ok=True)


@pytest.mark.parametrize("final_level", ["upstream", "interpolate"])
def test_variant_final_level(ops, final_level):
    mlp = body_head(ops)
    maps, calibs = body_frames(ops, 3, 2)
    ref = per_frame(ops, mlp, maps, calibs, final_level=final_level)
    vols, status = batched(ops, mlp, maps, calibs, final_level=final_level)
    print("%s: %s" % (final_level, status))
    assert all((st[-1] == 0) == (final_level == "interpolate") for st in status)
    assert_frames_equal(vols, status, ref, final_level)


def test_variant_view_row(ops):
    mlp = body_head(ops)
    maps, calibs = body_frames(ops, 3, 2)
    calibs = calibs.clone()
    calibs[:, 1, 0, 3] += 0.7  # view 1 partly off its image, as in test_view_row_selection
    ref1 = per_frame(ops, mlp, maps, calibs, view=1)
    ref0 = per_frame(ops, mlp, maps, calibs, view=0)
    assert not torch.equal(ref0[0][0], ref1[0][0])
    vols, status = batched(ops, mlp, maps, calibs, view=1)
    print("view 1: %s (view 0: %s)" % (status, [r[1] for r in ref0]))
    assert_frames_equal(vols, status, ref1, "view 1")


@pytest.mark.parametrize("h,w", [(48, 80), (80, 48)])
def test_variant_rect_maps(ops, h, w):
    """Random head and random maps of a non-square size (the inputs of tests/rect_cases.py's query cases): an
    exchanged (h, w) reads other texels in both calls alike, so this holds the batched launcher to the per-frame one."""
    v_n = 3
    mlp = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("G", 641, 2.0), syn.LAST_OP["G"])
    m = tv.pack_views(ops, np.stack([syn.rand_feat(256, h, w, 651 + v) for v in range(v_n)]))
    maps = [m, [m[2], m[0], m[1]]]
    calibs = torch.from_numpy(np.stack([tv.calibs_of(dict(proj="orthogonal", steps=[40 + 6 * v + FRAME_STEP * f
                                                                                   for v in range(v_n)]))
                                        for f in range(2)])).to(DEV)
    ref = per_frame(ops, mlp, maps, calibs)
    vols, status = batched(ops, mlp, maps, calibs)
    print("%d x %d maps: %s" % (h, w, status))
    assert all(st[0] == 1 and min(st[1:]) > 0 for st in status) and status[0] != status[1]
    assert_frames_equal(vols, status, ref, "%dx%d" % (h, w))


def test_variant_full_resolution(ops):
    mlp = body_head(ops)
    maps, calibs = body_frames(ops, 3, 2)
    ref = per_frame(ops, mlp, maps, calibs, res=FULL)
    vols, status = batched(ops, mlp, maps, calibs, res=FULL)
    print("17..257: %s" % status)
    assert all(st[0] == 1 and st[-1] > 0 for st in status) and status[0] != status[1]
    assert_frames_equal(vols, status, ref, "17..257")


# ---- 4. the reference's fixture ---------------------------------------------------------------------------------------
def test_fixture_frame_in_a_batch(ops):
    g = load_golden("views_dense65")
    case, layers, f, _, calibs = tv.case_inputs(g)
    v_n = case["V"]
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP["G"])
    m = tv.pack_views(ops, f)
    other = tv.calibs_of(dict(proj="orthogonal", steps=[9 + 11 * v for v in range(v_n)]))
    cal = torch.from_numpy(np.stack([other, calibs])).to(DEV)
    vols, status = batched(ops, mlp, [m[::-1], m], cal, case["proj"], res=tv.RES)
    vol = vols[1].cpu().numpy()
    ref = g["out"]
    firm = ~tv.undecided_reach(ref)
    assert firm.mean() > 0.5
    flips = int(((vol > 0.5) != (ref > 0.5))[firm].sum())
    print("views_dense65 as frame 1 of 2: status %s, %d of %d firm nodes, %d thresholded nodes differ"
          % (status, int(firm.sum()), firm.size, flips))
    assert flips == 0


# ---- 5. early hand-over -----------------------------------------------------------------------------------------------
def test_early_flags(ops):
    mlp = body_head(ops)
    maps, calibs = odd_frames(ops)
    n = len(maps)
    # what a caller's query_func returns on the coarsest lattice of each frame: row 0 of the multi-view query on the
    # level-at-a-time engine's level-0 points, scattered into [r0,r0,r0] (what Seg3dLossless.forward hands over)
    level0 = []
    for f in range(n):
        eng = ops.LevelEngine(DEV, LO, HI, RES)
        p0 = eng.select()
        pts = p0.t()[None].expand(len(maps[f]), 3, p0.shape[0])
        eng.scatter(ops.query_views(mlp, maps[f], pts, calibs[f], "orthogonal", syn.Z_SCALE)[:1])
        level0.append(eng.cur.clone())
    ref = per_frame(ops, mlp, maps, calibs)
    early = ops.EarlyFlags(DEV, n)
    vols, status = batched(ops, mlp, maps, calibs, early=early, expect_level0=level0)
    flags = early.wait().clone().tolist()
    print("early flags %s" % flags)
    assert flags == [[1, 0], [0, 0], [1, 0], [1, 0]]
    assert_frames_equal(vols, status, ref, "early")
    wrong = [v.clone() for v in level0]
    wrong[2][3, 4, 5] += 0.25
    vols, status = batched(ops, mlp, maps, calibs, early=early, expect_level0=wrong)
    assert early.wait().clone().tolist() == [[1, 0], [0, 0], [1, 1], [1, 0]]
    assert_frames_equal(vols, status, ref, "early, one expectation perturbed")
    with pytest.raises(ValueError):
        batched(ops, mlp, maps, calibs, early=ops.EarlyFlags(DEV, n - 1))


# ---- 6. dirty arena ---------------------------------------------------------------------------------------------------
def test_dirty_arena(ops):
    mlp = body_head(ops)
    maps, calibs = odd_frames(ops)
    vols, status = batched(ops, mlp, maps, calibs)  # sizes the stream's arena
    first = [v.clone() for v in vols]
    again, status2 = batched(ops, mlp, maps, calibs)
    assert status2 == status and all(torch.equal(a, b) for a, b in zip(again, first))
    for byte in (0x00, 0xFF, 0x7F, 0x5A):
        assert ops.scratch_fill(DEV, 0, byte) > 0
        vols, st = batched(ops, mlp, maps, calibs)
        assert st == status, "arena filled with 0x%02X: %s, clean %s" % (byte, st, status)
        for f in range(len(maps)):
            if status[f][0]:
                assert torch.equal(vols[f], first[f]), "arena filled with 0x%02X: frame %d" % (byte, f)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def _raw_call(mlp, maps, cals, n_frames, n_views, view, res, volumes, status):
    ctx = mlp.ctx
    ptrs = lambda ts: (ctypes.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])  # noqa: E731
    h, w, c = maps[0].shape
    bmin, bmax = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    return ctx.lib.mp_recon_views_batch(
        ctx.handle, mlp.id, n_frames, n_views, ptrs(maps), c, h, w, ptrs(cals), 0, float(syn.Z_SCALE), bmin, bmax,
        (ctypes.c_int * len(res))(*res), len(res), 0.5, 0, view, ptrs(volumes), ptrs(status), None, None)


def test_refusals(ops):
    mlp = body_head(ops)
    v_n, n = 3, 2
    maps, calibs = body_frames(ops, v_n, n)
    good = per_frame(ops, mlp, maps, calibs)

    def still_serves():
        vols, status = batched(ops, mlp, maps, calibs)
        assert_frames_equal(vols, status, good, "after a refusal")

    flat = [m for frame in maps for m in frame]
    cals = [calibs[f, v].contiguous() for f in range(n) for v in range(v_n)]
    many_m, many_c = (flat * 11)[:65], (cals * 11)[:65]
    volumes = [torch.empty((RES[-1],) * 3, dtype=torch.float32, device=DEV) for _ in range(33)]
    status = [torch.empty((1 + len(RES),), dtype=torch.int32, device=DEV) for _ in range(33)]

    def call(n_frames, n_views, view=0, res=RES, m=flat, c=cals):
        return _raw_call(mlp, m, c, n_frames, n_views, view, res, volumes, status)

    assert mlp.ctx.lib.mp_max_frame_views() == 64 == ops.MAX_FRAME_VIEWS
    for what, rc, want in (
            ("0 views", lambda: call(n, 0), MP_ERR_UNSUPPORTED),
            ("9 views", lambda: call(1, 9, m=many_m, c=many_c), MP_ERR_UNSUPPORTED),
            ("view = V", lambda: call(n, v_n, view=v_n), MP_ERR_ARG),
            ("view = -1", lambda: call(n, v_n, view=-1), MP_ERR_ARG),
            ("17,33,64", lambda: call(n, v_n, res=[17, 33, 64]), MP_ERR_ARG),
            ("resolution 1", lambda: call(n, v_n, res=[1]), MP_ERR_ARG),
            ("0 frames", lambda: call(0, v_n), MP_ERR_ARG),
            ("33 frames of 1 view", lambda: call(33, 1, m=many_m, c=many_c), MP_ERR_ARG),
            ("13 frames x 5 views = 65", lambda: call(13, 5, m=many_m, c=many_c), MP_ERR_ARG),
            ("22 frames x 3 views = 66", lambda: call(22, 3, m=(flat * 11), c=(cals * 11)), MP_ERR_ARG)):
        assert rc() == want, what
        assert b"mp_recon_views_batch" in mlp.ctx.lib.mp_last_error(mlp.ctx.handle), what
        still_serves()
    mlp.set_precision("f16w")
    try:
        assert call(n, v_n) == MP_ERR_UNSUPPORTED
        assert call(1, 1) == MP_ERR_UNSUPPORTED
    finally:
        mlp.set_precision("f32")
    still_serves()
    netc = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("C", 7, 1.0), syn.LAST_OP["C"])
    maps512 = [torch.zeros((8, 8, 512), device=DEV)] * (n * v_n)
    assert _raw_call(netc, maps512, cals, n, v_n, 0, RES, volumes, status) == MP_ERR_UNSUPPORTED
    still_serves()

    with pytest.raises(ValueError):  # frames and calibration sets
        ops.recon_views_batch(mlp, maps, calibs[:1], "orthogonal", syn.Z_SCALE, LO, HI, RES)
    with pytest.raises(ValueError):  # a frame with fewer views
        ops.recon_views_batch(mlp, [maps[0], maps[1][:2]], calibs, "orthogonal", syn.Z_SCALE, LO, HI, RES)
    with pytest.raises(ValueError):  # views and calibrations of a frame
        ops.recon_views_batch(mlp, maps, [calibs[0], calibs[1][:2]], "orthogonal", syn.Z_SCALE, LO, HI, RES)
    with pytest.raises(ValueError):  # volumes
        ops.recon_views_batch(mlp, maps, calibs, "orthogonal", syn.Z_SCALE, LO, HI, RES, volumes=volumes[:1])
    with pytest.raises(ValueError):  # above the cap: 22 x 3
        ops.recon_views_batch(mlp, [maps[0]] * 22, [calibs[0]] * 22, "orthogonal", syn.Z_SCALE, LO, HI, RES)
    still_serves()


# ---- 8. one frame, one view -------------------------------------------------------------------------------------------
def test_one_frame_one_view_equals_recon(ops):
    mlp = body_head(ops)
    maps, calibs = body_frames(ops, 1, 2)
    vols, status = batched(ops, mlp, maps[:1], calibs[:1], res=FULL)
    vol0, st0 = ops.recon(mlp, maps[0][0], calibs[0, 0:1], syn.Z_SCALE, LO, HI, FULL)
    print("one frame, one view: %s / %s" % (status, st0.tolist()))
    assert status[0] == st0.tolist() and st0[0] == 1 and st0[-1] > 0
    assert torch.equal(vols[0], vol0) and bool((vol0 > 0.5).any())
    # and two frames of one view each against the single-view batched call on the plain kernels
    vols, status = batched(ops, mlp, maps, calibs)
    vb, sb = ops.recon_batch(mlp, [m[0] for m in maps], calibs[:, 0], syn.Z_SCALE, LO, HI, RES)
    assert status == sb.tolist() and all(torch.equal(a, b) for a, b in zip(vols, vb))
