"""The texel sort of an octree level's point list (csrc/point_order.hip): mp_octree_order_points alone, the fused
reconstruction with and without it (MONOPORT_OCTREE_ORDER unset / y / z), and the frame whose list does not fit the
temporary list.  Inputs: lattices of 9, 17 and 33 nodes on 17 / 65 / 33-final grids (strides 2, 4, 1), a 16 x 24 map,
three frames per call -- the identity camera, the benchmark's tilt at a 45 degree orbit and a perspective camera that
has nodes behind the eye -- and a scratch arena filled with 0x5A beforehand (mp_scratch_fill).

The keys are restated in numpy float32 in the kernel's operation order (lattice_coord, project_row's FMA chain,
the perspective divisions, in_image, make_taps); an FMA is restated as one float64 product and sum rounded to float32,
which can differ from the fused operation in the last bit, so a point whose pixel coordinate lies within 1e-4 of an
integer (a "border point") may land in the neighbouring cell: the number of key runs along the sorted list may exceed
the number of distinct keys by two per border point, and the cameras are chosen so that border points (counted in
float64) stay at or below 1 % of each frame's lattice.

The temporary list holds r^3 / 8 entries: a list of the FULL lattice exceeds it and is, by the entry's definition,
left exactly as it was -- that is what the full-lattice count checks here; the sortedness checks run at 0, 1, 31,
32, 33 points and at the cap itself, r^3 // 8 (and r^3 // 8 + 1 is the first count left alone).  The purpose check
(fewer distinct cells per 32 consecutive entries than in the input order) runs on the 17- and 33-node lattices: the 91
points the 9-node lattice may sort are two tiles spread over as many cells as points, where no order can gather
anything.  Needs an MI355X."""
import numpy as np
import pytest

import rect_cases as rc
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
H, W = 16, 24
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
LATTICES = [(9, 17), (17, 65), (33, 33)]  # (nodes per axis, final resolution): strides 2, 4, 1
PERSP = dict(focal=0.8, depth=0.9)  # z_cam = 0.6 x + 0.8 z + 0.9 over the box: -0.5 .. 2.3
SENTINEL = np.uint32(0xFFFFFFFF)  # no node code: z would be 4095
DIRTY = 0x5A
RES = [9, 17, 33, 65]  # the fused tests: the last level is the one launch_recon sorts (kOrderMinRes = 65)


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cameras(oracle):
    """-> ([3][4,4] f32 calibrations, projections)"""
    return ([np.eye(4, dtype=np.float32), oracle.pifu_calib(*syn.scene_camera(45))[0], rc.persp_calib(**PERSP)[0]],
            ["orthogonal", "orthogonal", "perspective"])


# ---- the key, restated ---------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def keys_f32(codes, calib, proj, r, rf):
    """The kernel's texel_key in numpy float32, operation by operation."""
    f = np.float32
    stride = (rf - 1) // (r - 1)
    half = (f(1.0) / f(rf)) / f(2.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = [((((codes >> s) & 1023) * stride).astype(f) / f(rf) + half) * f(BMAX[i] - BMIN[i]) + f(BMIN[i])
             for i, s in enumerate((0, 10, 20))]
        row = lambda k: calib[k, 3] + _fma32(np.full_like(p[2], calib[k, 2]), p[2],
                                             _fma32(np.full_like(p[1], calib[k, 1]), p[1], calib[k, 0] * p[0]))
        x, y, z = row(0), row(1), row(2)
        if proj == "perspective":
            x, y = x / z, y / z
        inside = (x >= -1) & (x <= 1) & (y >= -1) & (y <= 1)
        ix = ((x + f(1.0)) * f(0.5)) * f(W - 1)
        iy = ((y + f(1.0)) * f(0.5)) * f(H - 1)
        x0 = np.clip(np.nan_to_num(np.floor(ix), nan=0.0, posinf=W, neginf=-2), 0, W - 1).astype(np.int64)
        y0 = np.clip(np.nan_to_num(np.floor(iy), nan=0.0, posinf=H, neginf=-2), 0, H - 1).astype(np.int64)
    return np.where(inside, y0 * W + x0, H * W)


def border_f64(codes, calib, proj, r, rf):
    """Points whose pixel coordinate (float64) lies within 1e-4 of an integer, or that have no finite one."""
    stride = (rf - 1) // (r - 1)
    c = calib.astype(np.float64)
    p = np.stack([(((codes >> s) & 1023) * stride / rf + 0.5 / rf) * (BMAX[i] - BMIN[i]) + BMIN[i]
                  for i, s in enumerate((0, 10, 20))])
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y, z = (c[k, :3] @ p + c[k, 3] for k in range(3))
        if proj == "perspective":
            x, y = x / z, y / z
        ix, iy = (x + 1) * 0.5 * (W - 1), (y + 1) * 0.5 * (H - 1)
        near = (np.abs(ix - np.round(ix)) < 1e-4) | (np.abs(iy - np.round(iy)) < 1e-4)
    return near | ~np.isfinite(ix) | ~np.isfinite(iy)


def runs(keys):
    return int(1 + (np.diff(keys) != 0).sum()) if keys.size else 0


def cells_per_tile(keys, tile=32):
    n = keys.shape[0] // tile * tile
    k = np.sort(keys[:n].reshape(-1, tile), axis=1)
    return float((1 + (np.diff(k, axis=1) != 0).sum(1)).mean())


def lattice_codes(r):
    """Every node of an r^3 lattice in z-major order (z, y, x)."""
    z, y, x = np.meshgrid(np.arange(r), np.arange(r), np.arange(r), indexing="ij")
    return (x | (y << 10) | (z << 20)).reshape(-1).astype(np.uint32)


def run_order(ops, lists, calibs, projs, r, rf):
    """mp_octree_order_points on host lists (one per frame) in buffers of r^3 + 8 entries whose tail holds SENTINEL, on
    a dirty arena -> (the buffers afterwards, the counts afterwards)."""
    bufs, counts = [], []
    for codes in lists:
        b = np.full(r ** 3 + 8, SENTINEL, np.uint32)
        b[:codes.size] = codes
        bufs.append(dev(b.view(np.int32)))
        counts.append(torch.tensor([codes.size], dtype=torch.int32, device=DEV))
    ops.scratch_fill(DEV, 1 << 20, DIRTY)
    ops.octree_order_points(bufs, counts, [dev(c) for c in calibs], r, (rf - 1) // (r - 1), rf, BMIN, BMAX, H, W,
                            projections=projs)
    return [b.cpu().numpy().view(np.uint32) for b in bufs], [int(c.item()) for c in counts]


def assert_sorted(out, codes, calib, proj, r, rf, what):
    n = codes.size
    assert np.array_equal(np.sort(out[:n]), np.sort(codes)), what  # a permutation of the input
    assert (out[n:] == SENTINEL).all(), what
    k = keys_f32(out[:n].astype(np.int64), calib, proj, r, rf)
    border = int(border_f64(codes.astype(np.int64), calib, proj, r, rf).sum())
    assert runs(k) <= np.unique(k).size + 2 * border, (what, runs(k), np.unique(k).size, border)
    return k


# ---- 1. the entry alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,rf", LATTICES)
def test_border_points_stay_below_one_percent(oracle, r, rf):
    """The condition of the run bound, on the CPU: per camera, border points are at most 1 % of the lattice."""
    codes = lattice_codes(r).astype(np.int64)
    for calib, proj in zip(*cameras(oracle)):
        share = float(border_f64(codes, calib, proj, r, rf).mean())
        print("lattice %d on %d, %s: %.3f %% border points" % (r, rf, proj, 100 * share))
        assert share <= 0.01


@pytest.mark.parametrize("r,rf", LATTICES)
def test_order_points_alone(ops, oracle, r, rf):
    calibs, projs = cameras(oracle)
    full = lattice_codes(r)
    cap = r ** 3 // 8
    for count in (0, 1, 31, 32, 33, cap, cap + 1, r ** 3):
        # frame f: a seeded subset of the lattice in z-major order (the full lattice: all of it)
        lists = [np.sort(np.random.RandomState(100 * r + f).permutation(full)[:count]) for f in range(3)]
        outs, counts = run_order(ops, lists, calibs, projs, r, rf)
        assert counts == [count] * 3
        for f in range(3):
            what = (r, rf, count, f)
            if count > cap:  # does not fit the temporary list: left exactly as it was
                assert np.array_equal(outs[f][:count], lists[f]) and (outs[f][count:] == SENTINEL).all(), what
                continue
            k = assert_sorted(outs[f], lists[f], calibs[f], projs[f], r, rf, what)
            if count == cap and r >= 17:  # what the sort is for
                before = cells_per_tile(keys_f32(lists[f].astype(np.int64), calibs[f], projs[f], r, rf))
                after = cells_per_tile(k)
                print("lattice %d on %d frame %d: %.2f -> %.2f distinct cells per 32 entries" % (r, rf, f, before, after))
                assert after < before, what
    # mixed counts in one call, the perspective frame alone, and the behind-the-eye nodes are really there
    lists = [full[:33], full[:0], np.sort(np.random.RandomState(7).permutation(full)[:cap])]
    outs, _ = run_order(ops, lists, calibs, projs, r, rf)
    for f in range(3):
        assert_sorted(outs[f], lists[f], calibs[f], projs[f], r, rf, ("mixed", r, f))
    k = keys_f32(full.astype(np.int64), calibs[2], projs[2], r, rf)
    assert (k == H * W).sum() > 0 and (k < H * W).sum() > 0


def test_a_frame_over_the_cap_keeps_its_order_and_the_others_are_sorted(ops, oracle):
    """Alternating z planes of the 33-node level (17 * 33 * 33 = 18513 nodes > 33^3 / 8 = 4492) in the middle frame."""
    r, rf = 33, 33
    calibs, projs = cameras(oracle)
    full = lattice_codes(r)
    cap = r ** 3 // 8
    planes = full[((full >> 20) & 1) == 0]
    assert planes.size > cap
    lists = [np.sort(np.random.RandomState(11).permutation(full)[:cap]), planes,
             np.sort(np.random.RandomState(12).permutation(full)[:cap // 2])]
    outs, counts = run_order(ops, lists, calibs, projs, r, rf)
    assert counts == [l.size for l in lists]
    assert np.array_equal(outs[1][:planes.size], planes) and (outs[1][planes.size:] == SENTINEL).all()
    for f in (0, 2):
        k = assert_sorted(outs[f], lists[f], calibs[f], projs[f], r, rf, f)
        assert not np.array_equal(outs[f][:lists[f].size], lists[f])
        assert cells_per_tile(k) < cells_per_tile(keys_f32(lists[f].astype(np.int64), calibs[f], projs[f], r, rf))


# ---- 2. fused reconstruction ----------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32)


def fused_inputs(ops, oracle, planes_of_frame1=None):
    """Three 16 x 24 body maps (random features, the depth planes in channels 0 / 1; the perspective frame's planes
    moved to its camera distance), one seeded noisy head, the three cameras."""
    calibs, projs = cameras(oracle)
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=31), 1)
    maps = []
    for f in range(3):
        m = syn.body_feat(256, H, W, 40 + f)
        if f == 2:
            m[0:2] += np.float32(PERSP["depth"])
        if f == 1 and planes_of_frame1 is not None:
            m[0:2] = planes_of_frame1
        maps.append(ops.pack_features(dev(m)[None]))
    return mlp, maps, [dev(c[None]) for c in calibs], projs


def recon_under(ops, monkeypatch, order, mlp, maps, cals, projs, single=False):
    if order is None:
        monkeypatch.delenv("MONOPORT_OCTREE_ORDER", raising=False)
    else:
        monkeypatch.setenv("MONOPORT_OCTREE_ORDER", order)
    ops.scratch_fill(DEV, 64 << 20, DIRTY)
    if not single:
        return ops.recon_batch(mlp, maps, cals, syn.Z_SCALE, BMIN, BMAX, RES, projections=projs)
    got = [ops.recon(mlp, maps[f], cals[f], syn.Z_SCALE, BMIN, BMAX, RES, projection=projs[f]) for f in range(3)]
    return [g[0] for g in got], torch.stack([g[1] for g in got])


@pytest.mark.parametrize("table", [True, False])
def test_fused_recon_is_the_same_under_every_order(ops, oracle, table, monkeypatch):
    from test_rect_maps_gpu import registered
    mlp, maps, cals, projs = fused_inputs(ops, oracle)
    with registered(ops, mlp, maps, table):
        runs_ = {o: recon_under(ops, monkeypatch, o, mlp, maps, cals, projs) for o in (None, "y", "z")}
        single = recon_under(ops, monkeypatch, None, mlp, maps, cals, projs, single=True)
    status = runs_[None][1].cpu().tolist()
    print("fused recon table %s: status %s" % (table, status))
    for f in range(3):  # every frame has a body and a sorted last level within the cap
        assert status[f][0] == 1 and 32 < status[f][-1] <= RES[-1] ** 3 // 8, status[f]
    for vols, st in list(runs_.values())[1:] + [single]:
        assert torch.equal(st, runs_[None][1])
        for f in range(3):
            assert torch.equal(bits(vols[f]), bits(runs_[None][0][f])), f
    assert not torch.equal(bits(runs_[None][0][0]), bits(runs_[None][0][1]))


# ---- 3. the cap inside the fused call -------------------------------------------------------------------------------
def test_fused_recon_with_a_frame_over_the_cap(ops, oracle, monkeypatch):
    """Frame 1's depth planes alternate by texel row between "inside over the whole depth" and "empty": under the
    benchmark's tilted camera the boundary shell of the 65-node level is most of the lattice, more than 65^3 / 8 nodes.
    The call equals MONOPORT_OCTREE_ORDER=y bit for bit; the other two frames stay within the cap (sorted)."""
    from test_rect_maps_gpu import registered
    planes = np.empty((2, H, W), np.float32)
    planes[0, 0::2], planes[1, 0::2] = 4.0, -4.0   # z_back < z < z_front everywhere in the box
    planes[0, 1::2], planes[1, 1::2] = -4.0, 4.0   # empty
    mlp, maps, cals, projs = fused_inputs(ops, oracle, planes)
    cap = RES[-1] ** 3 // 8
    with registered(ops, mlp, maps, True):
        vols, st = recon_under(ops, monkeypatch, None, mlp, maps, cals, projs)
        vols_y, st_y = recon_under(ops, monkeypatch, "y", mlp, maps, cals, projs)
    status = st.cpu().tolist()
    print("fused recon, frame 1 over the cap of %d: status %s" % (cap, status))
    assert status[1][-1] > cap and 32 < status[0][-1] <= cap and 32 < status[2][-1] <= cap
    assert torch.equal(st, st_y)
    for f in range(3):
        assert torch.equal(bits(vols[f]), bits(vols_y[f])), f
