"""The lossless octree housekeeping kernels (csrc/octree.hip) through the C-ABI on adversarial inputs:
mp_octree_select_box / mp_octree_select, mp_octree_conflicts, mp_lattice_points and mp_scatter_nodes against the numpy
restatement of the header's definition (tests/octree_ref.py), in both list orders (MONOPORT_OCTREE_ORDER), at
resolutions off the 2^k + 1 pattern, with ragged last words, volumes that touch every face, arbitrary evaluated sets,
counts below the capacity, values on the threshold and NaNs; then ops.LevelEngine and the fused ops.recon on fields and
boxes whose body reaches the faces of the box.  Every comparison is exact: the selected set (``packed[:count]`` sorted
-- the order of the list is unspecified), bits of volumes, bitsets and counts.  tests/test_octree_ref_cpu.py holds
the restatement to oracle.seg3d_lossless and shows that these inputs discriminate.  Needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest

import octree_ref as orf
import test_box_threshold_gpu as box_gpu
from monoport_amd import synthetic as syn
from oracle import pifu_oracle as po  # numpy parts only here; the built oracle is the `oracle` fixture
from test_box_threshold_cpu import B_MAX, B_MIN
from test_box_threshold_gpu import _check_recon, body  # noqa: F401  (body: that file's scene, as a fixture here)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
MP_OK = 0
POISON = -12345.0
IPOISON = -777
ORDERS = ["y", "z"]
# a box shrunk around the body of the `body` scene: the body crosses its faces
SHRUNK_MIN = np.array([-0.3, -0.5, -0.2], np.float32)
SHRUNK_MAX = np.array([0.25, 0.45, 0.15], np.float32)


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def abi(ops):
    """(library, context handle, stream) of the C-ABI."""
    ctx = ops.get_context(torch.device(DEV))
    return ctx.lib, ctx.handle, ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


@pytest.fixture()
def order(request, monkeypatch):
    """The list order of the selection kernels: the default (slabs of y outermost) or MONOPORT_OCTREE_ORDER=z."""
    if request.param == "z":
        monkeypatch.setenv("MONOPORT_OCTREE_ORDER", "z")
    else:
        monkeypatch.delenv("MONOPORT_OCTREE_ORDER", raising=False)
    return request.param


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _float3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in np.asarray(v, np.float32).reshape(3)])


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV)


def _full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device=DEV)


# ---- a. mp_octree_select_box against select_level --------------------------------------------------------------
def _gpu_select(abi, prev, ev_prev, box=None, balance=0.5, level=None, r=None):
    """One mp_octree_select_box (``box``) or mp_octree_select (``level``) call on poisoned outputs.  ``prev`` None:
    level 0 at resolution ``r``."""
    lib, h, st = abi
    if prev is not None:
        rp = prev.shape[0]
        r = 2 * rp - 1
        d_prev, d_evp = _dev(prev), _dev(orf.pack_bits(ev_prev))
    else:
        rp, d_prev, d_evp = 0, None, None
    words = r * r * ((r + 63) // 64)
    cur = _full((r, r, r), POISON, torch.float32)
    bnd = _full((words,), IPOISON, torch.int64)
    ev_cur = _full((words,), IPOISON, torch.int64)
    packed = _full((r ** 3,), IPOISON, torch.int32)
    count = _full((1,), IPOISON, torch.int32)
    fn, arg = (lib.mp_octree_select_box, box) if level is None else (lib.mp_octree_select, level)
    rc = fn(h, _p(d_prev), rp, _p(cur), r, _p(d_evp), _p(ev_cur), _p(bnd), int(arg), float(balance), _p(packed),
            _p(count), st)
    assert rc == MP_OK, lib.mp_last_error(h).decode()
    return dict(r=r, n=int(count.item()), cur=cur.cpu().numpy(), bnd=bnd.cpu().numpy().view(np.uint64),
                ev=ev_cur.cpu().numpy().view(np.uint64), packed=packed.cpu().numpy())


@functools.lru_cache(maxsize=4)
def _volume(name, rp):
    prev, ev_prev = orf.VOLUMES[name](rp, rp)
    return prev, ev_prev


@functools.lru_cache(maxsize=4)  # the list order varies fastest: both orders of a case share one
def _reference(name, rp, box, balance):
    """select_level of the volume, computed once and shared by both list orders."""
    cur, flags, sel, ev_after = orf.select_level(*_volume(name, rp), box, balance)
    return cur, flags, orf.mask_codes(sel), orf.pack_bits(ev_after)


def _assert_select(got, want, what):
    cur, flags, sel_codes, ev_words = want
    r, n = got["r"], got["n"]
    nan = np.isnan(cur)
    assert np.array_equal(np.isnan(got["cur"]), nan), what  # sign and payload of a NaN are not part of the contract
    assert np.array_equal(got["cur"].view(np.uint32)[~nan], cur.view(np.uint32)[~nan]), what
    assert np.array_equal(orf.unpack_bits(got["bnd"], r)[0], flags), what
    assert np.array_equal(got["ev"], ev_words), what  # pad bits zero
    assert n == sel_codes.size, (what, n, sel_codes.size)
    listed = np.sort(got["packed"][:n].astype(np.int64))
    assert np.array_equal(listed, sel_codes), what  # sel_codes is strictly ascending: no node twice
    assert (got["packed"][n:] == IPOISON).all(), what  # nothing is written behind the count


def _check_select(abi, name, rp, box, balance=0.5):
    got = _gpu_select(abi, *_volume(name, rp), box=box, balance=balance)
    _assert_select(got, _reference(name, rp, box, balance), (name, rp, box, balance))
    return got


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("box", [9, 7, 3, 1, 0])
@pytest.mark.parametrize("name", ["noise", "faces", "sparse", "plateau"])
@pytest.mark.parametrize("rp", [2, 3, 5, 12, 32, 33])
def test_select_box_matches_restatement(abi, rp, name, box, order):
    """r = 3 (narrower than every box), 5, 9, 23, 63 (a ragged single word) and 65 (a second word of one bit)."""
    got = _check_select(abi, name, rp, box)
    if box == 0:
        assert got["n"] == 0
    elif rp >= 12:
        assert 0 < got["n"] < got["r"] ** 3


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("box", [9, 7, 3, 1, 0])
def test_select_box_balance_off_half(abi, box, order):
    """balance 0.3 on the noise volume: a third of the nodes is inside instead of 3 %."""
    _check_select(abi, "noise", 33, box, 0.3)
    if box:
        assert not np.array_equal(_reference("noise", 33, box, 0.3)[1], _reference("noise", 33, box, 0.5)[1])


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("box", [9, 3, 1])
@pytest.mark.parametrize("name", ["noise", "seam"])
@pytest.mark.parametrize("rp", [64, 65, 66])
def test_select_box_across_word_boundaries(abi, rp, name, box, order):
    """r = 127 (a ragged second word), 129 (a third word of one bit) and 131 (of three bits): carries between the
    words of a row, both halves of the previous level's evaluated words."""
    got = _check_select(abi, name, rp, box)
    assert 0 < got["n"] < got["r"] ** 3


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("rp", [64, 65, 66])
def test_select_box_7_on_the_seam(abi, rp, order):
    _check_select(abi, "seam", rp, 7)


def test_list_order_follows_the_environment(abi, monkeypatch):
    """The variable is read on every call and switches to the z-major kernels: the same set in another order."""
    lists = {}
    for order in ORDERS:
        if order == "z":
            monkeypatch.setenv("MONOPORT_OCTREE_ORDER", "z")
        else:
            monkeypatch.delenv("MONOPORT_OCTREE_ORDER", raising=False)
        got = _check_select(abi, "noise", 33, 3)
        lists[order] = got["packed"][:got["n"]]
        lists[order, 0] = _gpu_select(abi, None, None, box=3, r=9)["packed"]
    assert not np.array_equal(lists["y"], lists["z"]) and not np.array_equal(lists["y", 0], lists["z", 0])


# ---- b. mp_octree_select, the level form -----------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("level,box", [(1, 9), (2, 7), (3, 3), (5, 3)])
def test_select_level_form_uses_the_box_of_the_level(abi, level, box, order):
    for name, rp in (("noise", 33), ("faces", 12)):
        got = _gpu_select(abi, *_volume(name, rp), level=level)
        _assert_select(got, _reference(name, rp, box, 0.5), (name, rp, level))
        same = _gpu_select(abi, *_volume(name, rp), box=box)
        assert got["n"] == same["n"] and np.array_equal(np.sort(got["packed"]), np.sort(same["packed"]))
        assert np.array_equal(got["ev"], same["ev"]) and np.array_equal(got["bnd"], same["bnd"])
        assert np.array_equal(got["cur"].view(np.uint32), same["cur"].view(np.uint32))


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("r", [2, 9, 63, 65])
def test_select_level_zero_lists_every_node(abi, r, order):
    for form in ("level", "box"):
        got = _gpu_select(abi, None, None, r=r, **(dict(level=0) if form == "level" else dict(box=3)))
        assert got["n"] == r ** 3
        assert np.array_equal(np.sort(got["packed"].astype(np.int64)), orf.mask_codes(np.ones((r, r, r), bool)))
        assert np.array_equal(got["ev"], orf.pack_bits(np.ones((r, r, r), bool)))  # pad bits zero


# ---- c. mp_octree_conflicts against conflicts ---------------------------------------------------------------------
def _conflict_case(r, balance, seed):
    """(codes [capacity], values [capacity], n, vol, ev): a hand-built list of n = 2/3 capacity nodes, then poison."""
    rng = np.random.default_rng(seed)
    m = r // 2
    below, above = np.float32(balance * 0.5), np.float32(balance + 0.3)
    vol = (below * (np.float32(0.5) + rng.random((r, r, r), dtype=np.float32))).astype(np.float32)  # all < balance
    nodes, values = [], []

    def add(x, y, z, value, interp=None):
        if interp is not None:
            vol[z, y, x] = interp
        nodes.append(x | (y << 10) | (z << 20))
        values.append(value)

    flip = 0
    for z in (0, r - 1):  # the eight corners: neighbourhoods of 8 nodes
        for y in (0, r - 1):
            for x in (0, r - 1):
                flip ^= 1
                if flip:
                    add(x, y, z, above)
                else:  # the interpolated value above, the exact one below
                    add(x, y, z, below, above)
    for x, y, z in ((m, m, 0), (m, m, r - 1), (m, 0, m), (m, r - 1, m), (0, m, m), (r - 1, m, m)):  # face centres
        add(x, y, z, above)
    if r >= 65:  # neighbours in the other word of the row
        add(63, 3, m - 3, above)
        add(64, m + 5, 3, below, above)
    if r >= 129:
        add(127, 5, m + 9, above)
        add(128, m - 9, 5, above)
    add(m - 2, m + 2, m, above)  # two adjacent conflicts: 18 shared neighbours, each claimed once
    add(m - 1, m + 2, m, above)
    add(m - 2, m + 2, m, above)  # and the first of them a second time
    on_threshold = (m + 2, 2, m - 2)
    add(*on_threshold, np.float32(balance))  # a factor of exactly 0: no conflict
    add(2, 2, m + 2, np.float32(np.nan))  # NaN: no conflict
    add(m, 2, m + 2, below)  # both below
    add(2, m + 2, 2, above, above)  # both above
    if len(nodes) % 2:
        add(2, m - 2, 2, below)
    n = len(nodes)
    capacity = n * 3 // 2
    tail = (m + 2) | ((m - 2) << 10) | ((m + 2) << 20)  # an isolated node below the threshold: a conflict if read
    codes = np.array(nodes + [tail] * (capacity - n), np.int64)
    vals = np.array(values + [above] * (capacity - n), np.float32)
    ev = rng.random((r, r, r)) < 0.3
    return codes, vals, n, vol, ev, on_threshold


def _gpu_conflicts(abi, codes, vals, n, vol, ev, balance, capacity=None):
    lib, h, st = abi
    r = vol.shape[0]
    capacity = codes.size if capacity is None else capacity
    d_codes, d_vals, d_vol = _dev(codes.astype(np.int32)), _dev(vals), _dev(vol)
    d_count = _dev(np.array([n], np.int32))
    d_ev = _dev(orf.pack_bits(ev))
    out = _full((r ** 3,), IPOISON, torch.int32)
    out_count = _full((1,), IPOISON, torch.int32)
    rc = lib.mp_octree_conflicts(h, _p(d_codes), _p(d_count), capacity, r, _p(d_vals) if capacity else None, _p(d_vol),
                                 float(balance), _p(d_ev), _p(out), _p(out_count), st)
    assert rc == MP_OK, lib.mp_last_error(h).decode()
    assert np.array_equal(d_vol.cpu().numpy().view(np.uint32), vol.view(np.uint32))  # read only
    return int(out_count.item()), out.cpu().numpy(), d_ev.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("balance", [0.5, 0.3])
@pytest.mark.parametrize("r", [9, 65, 129])
def test_conflicts_match_restatement(abi, r, balance):
    codes, vals, n, vol, ev, on_threshold = _conflict_case(r, balance, r)
    assert codes.size * 2 == n * 3
    want, ev_after = orf.conflicts(codes[:n], vals[:n], vol, ev, balance)
    x, y, z = on_threshold
    assert vals[:n].tolist().count(float(np.float32(balance))) == 1
    assert not ev[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2].all() and not (ev_after & ~ev)[z, y - 1:y + 2, x - 1:x + 2].any()
    if_read = orf.conflicts(codes, vals, vol, ev, balance)[0]
    assert if_read.size > want.size > 100  # the poison behind the count would be noticed
    n_out, out, ev_words = _gpu_conflicts(abi, codes, vals, n, vol, ev, balance)
    assert n_out == want.size
    assert np.array_equal(np.sort(out[:n_out].astype(np.int64)), want)  # strictly ascending: each node claimed once
    assert (out[n_out:] == IPOISON).all()
    assert np.array_equal(ev_words, orf.pack_bits(ev_after))
    # a count above the capacity is cut at the capacity
    n_out, out, ev_words = _gpu_conflicts(abi, codes, vals, codes.size, vol, ev, balance, capacity=n)
    assert n_out == want.size and np.array_equal(np.sort(out[:n_out].astype(np.int64)), want)
    assert np.array_equal(ev_words, orf.pack_bits(ev_after))


def test_conflicts_with_no_capacity(abi):
    codes, vals, n, vol, ev, _ = _conflict_case(9, 0.5, 1)
    n_out, out, ev_words = _gpu_conflicts(abi, codes, vals, n, vol, ev, 0.5, capacity=0)
    assert n_out == 0 and (out == IPOISON).all() and np.array_equal(ev_words, orf.pack_bits(ev))


# ---- d. mp_lattice_points and mp_scatter_nodes ---------------------------------------------------------------------
EXTREME_XYZ = [(1022, 1022, 1022), (1022, 0, 1022), (0, 1022, 0), (0, 0, 1022), (1022, 0, 0), (1022, 1022, 0),
               (0, 0, 0), (1, 2, 3), (511, 512, 513), (1, 1022, 1021)]


@pytest.mark.parametrize("res_final", [129, 161, 1023])
@pytest.mark.parametrize("stride", [1, 2, 16])
def test_lattice_points_decode_every_field(abi, stride, res_final):
    """Codes up to the 10-bit limit in every field, each axis with its own extreme (no volume is needed): bit for bit
    oracle.lattice_points on box B; rows past the count stay as they were.  One case has more nodes than the
    2048 blocks of the launch hold threads."""
    lib, h, st = abi
    rng = np.random.default_rng(stride * 10000 + res_final)
    many = 560000 if (stride, res_final) == (1, 1023) else 2300
    xyz = np.concatenate([np.array(EXTREME_XYZ, np.int64), rng.integers(0, 1023, (many, 3))])
    n, capacity = xyz.shape[0], xyz.shape[0] + 700
    codes = xyz[:, 0] | (xyz[:, 1] << 10) | (xyz[:, 2] << 20)
    d_codes = _dev(np.r_[codes, np.full(capacity - n, 1022 | (1022 << 10) | (1022 << 20))].astype(np.uint32).view(np.int32))
    d_count = _dev(np.array([n], np.int32))
    pts = _full((capacity, 3), POISON, torch.float32)
    rc = lib.mp_lattice_points(h, _p(d_codes), _p(d_count), capacity, stride, res_final, _float3(B_MIN),
                               _float3(B_MAX), _p(pts), st)
    assert rc == MP_OK, lib.mp_last_error(h).decode()
    got = pts.cpu().numpy()
    want = po.lattice_points(xyz[:, ::-1], stride, res_final, B_MIN, B_MAX).T
    assert np.array_equal(got[:n].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert (got[n:] == np.float32(POISON)).all()
    assert len({tuple(row) for row in got[:6].tolist()}) == 6
    rc = lib.mp_lattice_points(h, _p(d_codes), _p(d_count), 0, stride, res_final, _float3(B_MIN),
                               _float3(B_MAX), None, st)
    assert rc == MP_OK


@pytest.mark.parametrize("r", [65, 129])
def test_scatter_nodes_stops_at_the_count(abi, r):
    lib, h, st = abi
    rng = np.random.default_rng(r)
    vol = rng.random((r, r, r), dtype=np.float32)
    fixed = [0, r ** 3 - 1, 63, 64, r * r * (r - 1) + 63, r * (r - 1) + 64, r - 1]  # corners, both sides of x = 64
    # at r = 129 more nodes than the 2048 blocks of the launch hold threads
    lin = np.unique(np.r_[fixed, rng.choice(r ** 3, 3000 if r == 65 else 900000, replace=False)])
    lin = rng.permutation(lin)
    capacity = lin.size
    n = capacity * 2 // 3
    z, y, x = np.unravel_index(lin, (r, r, r))
    codes = (x | (y << 10) | (z << 20)).astype(np.int64)
    vals = (rng.random(capacity, dtype=np.float32) + np.float32(2)).astype(np.float32)
    vals[1] = np.nan
    want = vol.copy()
    want.reshape(-1)[lin[:n]] = vals[:n]
    d_vol, d_codes, d_vals = _dev(vol), _dev(codes.astype(np.int32)), _dev(vals)
    d_count = _dev(np.array([n], np.int32))
    rc = lib.mp_scatter_nodes(h, _p(d_codes), _p(d_count), capacity, r, _p(d_vals), _p(d_vol), st)
    assert rc == MP_OK, lib.mp_last_error(h).decode()
    got = d_vol.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))  # rows past the count ignored, the rest untouched
    assert (got.reshape(-1)[lin[n:]] < 1).all() and np.isnan(got.reshape(-1)[lin[1]])


# ---- e. the level-at-a-time engine on analytic fields ----------------------------------------------------------------
def _host_query(field):
    """query_func of the engine: the points go to the host, the numpy field back -- the values the reference sees."""
    def query_func(points):  # [1,N,3] on the device -> [1,1,N]
        p = points[0].cpu().numpy()
        return torch.from_numpy(field(p.T)).to(points.device)[None, None]
    return query_func


def _drive_engine(ops, field, res, faster, final_level):
    """ops.recon_generic's loop, keeping the engine: (volume, counts, rounds)."""
    eng = ops.LevelEngine(DEV, B_MIN, B_MAX, res, 0.5, faster, final_level)
    q = _host_query(field)
    eng.scatter(q(eng.select()[None]))
    assert not eng.empty()
    for _ in range(1, len(res)):
        pts = eng.select()
        while pts is not None:
            pts = eng.scatter(q(pts[None]))
    return eng.cur.cpu().numpy(), eng.counts, eng.rounds


ENGINE_CASES = [("fin", res, faster, rule)
                for res in ([6, 11, 21, 41, 81], [12, 23, 45, 89])
                for faster, rule in ((True, "dilate3"), (True, "upstream"), (True, "interpolate"), (False, "dilate3"))]
ENGINE_CASES += [("corner", [2, 3, 5, 9, 17, 33], faster, "dilate3") for faster in (True, False)]


@pytest.mark.parametrize("name,res,faster,final_level", ENGINE_CASES,
                         ids=lambda v: "r%d" % v[0] if isinstance(v, list) else str(v))
def test_engine_on_analytic_fields(ops, name, res, faster, final_level):
    """A body on four faces of box B (a sheet thinner than the coarse spacing: several conflict rounds per level) and
    a ball around a corner from 2 nodes per side on: volume bits, counts and rounds of oracle.seg3d_lossless."""
    field = orf.FIELDS[name]
    stats, rounds = [], []
    ref = po.seg3d_lossless(field, B_MIN, B_MAX, res, stats=stats, rounds=rounds, faster=faster,
                            final_level=final_level)
    assert ref is not None
    vol, counts, eng_rounds = _drive_engine(ops, field, res, faster, final_level)
    print("%s %s faster=%s %s: counts %s rounds %s" % (name, res, faster, final_level, counts, eng_rounds))
    assert counts == stats and eng_rounds == rounds
    assert np.array_equal(vol.view(np.uint32), ref.view(np.uint32))
    if name == "fin":
        assert orf.faces_reached(ref > np.float32(0.5)) >= 4
        if not faster:
            assert max(rounds) >= (2 if res[0] == 6 else 1)
    v2, counts2 = ops.recon_generic(_host_query(field), {}, DEV, B_MIN, B_MAX, res, faster=faster,
                                    final_level=final_level)
    assert counts2 == stats and np.array_equal(v2.cpu().numpy().view(np.uint32), ref.view(np.uint32))


# ---- f. the fused path off the 2^k + 1 pattern ---------------------------------------------------------------------
OFF_PATTERN = [[12, 23, 45, 89], [6, 11, 21, 41, 81, 161], [3, 5, 9, 17, 33]]


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("balance", [0.5, 0.3])
@pytest.mark.parametrize("res", OFF_PATTERN, ids=lambda r: "r%d" % r[0])
def test_fused_recon_off_the_pattern(ops, oracle, body, res, balance, order, monkeypatch):
    """[3, 5, ...] on B puts none of its 27 coarsest nodes into the body: both sides stop there (its levels run on
    the shrunk box below)."""
    monkeypatch.setattr(ops, "SKIP_TABLE", False)
    if res[0] == 3:
        stats = []
        assert oracle.seg3d_lossless(body["gpu_query"], B_MIN, B_MAX, res, balance_value=balance, stats=stats) is None
        _, status = ops.recon(body["mlp"], body["fh"], body["cal"], syn.Z_SCALE, B_MIN, B_MAX, res, balance)
        assert status.cpu().numpy().tolist() == [0] + stats + [0] * (len(res) - 1) == [0, 27, 0, 0, 0, 0]
        return
    v, st = _check_recon(ops, oracle, body["mlp"], body["fh"], body["cal"], body["gpu_query"], balance, res=res)
    assert (v > np.float32(balance)).sum() > 100 and all(s > 0 for s in st[1:])


@pytest.mark.parametrize("order", ORDERS, indirect=True)
def test_fused_recon_on_a_box_the_body_leaves(ops, oracle, body, order, monkeypatch):
    """A box shrunk around the body: inside voxels on the faces of the volume, where the dilation is clipped; from 3
    nodes per side too, a level narrower than the 9^3 box."""
    monkeypatch.setattr(ops, "SKIP_TABLE", False)
    monkeypatch.setattr(box_gpu, "B_MIN", SHRUNK_MIN)
    monkeypatch.setattr(box_gpu, "B_MAX", SHRUNK_MAX)
    for res, balance in (([12, 23, 45, 89], 0.5), ([12, 23, 45, 89], 0.3), ([3, 5, 9, 17, 33], 0.5),
                         ([3, 5, 9, 17, 33], 0.3)):
        v, st = _check_recon(ops, oracle, body["mlp"], body["fh"], body["cal"], body["gpu_query"], balance, res=res)
        assert all(s > 0 for s in st[1:])
        # v is the reference's volume bit for bit; on B itself the body touches no face (test_box_threshold_cpu.py)
        assert orf.faces_reached(v > np.float32(balance)) >= 4


def test_recon_batch_off_the_pattern_equals_single_frames(ops, oracle, body):
    res = [12, 23, 45, 89]
    feats, cals = [], []
    for i in range(3):
        feats.append(ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2 + i))[None].to(DEV)))
        cals.append(torch.from_numpy(oracle.pifu_calib(*syn.scene_camera(30 + 25 * i))).to(DEV))
    vols, status = ops.recon_batch(body["mlp"], feats, cals, syn.Z_SCALE, B_MIN, B_MAX, res, 0.3)
    st = status.cpu().numpy()
    assert (st[:, 0] == 1).all() and len({tuple(row) for row in st[:, 1:].tolist()}) == 3
    for i in range(3):
        v1, s1 = ops.recon(body["mlp"], feats[i], cals[i], syn.Z_SCALE, B_MIN, B_MAX, res, 0.3)
        assert np.array_equal(s1.cpu().numpy(), st[i]), i
        assert torch.equal(v1.view(torch.int32), vols[i].view(torch.int32)), i
