"""Multi-view reconstruction as one fused octree call (mp_recon_views, Seg3dLossless(fuse_views=True)): against the
reference's dense multi-view volume, bit for bit against the level-at-a-time engine on the same head, maps and
calibrations, and through the C-ABI.  Needs an MI355X.

Why "bit for bit" is derivable: both engines select the same nodes with the same housekeeping kernels, take their
world coordinates through the same f32 operation sequence (lattice_coord / lattice_points_kernel) and evaluate
each (point, view) column with the same kernel arithmetic; neither uses skip tables.  So the first level's values
are equal, hence the next level's node set, and so on."""
import ctypes
import warnings

import numpy as np
import pytest

import test_query_views_gpu as tv
from conftest import load_golden
from monoport_amd import synthetic as syn
from test_box_threshold_cpu import B_MAX, B_MIN
from test_query_batch_persp_gpu import persp_body_mlp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
FULL = [17, 33, 65, 129, 257]
UNIT_MIN, UNIT_MAX = np.array([[-1.0, -1, -1]]), np.array([[1.0, 1, 1]])
MP_ERR_ARG, MP_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops
    return ops


# ---- inputs: the recipe of the golden's DENSE_CASE (tools/gen_golden_query_views.py) for any V ---------------
_FEAT = {}


def body_maps(v_n):
    for v in range(v_n):
        if v not in _FEAT:
            _FEAT[v] = syn.body_feat(256, 128, 128, 252 + v)
    return np.stack([_FEAT[v] for v in range(v_n)])


def body_case(v_n, perspective=False):
    """-> (net, feats_stages, [V,4,4] calibs on the device)"""
    if perspective:
        layers = persp_body_mlp("G", 251, 0.05)
        yaws = [(0.1, np.sqrt(1 - 0.1 ** 2)), (0.0, 1.0), (-0.1, np.sqrt(1 - 0.1 ** 2))]
        calibs = tv.calibs_of(dict(proj="perspective", yaws=yaws[:v_n]))
    else:
        layers = syn.body_mlp("G", noise=0.05, seed=251)
        calibs = tv.calibs_of(dict(proj="orthogonal", steps=[6 * v for v in range(v_n)]))
    net = tv._net("G", layers, v_n, "perspective" if perspective else "orthogonal")
    feats = [[torch.zeros(v_n, 256, 2, 2, device=DEV)]] * 3 + [[torch.from_numpy(body_maps(v_n)).to(DEV)]]
    return net, feats, torch.from_numpy(calibs).to(DEV)


def view_query_func(net, v_n, row=0):
    def query_func(points, im_feat_list, calib_tensor):  # RTL/main.py:169-183, one row of get_preds()
        samples = points.repeat(v_n, 1, 1).permute(0, 2, 1)
        return net.query(im_feat_list, points=samples, calibs=calib_tensor)[0][row:row + 1]
    return query_func


def engine(query_func, resolutions, b_min=UNIT_MIN, b_max=UNIT_MAX, balance=0.5, **kw):
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    return Seg3dLossless(query_func=query_func, b_min=np.asarray(b_min).reshape(1, 3),
                         b_max=np.asarray(b_max).reshape(1, 3), resolutions=resolutions, balance_value=balance,
                         faster=True, **kw).to(DEV)


def same_bits(a, b):
    """torch.equal with NaN equal to NaN."""
    return bool(torch.equal(torch.isnan(a), torch.isnan(b))
                and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)))


def fused_and_generic(net, v_n, feats, calib, resolutions, row=0, view=0, **kw):
    """Both engines on the same inputs, warnings as errors -> (fused engine, its volume, generic engine, its volume)"""
    qf = view_query_func(net, v_n, row)
    ef = engine(qf, resolutions, fuse_views=True, view=view, **kw)
    eg = engine(qf, resolutions, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        vf = ef(im_feat_list=feats, calib_tensor=calib)
        vg = eg(im_feat_list=feats, calib_tensor=calib)
    assert ef.last_path == "fused" and eg.last_path == "generic"
    return ef, vf, eg, vg


# ---- 1. against the reference ---------------------------------------------------------------------------------
def test_fused_views_vs_dense_reference(ops):
    g = load_golden("views_dense65")
    case, layers, f, _, calibs = tv.case_inputs(g)
    v_n = case["V"]
    net = tv._net("G", layers, v_n)
    feats = [[torch.zeros(v_n, 256, 2, 2, device=DEV)]] * 3 + [[torch.from_numpy(f).to(DEV)]]
    eng = engine(view_query_func(net, v_n), tv.RES, fuse_views=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        vol = eng(im_feat_list=feats, calib_tensor=torch.from_numpy(calibs).to(DEV))
    assert eng.last_path == "fused"
    vol = vol[0, 0].cpu().numpy()
    ref = g["out"]
    firm = ~tv.undecided_reach(ref)
    assert firm.mean() > 0.5
    flips = int(((vol > 0.5) != (ref > 0.5))[firm].sum())
    print("views_dense65 fused: %d of %d firm nodes, %d thresholded nodes differ" % (int(firm.sum()), firm.size, flips))
    assert flips == 0


# ---- 2. fused == generic, bit for bit ---------------------------------------------------------------------------
CASES = {
    "V2": dict(v_n=2, res=FULL),
    "V3": dict(v_n=3, res=FULL),
    "V8": dict(v_n=8, res=FULL),
    "boxB_0.3": dict(v_n=3, res=FULL, b_min=B_MIN, b_max=B_MAX, balance=0.3),
    "perspective": dict(v_n=3, res=FULL, perspective=True),
    "upstream": dict(v_n=3, res=FULL[:3], final_level="upstream"),
    "interpolate": dict(v_n=3, res=FULL[:3], final_level="interpolate"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_generic_bitwise(ops, name):
    case = dict(CASES[name])
    v_n, res, balance = case.pop("v_n"), case.pop("res"), case.get("balance", 0.5)
    net, feats, calib = body_case(v_n, case.pop("perspective", False))
    ef, vf, eg, vg = fused_and_generic(net, v_n, feats, calib, res, **case)
    assert vf is not None and vg is not None
    sf, sg = ef.last_status.tolist(), eg.last_status.tolist()
    above = float((vf > balance).float().mean())
    print("%s: status fused %s generic %s, above the threshold %.4f, NaN %d"
          % (name, sf, sg, above, int(torch.isnan(vf).sum())))
    assert bool((vf > balance).any()) and bool((vf < balance).any())  # neither an empty nor a full scene
    if case.get("final_level") != "interpolate":
        assert sf[-1] > 0
    assert sf == sg
    assert same_bits(vf, vg) if name == "perspective" else torch.equal(vf, vg)


# ---- 3. row selection --------------------------------------------------------------------------------------------
def test_view_row_selection(ops):
    v_n = 3
    net, feats, calib = body_case(v_n)
    calib = calib.clone()
    calib[1, 0, 3] += 0.7  # view 1 partly off its image: rows 0 and 1 of the result differ
    p0 = ops.LevelEngine(DEV, UNIT_MIN[0], UNIT_MAX[0], FULL[:3]).select()  # the engines' coarsest lattice
    rows = net.query(feats, points=p0[None].repeat(v_n, 1, 1).permute(0, 2, 1), calibs=calib)[0]
    n_diff = int((rows[0] != rows[1]).sum())
    print("level-0 rows 0 / 1 differ in %d of %d nodes; above 0.5: %d / %d"
          % (n_diff, rows.shape[-1], int((rows[0] > 0.5).sum()), int((rows[1] > 0.5).sum())))
    assert n_diff > 0 and bool((rows[0] > 0.5).any()) and bool((rows[1] > 0.5).any())

    # the caller returns row 1 and says so: fused, equal to the generic result
    ef, vf, eg, vg = fused_and_generic(net, v_n, feats, calib, FULL[:3], row=1, view=1)
    assert torch.equal(vf, vg) and ef.last_status.tolist() == eg.last_status.tolist()
    row1 = vg.clone()

    # the caller returns row 1 under an engine that expects row 0: warning, generic engine, the row-1 volume
    eng = engine(view_query_func(net, v_n, row=1), FULL[:3], fuse_views=True, view=0)
    with pytest.warns(UserWarning, match="level-at-a-time"):
        vol = eng(im_feat_list=feats, calib_tensor=calib)
    assert eng.last_path == "generic" and torch.equal(vol, row1)
    _, v0, _, _ = fused_and_generic(net, v_n, feats, calib, FULL[:3], row=0, view=0)
    assert not torch.equal(v0, row1)

    # a row the head does not have
    eng = engine(view_query_func(net, v_n), FULL[:3], fuse_views=True, view=v_n)
    with pytest.raises(ValueError, match="view"):
        eng(im_feat_list=feats, calib_tensor=calib)


# ---- 4. C-ABI ----------------------------------------------------------------------------------------------------
def _abi_inputs(ops, v_n):
    layers = syn.body_mlp("G", noise=0.05, seed=251)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP["G"])
    fh = tv.pack_views(ops, body_maps(v_n))
    calibs = torch.from_numpy(tv.calibs_of(dict(proj="orthogonal", steps=[6 * v for v in range(v_n)]))).to(DEV)
    return mlp, fh, calibs


def test_abi_one_view_equals_recon(ops):
    mlp, fh, calibs = _abi_inputs(ops, 1)
    vol1, st1 = ops.recon_views(mlp, fh, calibs, "orthogonal", syn.Z_SCALE, UNIT_MIN[0], UNIT_MAX[0], FULL)
    vol0, st0 = ops.recon(mlp, fh[0], calibs[0:1], syn.Z_SCALE, UNIT_MIN[0], UNIT_MAX[0], FULL)
    print("one view: status %s / %s" % (st1.tolist(), st0.tolist()))
    assert st1.tolist() == st0.tolist() and st1[0] == 1 and st1[-1] > 0
    assert torch.equal(vol1, vol0) and bool((vol1 > 0.5).any())


def test_abi_counts_equal_generic_engine(ops):
    v_n = 3
    mlp, fh, calibs = _abi_inputs(ops, v_n)
    vol, st = ops.recon_views(mlp, fh, calibs, "orthogonal", syn.Z_SCALE, UNIT_MIN[0], UNIT_MAX[0], FULL)

    def query_func(points):
        pts = points[0].t()[None].expand(v_n, 3, points.shape[1])
        return ops.query_views(mlp, fh, pts, calibs, "orthogonal", syn.Z_SCALE)[:1]
    gen, counts = ops.recon_generic(query_func, {}, DEV, UNIT_MIN[0], UNIT_MAX[0], FULL)
    print("V = 3: status %s, generic counts %s" % (st.tolist(), counts))
    assert st.tolist() == [1] + counts and counts[-1] > 0
    assert torch.equal(vol, gen)


def _raw_call(ops, mlp, maps, cals, n_views, view, res, volume, status):
    ctx = mlp.ctx
    ptrs = ctypes.c_void_p * max(len(maps), 1)
    h, w, c = maps[0].shape
    bmin, bmax = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    return ctx.lib.mp_recon_views(
        ctx.handle, mlp.id, n_views, ptrs(*[m.data_ptr() for m in maps]), c, h, w,
        ptrs(*[cb.data_ptr() for cb in cals]), 0, float(syn.Z_SCALE), bmin, bmax, (ctypes.c_int * len(res))(*res),
        len(res), 0.5, 0, view, volume.data_ptr(), status.data_ptr(), None, None)


def test_abi_error_paths(ops):
    v_n = 3
    mlp, fh, calibs = _abi_inputs(ops, v_n)
    res = FULL[:3]
    good, good_st = ops.recon_views(mlp, fh, calibs, "orthogonal", syn.Z_SCALE, UNIT_MIN[0], UNIT_MAX[0], res)
    good, good_st = good.clone(), good_st.tolist()
    cals = [calibs[v].contiguous() for v in range(v_n)]
    volume = torch.empty((res[-1],) * 3, dtype=torch.float32, device=DEV)
    status = torch.empty((1 + len(res),), dtype=torch.int32, device=DEV)

    def still_serves():
        vol, st = ops.recon_views(mlp, fh, calibs, "orthogonal", syn.Z_SCALE, UNIT_MIN[0], UNIT_MAX[0], res)
        assert torch.equal(vol, good) and st.tolist() == good_st

    nine_m, nine_c = (fh * 3)[:9], (cals * 3)[:9]
    for what, rc, want in (
            ("0 views", lambda: _raw_call(ops, mlp, fh, cals, 0, 0, res, volume, status), MP_ERR_UNSUPPORTED),
            ("9 views", lambda: _raw_call(ops, mlp, nine_m, nine_c, 9, 0, res, volume, status), MP_ERR_UNSUPPORTED),
            ("view = V", lambda: _raw_call(ops, mlp, fh, cals, v_n, v_n, res, volume, status), MP_ERR_ARG),
            ("view = -1", lambda: _raw_call(ops, mlp, fh, cals, v_n, -1, res, volume, status), MP_ERR_ARG),
            ("17,33,64", lambda: _raw_call(ops, mlp, fh, cals, v_n, 0, [17, 33, 64], volume, status), MP_ERR_ARG)):
        assert rc() == want, what
        still_serves()
    mlp.set_precision("f16w")
    try:
        assert _raw_call(ops, mlp, fh, cals, v_n, 0, res, volume, status) == MP_ERR_UNSUPPORTED
        assert _raw_call(ops, mlp, fh[:1], cals[:1], 1, 0, res, volume, status) == MP_ERR_UNSUPPORTED
    finally:
        mlp.set_precision("f32")
    still_serves()
    with pytest.raises(ValueError):
        ops.recon_views(mlp, fh, calibs[:2], "orthogonal", syn.Z_SCALE, UNIT_MIN[0], UNIT_MAX[0], res)


# ---- 5. empty scene, async, trusted path --------------------------------------------------------------------------
def test_empty_scene_returns_none(ops):
    v_n = 3
    layers = syn.body_mlp("G", noise=0.05, seed=251)
    layers[-1][1][0] -= np.float32(30.0)  # sigmoid(y - 30): below the threshold everywhere
    net = tv._net("G", layers, v_n)
    feats = [[torch.zeros(v_n, 256, 128, 128, device=DEV)]]
    calib = torch.from_numpy(tv.calibs_of(dict(proj="orthogonal", steps=[0, 6, 12]))).to(DEV)
    eng = engine(view_query_func(net, v_n), FULL[:3], fuse_views=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert eng(im_feat_list=feats, calib_tensor=calib) is None
    assert eng.last_path == "fused" and eng.last_status[0] == 0 and eng.last_status[1] == 17 ** 3


def test_forward_async_equals_forward(ops):
    v_n = 3
    net, feats, calib = body_case(v_n)
    eng = engine(view_query_func(net, v_n), FULL[:4], fuse_views=True)
    vol = eng(im_feat_list=feats, calib_tensor=calib)
    status = eng.last_status.tolist()
    avol, astatus = eng.forward_async(im_feat_list=feats, calib_tensor=calib)
    assert avol.is_cuda and astatus.is_cuda
    assert torch.equal(avol, vol[0, 0]) and astatus.tolist() == status and status[-1] > 0


def test_trusted_path_keyed_by_views_and_view(ops):
    """validate="first": after VALIDATE_CALLS agreeing calls the trusted path serves the frame; a change of
    ``view`` or of V validates again (never rides on the old trust)."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    net3, feats3, calib3 = body_case(3)
    calib3 = calib3.clone()
    calib3[1, 0, 3] += 0.7  # rows 0 and 1 differ (test_view_row_selection)
    net2, feats2, calib2 = body_case(2)
    state = dict(net=net3, v_n=3, row=0)

    def query_func(points, im_feat_list, calib_tensor):
        samples = points.repeat(state["v_n"], 1, 1).permute(0, 2, 1)
        r = state["row"]
        return state["net"].query(im_feat_list, points=samples, calibs=calib_tensor)[0][r:r + 1]

    res = FULL[:3]
    fresh = {}
    for key, (net, v_n, row, feats, calib) in dict(a=(net3, 3, 0, feats3, calib3), b=(net3, 3, 1, feats3, calib3),
                                                   c=(net2, 2, 0, feats2, calib2)).items():
        fresh[key] = engine(view_query_func(net, v_n, row), res, fuse_views=True, view=row)(
            im_feat_list=feats, calib_tensor=calib).clone()
    assert not torch.equal(fresh["a"], fresh["b"])

    eng = engine(query_func, res, fuse_views=True, validate="first")
    trusted = []
    inner = eng._forward_trusted

    def spy(kwargs):
        out = inner(kwargs)
        trusted.append(out is not NotImplemented)
        return out
    eng._forward_trusted = spy
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for i in range(Seg3dLossless.VALIDATE_CALLS):
            vol = eng(im_feat_list=feats3, calib_tensor=calib3)
            assert not any(trusted) and eng.last_path == "fused" and torch.equal(vol, fresh["a"])
        vol = eng(im_feat_list=feats3, calib_tensor=calib3)
        assert trusted == [True] and eng.last_path == "fused" and torch.equal(vol, fresh["a"])
        # the caller switches to row 1 and says so: validated again, then served correctly
        trusted.clear()
        state["row"], eng.view = 1, 1
        vol = eng(im_feat_list=feats3, calib_tensor=calib3)
        assert not any(trusted) and eng.last_path == "fused" and torch.equal(vol, fresh["b"])
        # another head with V = 2 behind the same query_func
        trusted.clear()
        state.update(net=net2, v_n=2, row=0)
        eng.view = 0
        vol = eng(im_feat_list=feats2, calib_tensor=calib2)
        assert not any(trusted) and eng.last_path == "fused" and torch.equal(vol, fresh["c"])
