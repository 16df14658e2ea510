"""The counted, batched multi-view query (mp_query_views_counted_batch, csrc/query_views.hip with BATCH and without
LATTICE): row ``view`` of ops.query_views for n frames x V views in one launch, on point sets whose sizes are read
from device memory.  The reference of every comparison is ops.query_views on the same maps, calibrations and points,
as int32 bits.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn
from test_query_views_gpu import TOL_MODEL, TOL_REF, calibs_of, case_inputs, model_views, pack_views, persp_calib_yaw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
H, W, CAP = 16, 24, 200  # the smallest maps that still have a border and are not square
SENTINEL = 0x7FC12345    # a NaN payload no kernel writes: what untouched columns must still hold
ARG, UNSUPPORTED = -1, -3  # MP_ERR_ARG, MP_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops
    return ops


def bits(t):
    return t.contiguous().view(torch.int32)


def sentinel_outs(n, cout, cap=CAP):
    return [torch.full((cout, cap), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32) for _ in range(n)]


def count_vectors(n, g):
    """Per-frame counts drawn from {0, 1, G-1, G, G+1, 3G+2, cap}: every value in every frame (the seven rotations),
    zeros in the first, a middle and the last frame at once, and all frames zero."""
    s = [0, 1, g - 1, g, g + 1, 3 * g + 2, CAP]
    vecs = [[s[(f + r) % 7] for f in range(n)] for r in range(7)]
    zeros = [s[1 + f % 6] for f in range(n)]
    for f in (0, n // 2, n - 1):
        zeros[f] = 0
    return vecs + [zeros, [0] * n]


class Frames:
    """n frames of V views: their own maps [H,W,C], orthogonal calibrations and CAP points each.  ``shifted(view)``
    moves the calibration of view ``view`` of every frame sideways, so that part of the points leave that view's image
    and stay inside the others'."""

    def __init__(self, ops, kind, v_n, n, seed):
        self.ops, self.kind, self.v_n, self.n = ops, kind, v_n, n
        c = 256 if kind == "G" else 512
        self.mlp = ops.PackedMLP.from_layers(DEV, syn.rand_mlp(kind, seed, 2.0), syn.LAST_OP[kind])
        self.maps = [[ops.pack_features(torch.from_numpy(syn.rand_feat(c, H, W, seed + 100 * f + v))[None].to(DEV))
                      for v in range(v_n)] for f in range(n)]
        self.calibs = torch.from_numpy(np.stack([
            np.stack([calibs_of(dict(proj="orthogonal", steps=[(17 * f + 41 * v) % 360]))[0] for v in range(v_n)])
            for f in range(n)])).to(DEV)
        self.points = [torch.from_numpy(syn.rand_points(CAP, seed + 7 * f, 1.1)).to(DEV) for f in range(n)]

    def shifted(self, view):
        cal = self.calibs.clone()
        cal[:, view, 0, 3] += 0.7
        return cal

    def reference(self, cal):
        """[n][V,Cout,CAP]: ops.query_views per frame, the same points given to every view."""
        return [self.ops.query_views(self.mlp, self.maps[f], self.points[f][None].expand(self.v_n, 3, CAP), cal[f],
                                     "orthogonal", syn.Z_SCALE) for f in range(self.n)]

    def in_image(self, cal, f):
        """[V,CAP] bool on the host: which points of frame f each view sees, from the projections."""
        xyz = torch.stack([self.ops.orthogonal(self.points[f][None], cal[f, v:v + 1])[0] for v in range(self.v_n)])
        return ((xyz[:, 0].abs() <= 1) & (xyz[:, 1].abs() <= 1)).cpu().numpy()


@pytest.mark.parametrize("kind,v_n,n", [("C", 2, 1), ("C", 3, 5), ("C", 8, 8), ("G", 2, 10)])
def test_equals_query_views(ops, kind, v_n, n):
    fr = Frames(ops, kind, v_n, n, 900 + 10 * v_n + n)
    cout = fr.mlp.cout
    g = 64 // v_n
    for view in range(v_n):
        cal = fr.shifted(view)
        ref = fr.reference(cal)
        for f in range(n):
            seen = fr.in_image(cal, f)
            other = np.delete(seen, view, 0).any(0)
            assert int((~seen[view] & other).sum()) >= 20 and int((seen[view] & other).sum()) >= 20
            out_only = torch.from_numpy(~seen[view] & other).to(DEV)
            assert (ref[f][view][:, out_only] == 0).all()          # exact 0 outside view `view` ...
            assert (ref[f][1 - view if v_n == 2 else (view + 1) % v_n][:, out_only] != 0).any()  # ... and rows differ
        for counts in count_vectors(n, g):
            cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
            outs = sentinel_outs(n, cout)
            got = ops.query_views_counted_batch(fr.mlp, fr.maps, fr.points, [cnt[f:f + 1] for f in range(n)], cal,
                                                "orthogonal", syn.Z_SCALE, view=view, outs=outs)
            assert got is outs
            for f, k in enumerate(counts):
                assert torch.equal(bits(got[f][:, :k]), bits(ref[f][view][:, :k])), (view, counts, f)
                assert (bits(got[f][:, k:]) == SENTINEL).all(), (view, counts, f)
    # a fresh result: zeros behind the counts
    cnt = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    fresh = ops.query_views_counted_batch(fr.mlp, fr.maps, fr.points, [cnt[f:f + 1] for f in range(n)], fr.calibs,
                                          "orthogonal", syn.Z_SCALE)
    assert all(tuple(o.shape) == (cout, CAP) and (o[:, 5:] == 0).all() for o in fresh)


def test_perspective_poisons_every_row(ops):
    """A point with z == 0 in ONE view (x = 0, z = -3.75 under the (0.6, 0.8) yaw camera) is NaN in the written row
    whichever view is asked for; every other point is finite; the bits are ops.query_views'."""
    v_n, n = 3, 2
    mlp = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("C", 950, 2.0), syn.LAST_OP["C"])
    maps = [[ops.pack_features(torch.from_numpy(syn.rand_feat(512, H, W, 960 + 10 * f + v))[None].to(DEV))
             for v in range(v_n)] for f in range(n)]
    cal = torch.from_numpy(np.stack([persp_calib_yaw(0.6, 0.8), persp_calib_yaw(0.0, 1.0),
                                     persp_calib_yaw(-0.6, 0.8)]))[None].repeat(n, 1, 1, 1).to(DEV)
    points = []
    for f in range(n):
        p = syn.rand_points(CAP, 970 + f, 1.2)
        p[:, :4] = np.array([[0.0] * 4, [0.0, 0.5, -0.5, 0.25], [-3.75] * 4], np.float32)
        points.append(torch.from_numpy(p).to(DEV))
    counts = [CAP, 37]
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    ref = [ops.query_views(mlp, maps[f], points[f][None].expand(v_n, 3, CAP), cal[f], "perspective", syn.Z_SCALE)
           for f in range(n)]
    for view in range(v_n):
        got = ops.query_views_counted_batch(mlp, maps, points, [cnt[f:f + 1] for f in range(n)], cal, "perspective",
                                            syn.Z_SCALE, view=view, outs=sentinel_outs(n, 3))
        for f, k in enumerate(counts):
            nan = torch.isnan(got[f][:, :k])
            assert nan[:, :4].all() and not nan[:, 4:].any()
            assert torch.equal(bits(got[f][:, :k]), bits(ref[f][view][:, :k]))
            assert (bits(got[f][:, k:]) == SENTINEL).all()


@pytest.fixture(scope="module")
def golden_c(ops):
    g = load_golden("query_views_C_ortho")
    case, layers, f, p, calibs = case_inputs(g)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP["C"])
    fh = pack_views(ops, f)
    pts = torch.from_numpy(np.ascontiguousarray(p)).to(DEV)
    cal = torch.from_numpy(calibs).to(DEV)
    model = model_views(ops, layers, fh, pts[None].repeat(case["V"], 1, 1), cal, syn.LAST_OP["C"])
    return g, case, mlp, fh, pts, cal, model


@pytest.mark.parametrize("alone", [True, False])
def test_reference_fixture_c_ortho(ops, golden_c, alone):
    """The reference's query_views_C_ortho fixture (128^2 maps, capacity = count = 8192) as the only frame and as frame
    1 of 3 between two frames of other seeds."""
    g, case, mlp, fh, pts, cal, model = golden_c
    v_n, cap = case["V"], pts.shape[1]
    assert cap == 8192 and g["out"].shape[0] == v_n
    maps, points, cals, me = [fh], [pts], [cal], 0
    if not alone:
        other = [[ops.pack_features(torch.from_numpy(syn.rand_feat(512, 128, 128, 980 + 10 * k + v))[None].to(DEV))
                  for v in range(v_n)] for k in range(2)]
        maps, me = [other[0], fh, other[1]], 1
        points = [torch.from_numpy(syn.rand_points(cap, 990, 1.2)).to(DEV), pts,
                  torch.from_numpy(syn.rand_points(cap, 991, 1.2)).to(DEV)]
        cals = [cal.flip(0), cal, cal.roll(1, 0)]
    cnt = torch.tensor([cap - 11 * abs(f - me) for f in range(len(maps))], dtype=torch.int32, device=DEV)
    for view in (0, 1):
        out = ops.query_views_counted_batch(mlp, maps, points, [cnt[f:f + 1] for f in range(len(maps))], cals,
                                            "orthogonal", syn.Z_SCALE, view=view)[me].cpu().numpy()
        ref = g["out"][view]
        err = float(np.abs(out - ref).max())
        err_model = float(np.abs(out - model[view]).max())
        print("query_views_C_ortho view %d (%s): max |d| = %.3g vs the reference, %.3g vs float64"
              % (view, "alone" if alone else "frame 1 of 3", err, err_model))
        assert err <= TOL_REF
        assert np.array_equal(out == 0, ref == 0) and (ref == 0).all(0).sum() > 100
        assert err_model <= TOL_MODEL


def raw(mlp, n, v_n, maps, c, h, w, points, cap, counts, cals, projection, view, outs):
    arr = lambda ts: None if ts is None else (ctypes.c_void_p * len(ts))(*[t if t is None or isinstance(t, int)
                                                                         else t.data_ptr() for t in ts])
    return mlp.ctx.lib.mp_query_views_counted_batch(
        mlp.ctx.handle, mlp.id, n, v_n, arr(maps), c, h, w, arr(points), cap, arr(counts), arr(cals), projection,
        ctypes.c_float(syn.Z_SCALE), view, arr(outs), None)


def test_refusals(ops):
    from monoport_amd._lib import MonoportError
    v_n, n = 2, 2
    fr = Frames(ops, "C", v_n, n, 1000)
    mlp = fr.mlp
    cnt = torch.tensor([CAP, 70], dtype=torch.int32, device=DEV)
    counts = [cnt[0:1], cnt[1:2]]
    ref = fr.reference(fr.calibs)
    flat = [m for frame in fr.maps for m in frame]
    cals = [fr.calibs[f, v].contiguous() for f in range(n) for v in range(v_n)]
    outs = sentinel_outs(n, 3)

    def valid():
        for o in outs:
            o.view(torch.int32).fill_(SENTINEL)
        assert raw(mlp, n, v_n, flat, 512, H, W, fr.points, CAP, counts, cals, 0, 1, outs) == 0
        for f, k in enumerate((CAP, 70)):
            assert torch.equal(bits(outs[f][:, :k]), bits(ref[f][1][:, :k])) and (bits(outs[f][:, k:]) == SENTINEL).all()

    def untouched():
        torch.cuda.synchronize()
        assert all((bits(o) == SENTINEL).all() for o in outs)

    valid()
    for o in outs:
        o.view(torch.int32).fill_(SENTINEL)
    many = lambda ts, k: (list(ts) * k)[:k]
    refused = [
        (UNSUPPORTED, dict(v_n=0)), (UNSUPPORTED, dict(v_n=9, maps=many(flat, 18), cals=many(cals, 18))),
        (ARG, dict(n=0)), (ARG, dict(n=33, maps=many(flat, 66), cals=many(cals, 66), points=many(fr.points, 33),
                                    counts=many(counts, 33), outs=many(outs, 33))),
        (ARG, dict(view=-1)), (ARG, dict(view=2)), (ARG, dict(projection=2)), (ARG, dict(c=256)),
        (ARG, dict(h=0)), (ARG, dict(cap=-1)), (ARG, dict(maps=None)), (ARG, dict(points=None)), (ARG, dict(counts=None)),
        (ARG, dict(cals=None)), (ARG, dict(outs=None)),
        (ARG, dict(maps=flat[:3] + [None])), (ARG, dict(cals=cals[:3] + [None])), (ARG, dict(points=[fr.points[0], None])),
        (ARG, dict(counts=[counts[0], None])), (ARG, dict(outs=[outs[0], None])),
        (ARG, dict(maps=flat[:3] + [flat[3].data_ptr() + 4])), (ARG, dict(points=[fr.points[0], fr.points[1].data_ptr() + 2])),
        (ARG, dict(outs=[outs[0], outs[1].data_ptr() + 1])), (ARG, dict(counts=[counts[0], cnt.data_ptr() + 2])),
    ]
    base = dict(n=n, v_n=v_n, maps=flat, c=512, h=H, w=W, points=fr.points, cap=CAP, counts=counts, cals=cals,
                projection=0, view=1, outs=outs)
    for code, change in refused:
        assert raw(mlp, **dict(base, **change)) == code, change
        untouched()
    # n_frames x n_views beyond MP_MAX_FRAME_VIEWS: 9 frames of 8 views
    big = dict(n=9, v_n=8, maps=many(flat, 72), cals=many(cals, 72), points=many(fr.points, 9), counts=many(counts, 9),
               outs=many(outs, 9))
    assert raw(mlp, **dict(base, **big)) == ARG
    untouched()
    # capacity == 0: MP_OK before the frames' buffers are looked at
    assert raw(mlp, **dict(base, cap=0, points=[None, None], outs=[None, None], counts=[None, None])) == 0
    untouched()
    # a head that is not f32 (netG heads only have such precisions)
    g_mlp = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("G", 1001, 2.0), syn.LAST_OP["G"])
    g_maps = [ops.pack_features(torch.zeros((1, 256, H, W), device=DEV)) for _ in range(n * v_n)]
    g_outs = sentinel_outs(n, 1)
    g_mlp.set_precision("f16w")
    assert raw(g_mlp, **dict(base, maps=g_maps, c=256, outs=g_outs)) == UNSUPPORTED
    with pytest.raises(MonoportError, match="f32"):
        ops.query_views_counted_batch(g_mlp, [g_maps[:2], g_maps[2:]], fr.points, counts, fr.calibs, "orthogonal",
                                      syn.Z_SCALE, outs=g_outs)
    g_mlp.set_precision("f32")
    assert raw(g_mlp, **dict(base, maps=g_maps, c=256, outs=g_outs)) == 0
    # (C, Cout) outside the four built heads: no such head can be created to begin with
    dims = (ctypes.c_int * 6)(129, 1024, 512, 256, 128, 3)
    assert mlp.ctx.lib.mp_mlp_create(mlp.ctx.handle, 5, dims, 2, ctypes.byref(ctypes.c_int())) == UNSUPPORTED
    # through ops: what the C-ABI refuses raises, what Python can see raises ValueError before any device work
    for o in outs:
        o.view(torch.int32).fill_(SENTINEL)
    for view in (-1, 2):
        with pytest.raises(MonoportError, match="view"):
            ops.query_views_counted_batch(mlp, fr.maps, fr.points, counts, fr.calibs, "orthogonal", syn.Z_SCALE,
                                          view=view, outs=outs)
    with pytest.raises(ValueError, match="projection"):
        ops.query_views_counted_batch(mlp, fr.maps, fr.points, counts, fr.calibs, "fisheye", syn.Z_SCALE, outs=outs)
    with pytest.raises(ValueError, match="query_views_counted_batch"):
        ops.query_views_counted_batch(mlp, fr.maps, fr.points[:1], counts, fr.calibs, "orthogonal", syn.Z_SCALE)
    with pytest.raises(ValueError, match="query_views_counted_batch"):
        ops.query_views_counted_batch(mlp, [fr.maps[0]] * 33, [fr.points[0]] * 33, [counts[0]] * 33,
                                      [fr.calibs[0]] * 33, "orthogonal", syn.Z_SCALE)
    untouched()
    valid()
