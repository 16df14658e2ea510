"""Every head the f32 query kernels admit -- C in {256, 512} x Cout in {1, 3} x last_op in {none, sigmoid, tanh} --
on every kernel family, against float64 (inputs and references: tests/head_cases.py, whose conditions
tests/test_query_heads_cpu.py asserts).  Needs an MI355X.

Which case reaches which instantiation (all 12 heads = every (C, Cout) line x every last_op):

  test_fused_query                 launch_query_set: pifu_query_kernel<C,Cout,WPS,false> (64-point tiles), all 12 heads;
                                   C = 256 also forced onto query_small.hip's 32-point kernel <Cout>, same bits
  test_direct_mlp                  launch_query_set, direct: pifu_query_kernel<C,Cout,WPS,true>, all 12 heads
  test_surface_classifier_default  the same <512,1,1,true> through SurfaceClassifier(last_op=None)
  test_batched_and_counted_forms   mp_query_batch / mp_query_counted / mp_query_counted_batch on the four (C, Cout)
                                   pairs, last_op = none (device counts: both f32 kernels of C = 256 read them)
  test_skip_table_query            launch_query_tab: pifu_query_tabws_kernel<Cout>, Cout {1, 3} x every last_op
  test_query_views                 launch_query_views: pifu_query_views_kernel<C,Cout,WPS,false>, V = 2, 3, all 12 heads
  test_one_view_is_plain_query     the same with V = 1, all 12 heads
  test_forward_views_*             launch_query_views, direct: <C,Cout,WPS,true>; V = 1 all 12 heads, V = 2 four pairs
  test_views_counted_batch         launch_query_views_counted_batch: all four (C, Cout) lines, every last_op
  test_octree_512_1                the octree-lattice form of pifu_query_kernel<512,1,1,false> (mp_recon)

Bars.  Bounded activations: the project's |gpu - f32 oracle| <= 2e-5 and |gpu - f64| <= max(2 y32, 1e-5), y32 = the
float32 oracle's own error on the case.  last_op = none: |gpu - f64| <= 2 Y0, Y0 = the largest y32 over the linear
cases of that C, computed here from the oracle.  The multi-view cases take the float32 torch-CPU evaluation of the
model as their oracle.  Everything else is exactly 0 (points outside the image) or bit equality.

Measured on an MI355X, max |gpu - f64| over the cases of each row (the yardsticks are recomputed by every run; the
multi-view ones depend a little on the CPU's BLAS):
  Y0 (oracle float32 vs float64, linear heads)        C = 256: 5.84e-6          C = 512: 9.54e-6
  Y0 of the multi-view model (torch float32)          C = 256: 3.73e-6          C = 512: 3.71e-6
  fused, last_op = none                               C = 256: 5.96e-6          C = 512: 8.70e-6   (bar 2 Y0)
  fused, sigmoid / tanh                               C = 256: 3.65e-6          C = 512: 4.72e-6   (y32 <= 4.6e-6)
  skip table, last_op = none / bounded                C = 256: 6.20e-6 / 4.63e-6; |table - plain| <= 2.0e-6
  direct, last_op = none                              C = 256: 2.27e-6          C = 512: 1.61e-6   (bar 2 Y0)
  SurfaceClassifier(), (512, 1, none)                 1.28e-6
  multi-view V = 2, last_op = none / bounded          C = 256: 3.41e-6 / 2.26e-6   C = 512: 4.34e-6 / 2.39e-6
  multi-view V = 3, last_op = none / bounded          C = 256: 2.74e-6 / 2.01e-6   C = 512: 2.79e-6 / 2.79e-6
  mlp_forward_views V = 2, last_op = none             C = 256: 1.07e-6          C = 512: 9.06e-7   (bar 2 Y0)
The fused error is the float32 projection's and sampling's (the direct form, fed the same float32 features, is 3-5
times closer): no case came nearer than 0.58 of its bar, and no instantiation was found wrong.
"""
import contextlib

import numpy as np
import pytest

import head_cases as hc
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
TOL_ORACLE = 2e-5  # tests/test_query_gpu.py: against the float32 oracle
FLOOR64 = 1e-5     # tests/test_query_gpu.py: err <= max(2 * reference's own error, 1e-5)
N = hc.N
CAP = 264          # capacity of the counted forms
SENTINEL = -7.5
UNIT_BOX = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


@contextlib.contextmanager
def small_gate(mode):
    """mp_query_tune: 0 = 64-point tiles, 1 = 32-point tiles, -1 = the default gate."""
    from monoport_amd import _lib
    lib = _lib.load()
    lib.mp_query_tune(mode)
    try:
        yield
    finally:
        lib.mp_query_tune(-1)


class Scene:
    """Device copies of the head_cases scenes, heads and single-call results, made once and shared."""

    def __init__(self, ops):
        self.ops = ops
        self._mlp, self._maps, self._pts, self._cal, self._plain, self._direct, self._x = {}, {}, {}, {}, {}, {}, {}

    def mlp(self, head):
        if head not in self._mlp:
            c, cout, last_op = head
            self._mlp[head] = self.ops.PackedMLP.from_layers(DEV, hc.layers_of(c, cout), last_op)
        return self._mlp[head]

    def maps(self, c):
        if c not in self._maps:
            f, p, calibs = hc.scene_views(c)
            self._maps[c] = [self.ops.pack_features(torch.from_numpy(f[v].copy())[None].to(DEV)) for v in range(hc.MAX_V)]
            self._pts[c] = torch.from_numpy(p.copy()).to(DEV)
            self._cal[c] = torch.from_numpy(calibs.copy()).to(DEV)
        return self._maps[c]

    def pts(self, c):
        self.maps(c)
        return self._pts[c]  # [3,N]

    def calibs(self, c):
        self.maps(c)
        return self._cal[c]  # [MAX_V,4,4]

    def plain(self, head, view=0):
        """ops.query of view ``view``'s map and calibration: [Cout,N] on the device."""
        if (head, view) not in self._plain:
            c = head[0]
            out = self.ops.query(self.mlp(head), self.maps(c)[view], self.pts(c)[None], self.calibs(c)[view], syn.Z_SCALE)
            assert out.shape == (1, head[1], N)
            self._plain[head, view] = out[0].clone()
        return self._plain[head, view]

    def x(self, c, v_n=1):
        if (c, v_n) not in self._x:
            self._x[c, v_n] = torch.from_numpy(np.stack([hc.direct_features(c, v) for v in range(v_n)])).to(DEV)
        return self._x[c, v_n]  # [V,C+1,N]

    def direct(self, head):
        if head not in self._direct:
            out = self.ops.mlp_forward(self.mlp(head), self.x(head[0]))
            assert out.shape == (1, head[1], N)
            self._direct[head] = out[0].clone()
        return self._direct[head]


@pytest.fixture(scope="module")
def scene(ops):
    return Scene(ops)


def check_against_oracle(what, head, out, ref64, ref32, y_case, y_linear, inside):
    """The bars of this file on one [.., Cout, N] result (numpy).  ref32 None: no float32 oracle for this form."""
    last_op = head[2]
    assert out.shape == ref64.shape and np.isfinite(out).all()
    assert (out[..., ~inside] == 0).all() and (out[..., inside] != 0).all()
    err64 = float(np.abs(out - ref64).max())
    if last_op == 0:
        print("%s %s: |gpu-f64| %.3g, Y0 %.3g (this case's y32 %.3g)" % (what, hc.head_id(head), err64, y_linear, y_case))
        assert err64 <= 2 * y_linear
    else:
        err32 = float(np.abs(out - ref32).max()) if ref32 is not None else 0.0
        print("%s %s: |gpu-f64| %.3g, y32 %.3g, |gpu-f32 oracle| %.3g" % (what, hc.head_id(head), err64, y_case, err32))
        assert err32 <= TOL_ORACLE
        assert err64 <= max(2 * y_case, FLOOR64)
    return err64


def fused_bars(what, head, out):
    c, cout, last_op = head
    return check_against_oracle(what, head, out, hc.ref_query(c, cout, last_op, "f64").astype(np.float64),
                                hc.ref_query(c, cout, last_op, "f32"), hc.y32(c, cout, last_op), hc.y0(c), hc.in_image(c))


# ---- 1. the fused query ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", hc.HEADS, ids=hc.head_id)
def test_fused_query(ops, scene, head):
    c, cout, last_op = head
    mlp, fh, pts, cal = scene.mlp(head), scene.maps(c)[0], scene.pts(c)[None], scene.calibs(c)[0]
    if c == 256:  # the gate between the two f32 kernels exists for C = 256 only
        with small_gate(0):
            out = ops.query(mlp, fh, pts, cal, syn.Z_SCALE)
        with small_gate(1):
            out32 = ops.query(mlp, fh, pts, cal, syn.Z_SCALE)
        assert torch.equal(out, out32)  # 64-point and 32-point tiles: the same bits
    else:
        out = ops.query(mlp, fh, pts, cal, syn.Z_SCALE)
    assert out.shape == (1, cout, N)
    assert torch.equal(out[0], scene.plain(head))  # the default gate: the same bits again
    fused_bars("fused", head, out[0].cpu().numpy())


# ---- 2. the direct MLP ----------------------------------------------------------------------------------------
def direct_bars(what, head, out):
    """Float64 restatement of SurfaceClassifier.forward on the scene's own float32 features (no mask: every column
    counts).  Bounded: the 2e-5 of test_surface_classifier_forward_on_explicit_features; linear: 2 Y0."""
    c, cout, last_op = head
    ref = hc.ref_direct(c, cout, last_op)
    assert out.shape == ref.shape and np.isfinite(out).all()
    err = float(np.abs(out - ref).max())
    print("%s %s: |gpu-f64| %.3g, Y0 %.3g (numpy float32 on the same features: %.3g)"
          % (what, hc.head_id(head), err, hc.y0(c), hc.y0_direct(c)))
    assert err <= (2 * hc.y0(c) if last_op == 0 else TOL_ORACLE)


@pytest.mark.parametrize("head", hc.HEADS, ids=hc.head_id)
def test_direct_mlp(ops, scene, head):
    direct_bars("direct", head, scene.direct(head).cpu().numpy())


def test_surface_classifier_default_last_op(ops, scene):
    """SurfaceClassifier(channels) -- last_op=None, the module's default as in the reference -- on a 512-channel,
    one-output head: the module's forward is ops.mlp_forward on a last_op = none head."""
    from monoport_amd.modeling.heads import SurfaceClassifier
    head = (512, 1, 0)
    layers = hc.layers_of(512, 1)
    mod = SurfaceClassifier([513, 1024, 512, 256, 128, 1])
    assert mod.last_op is None and mod.num_views == 1
    mod.load_state_dict({**{"filters.%d.weight" % i: torch.from_numpy(w)[:, :, None] for i, (w, _) in enumerate(layers)},
                         **{"filters.%d.bias" % i: torch.from_numpy(b) for i, (_, b) in enumerate(layers)}})
    mod.to(DEV).eval()
    with torch.no_grad():
        out = mod(scene.x(512))
    assert mod.packed().last_op == 0 and out.shape == (1, 1, N)
    assert torch.equal(out[0], scene.direct(head))
    direct_bars("SurfaceClassifier()", head, out[0].cpu().numpy())
    assert float(out.abs().max()) > 1.0  # a logit, not a squashed value


# ---- 3. batched and counted forms ---------------------------------------------------------------------------
@pytest.mark.parametrize("pair", hc.PAIRS, ids=hc.head_id)
def test_batched_and_counted_forms(ops, scene, pair):
    """mp_query_batch (3 frames, own map and calibration each), mp_query_counted and mp_query_counted_batch (counts
    0 / 65 / 257 in capacity 264) return the single-frame bits of test_fused_query; columns past a count are not
    written."""
    c, cout = pair
    head = (c, cout, 0)
    mlp, maps, cals = scene.mlp(head), scene.maps(c), scene.calibs(c)
    single = [scene.plain(head, v) for v in range(3)]
    assert not torch.equal(single[0], single[1]) and not torch.equal(single[1], single[2])
    batch = ops.query_batch(mlp, maps, scene.pts(c)[None].repeat(3, 1, 1), cals, ["orthogonal"] * 3, syn.Z_SCALE)
    assert batch.shape == (3, cout, N)
    for v in range(3):
        assert torch.equal(batch[v], single[v]), v
    padded = torch.full((3, CAP), 1e30, device=DEV)  # a kernel that read past the count would show it
    padded[:, :N] = scene.pts(c)
    counts = (0, 65, N)
    for gate in ((0, 1) if c == 256 else (-1,)):
        with small_gate(gate):
            out = torch.full((cout, CAP), SENTINEL, device=DEV)
            ops.query_counted(mlp, maps[0], padded, torch.tensor([N], dtype=torch.int32, device=DEV), cals[0],
                              syn.Z_SCALE, out=out)
            outs = [torch.full((cout, CAP), SENTINEL, device=DEV) for _ in counts]
            ops.query_counted_batch(mlp, maps, [padded.clone() for _ in counts],
                                    [torch.tensor([k], dtype=torch.int32, device=DEV) for k in counts],
                                    [cals[v] for v in range(3)], syn.Z_SCALE, outs=outs)
        assert torch.equal(out[:, :N], single[0]) and bool((out[:, N:] == SENTINEL).all()), gate
        for v, k in enumerate(counts):
            assert torch.equal(outs[v][:, :k], single[v][:, :k]), (gate, v)
            assert bool((outs[v][:, k:] == SENTINEL).all()), (gate, v)


# ---- 4. the skip table (C = 256) ----------------------------------------------------------------------------
@pytest.mark.parametrize("head", [h for h in hc.HEADS if h[0] == 256], ids=hc.head_id)
def test_skip_table_query(ops, scene, head):
    c, cout, last_op = head
    mlp, fh = scene.mlp(head), scene.maps(c)[0]
    plain = scene.plain(head)
    try:
        table = ops.skip_table(mlp, fh)
        out = ops.query(mlp, fh, scene.pts(c)[None], scene.calibs(c)[0], syn.Z_SCALE)[0]
    finally:
        ops.skip_table_release(mlp.ctx)
    again = ops.query(mlp, fh, scene.pts(c)[None], scene.calibs(c)[0], syn.Z_SCALE)[0]
    assert torch.equal(again, plain)      # released: the plain path again
    assert not torch.equal(out, plain)    # ... and the table kernel really ran
    fused_bars("table", head, out.cpu().numpy())
    print("table %s: |table - plain| %.3g" % (hc.head_id(head), float((out - plain).abs().max())))
    del table


# ---- 5. multi-view ------------------------------------------------------------------------------------------
def y0_views(c):
    """The linear multi-view yardstick of this C: the float32 torch-CPU model's largest error over Cout and V."""
    return max(hc.y0_views(c, v_n) for v_n in (2, 3))


@pytest.mark.parametrize("v_n", [2, 3])
@pytest.mark.parametrize("head", hc.HEADS, ids=hc.head_id)
def test_query_views(ops, scene, head, v_n):
    c, cout, last_op = head
    pts = scene.pts(c)[None].expand(v_n, 3, N)
    out = ops.query_views(scene.mlp(head), scene.maps(c)[:v_n], pts, scene.calibs(c)[:v_n], "orthogonal", syn.Z_SCALE)
    out = out.cpu().numpy()
    ref64, ref32 = hc.ref_views(c, cout, last_op, v_n, "f64"), hc.ref_views(c, cout, last_op, v_n, "f32")
    assert out.shape == (v_n, cout, N)
    y_case = hc.y32_views(c, cout, last_op, v_n)
    for v in range(v_n):  # row v: the view mean under view v's mask
        check_against_oracle("views V=%d row %d" % (v_n, v), head, out[v], ref64[v], ref32[v], y_case, y0_views(c),
                             hc.in_image(c, v))
    both = hc.in_image(c, 0) & hc.in_image(c, 1)
    assert np.array_equal(out[0][:, both], out[1][:, both])  # one prediction, V masks
    assert np.abs(out[0][:, both] - scene.plain(head).cpu().numpy()[:, both]).max() > 1e-3  # not the single-view field


@pytest.mark.parametrize("head", hc.HEADS, ids=hc.head_id)
def test_one_view_is_plain_query(ops, scene, head):
    """include/monoport_hip.h: mp_query_views with one view returns mp_query's bits."""
    c = head[0]
    one = ops.query_views(scene.mlp(head), scene.maps(c)[:1], scene.pts(c)[None], scene.calibs(c)[:1], "orthogonal",
                          syn.Z_SCALE)
    assert one.shape == (1, head[1], N) and torch.equal(one[0], scene.plain(head))


@pytest.mark.parametrize("head", hc.HEADS, ids=hc.head_id)
def test_forward_views_one_view_is_mlp_forward(ops, scene, head):
    one = ops.mlp_forward_views(scene.mlp(head), scene.x(head[0]))
    assert one.shape == (1, head[1], N) and torch.equal(one[0], scene.direct(head))


@pytest.mark.parametrize("pair", hc.PAIRS, ids=hc.head_id)
def test_forward_views_two_views(ops, scene, pair):
    """mp_mlp_forward_views on the explicit features of two views against mlp_views at float64.  The bar is the linear
    heads' 2 Y0 of the single-view oracle: the same layers and weights, and the view means only average errors."""
    c, cout = pair
    head = (c, cout, 0)
    out = ops.mlp_forward_views(scene.mlp(head), scene.x(c, 2)).cpu().numpy()
    ref = hc.ref_direct_views(c, cout, 0, 2)
    assert out.shape == ref.shape == (1, cout, N) and np.isfinite(out).all()
    err = float(np.abs(out - ref).max())
    print("forward_views V=2 %s: |gpu-f64| %.3g, Y0 %.3g (mlp_views at float32: %.3g)"
          % (hc.head_id(head), err, hc.y0(c), hc.y0_direct_views(c, 2)))
    assert err <= 2 * hc.y0(c)
    assert np.abs(out[0] - scene.direct(head).cpu().numpy()).max() > 1e-3  # the second view counts


@pytest.mark.parametrize("head", [(512, 1, 0), (256, 3, 0), (512, 3, 0), (256, 1, 1), (256, 1, 2)], ids=hc.head_id)
def test_views_counted_batch(ops, scene, head):
    """mp_query_views_counted_batch, 2 frames x 2 views with counts (65, 0): frame 0's first 65 columns are row
    ``view`` of mp_query_views bit for bit, nothing else is written."""
    c, cout, last_op = head
    mlp, maps, cals = scene.mlp(head), scene.maps(c), scene.calibs(c)
    pts = scene.pts(c)[None].expand(2, 3, N)
    rows = ops.query_views(mlp, maps[:2], pts, cals[:2], "orthogonal", syn.Z_SCALE)
    assert not torch.equal(rows[0], rows[1]) and float(rows[:, :, :65].abs().max()) > 0
    padded = torch.full((3, CAP), 1e30, device=DEV)
    padded[:, :N] = scene.pts(c)
    counts = [torch.tensor([k], dtype=torch.int32, device=DEV) for k in (65, 0)]
    for view in (0, 1):
        outs = [torch.full((cout, CAP), SENTINEL, device=DEV) for _ in range(2)]
        ops.query_views_counted_batch(mlp, [maps[:2], maps[1:3]], [padded, padded.clone()], counts,
                                      [cals[:2], cals[1:3]], "orthogonal", syn.Z_SCALE, view=view, outs=outs)
        assert torch.equal(outs[0][:, :65], rows[view][:, :65]), view
        assert bool((outs[0][:, 65:] == SENTINEL).all()) and bool((outs[1] == SENTINEL).all()), view


# ---- 6. the octree with a (512, 1) head -----------------------------------------------------------------------
def test_octree_512_1(ops):
    """mp_recon accepts any Cout = 1 head: a 512-channel sigmoid head (analytic body weights, so there is a surface)
    through the fused octree equals the level-at-a-time engine driven by ops.query on the same head, bit for bit."""
    res = [9, 17, 33]
    layers = hc.body_layers(512)
    f, calib = hc.body_scene(512)
    mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
    fh = ops.pack_features(torch.from_numpy(f)[None].to(DEV))
    cal = torch.from_numpy(calib.copy())[None].to(DEV)
    vol, status = ops.recon(mlp, fh, cal, syn.Z_SCALE, UNIT_BOX[0], UNIT_BOX[1], res)

    def query_func(points):
        return ops.query(mlp, fh, points.permute(0, 2, 1), cal, syn.Z_SCALE)

    gen, counts = ops.recon_generic(query_func, {}, DEV, UNIT_BOX[0], UNIT_BOX[1], res)
    assert status.tolist() == [1] + counts and counts[0] == 9 ** 3 and counts[-1] > 0
    assert vol.shape == (33, 33, 33) and torch.equal(vol, gen)
    inside = float((vol > 0.5).float().mean())
    print("octree (512, 1, sigmoid): counts %s, %.1f %% of the nodes inside" % (counts, 100 * inside))
    assert bool((vol > 0.5).any()) and bool((vol < 0.5).any())
    # the coarsest lattice (every node of it is queried) against the float32 oracle
    from oracle import pifu_oracle as orc
    ref = orc.dense_volume(lambda q: orc.query(f, q, calib, layers, 1, syn.Z_SCALE, precision="f32")[0],
                           UNIT_BOX[0], UNIT_BOX[1], 9, 33)
    assert np.abs(vol[::4, ::4, ::4].cpu().numpy() - ref).max() <= TOL_ORACLE
