"""The kernels between the encoders' convolutions over the map shapes their entry points admit, not only the square
maps of the stock encoders: csrc/encoder_ops.hip (avgpool2_gn, upsample_add_gn on both of its kernels, gn_apply,
group_norm, gn_stats, concat3_add, upsample_bicubic2x), scale_shift_add and the channels-last packer of csrc/pack.hip,
each against the float64 restatement of its definition in tests/elementwise_ref.py (held to torch's float64 CPU ops by
tests/test_elementwise_ref_cpu.py) -- values, not only the statistics of whatever was written.  Needs an MI355X.

Admission.  mp_avgpool2_gn: C % 32 == 0, H % 2 == 0, W % 8 == 0.  mp_upsample_bicubic2x_gn: C % 32 == 0, h, w >= 2,
w % 2 == 0; it runs the banded LDS kernel where 2w divides 256, 2h % 16 == 0 and (C / 32 * 2h) % 256 == 0
(mp_upsample_gn_banded, the function the launcher itself dispatches by) and the one-output-per-thread kernel everywhere
else.  mp_gn_apply: C % 32 == 0, H * W % 4 == 0.  mp_group_norm / mp_gn_stats: C % groups == 0, H * W % 4 == 0;
mp_gn_finalize: C / groups <= 64.  mp_concat3_add / mp_scale_shift_add: H * W % 4 == 0.  mp_upsample_bicubic2x and
mp_feat_pack_hwc: any size.

The lattices (elementwise_ref.py).  A workgroup is (image, group, slice): the C / 32 planes of a group are cut into
16 slices of ceil(steps / 16) steps, a step being one float4 (one output for the per-element upsample); a thread adds
its values in float32 and moves the sums to double after every 64 steps.  Rows are the smallest shapes at which each
class of that scheme can go wrong: fewer steps than slices (idle slices), a step count 16 does not divide (a short or
empty last slice), 3 and 5 channels per group (slices that cross planes), one output row per plane and one float4 per
output row, H != W in both directions, N in 1, 2, 3, 5, 7, a stock shape as control, and one row per kernel form with
64 steps per thread (2^18 values per group at one output per step, 2^20 at four): the only rows on which the flush to
double runs.  The upsample rows cover every clause of the banded kernel's rule on either side -- "banded", and missed
by "wide" (2w > 256), "width" (2w does not divide 256), "band" (2h % 16), "slice" ((C / 32 * 2h) % 256) -- with, on
the banded side, one band per slice holding both border clamps, two planes per slice, a slice that crosses a plane
between bands, 4 to 256 outputs per row, tall and wide maps.

Statistics.  avgpool2_gn, upsample_add_gn (both kernels) and gn_apply add the GroupNorm(32, C) statistics of what
they write into an accumulator when given one.  On EVERY row that does, the (scale, shift) decoded from it
(ops.gn_reference_ss) is held to scale_shift of the tensor that launch wrote: 2e-5 * max(1, max|ref|), the project's
existing bar (_check_ss of test_conv_admitted_shapes_gpu.py).

Bars and where they come from, with the maxima measured on an MI355X.
  avgpool2_gn: 2^-22 * max|x| -- three float32 additions of partial sums <= 4 max|x| (<= 3 * 2^-24 * 4 max|x| / 4 after
    the exact * 0.25).  Measured: <= 4.4e-8 * max|x| over the seven rows.
  upsample_add_gn, upsample_bicubic2x: 4e-6 * max(1, max|ref|) against bicubic2x, which takes the source coordinate in
    float32 as torch does for a float32 tensor (with a float64 coordinate the rounding of the coordinate alone is
    5e-6 of that scale at 128 rows, more than the bar).  The bar is 5x the 8.0e-7 a float32 evaluation in the kernel's
    op order was measured at when it was set (on this file's data test_elementwise_ref_cpu.py measures 8.2e-7 on the
    rows with ``add`` and 9.7e-7 without, and holds that model to 1e-6), which allows for FMA contraction, and is 5x
    below the 2e-5 of test_dropin_gpu.py.  Every row is also bit-equal to ops.upsample_bicubic2x(x, add), a third
    kernel with the same arithmetic, and prints the error of torch's own float32 interpolate on the GPU against the
    same reference: a row past the bar with torch within it is a kernel finding, not a reason to move the bar.
    Measured, of the scale: banded kernel <= 8.2e-7 (torch <= 5.3e-7), per-element kernel <= 9.7e-7 (torch <= 5.2e-7),
    upsample_bicubic2x on the odd maps <= 5.5e-7 (torch <= 3.8e-7) -- the float32 model's own figures: the library is
    built without FMA contraction.
  gn_apply: 5e-5 * max(1, max|ref|), the existing bar (test_encoder_dataflow_gpu.py).  Measured on the flush row
    (1, 32, 1024, 1024), max|d| against float64 at max|ref| = 9.4: 1.07e-6; torch's own float32 relu(GroupNorm) + res on
    the GPU: 1.07e-6.
  group_norm, gn_stats + gn_finalize: 2e-5 * max(1, max|ref|), the existing bar (test_dropin_gpu.py).  Measured on the
    flush row (1, 2, 1024, 1024, 2 groups), max|d| against float64 at max|ref| = 7.9: 6.7e-7; torch's own float32
    group_norm on the GPU: 9.5e-7.
  (scale, shift) from the accumulators: <= 7.9e-7 over all 70 launches that were given one (bar 2e-5 * scale).
  scale_shift_add: 2^-22 * max(|t * scale| + |shift| + |res|), three roundings of half an ulp of at most that sum.
  concat3_add (one IEEE addition per element) and pack_features (a copy): bit for bit against float32 torch on the CPU.

What the file catches.  Each of these was built into the library once and run against this file on an MI355X:
  sy and sx swapped in upsample_add_gn_kernel: the five non-square banded rows of
    test_upsample_add_gn_over_its_predicate fail (the square control does not);
  2h used for 2w where UpsampleAddOp::run splits its index into (oy, ox): six per-element rows fail, all with h != w;
  ``e1 += s1`` dropped from the flush of ew_gn_kernel: upsample row (1, 32, 256, 256) fails on its statistics and
    gn_apply row (1, 32, 1024, 1024) on its values (the statistics of its input come through the same kernel);
    dropped from gn_partial_kernel: group_norm row (1, 2, 1024, 1024, 2) fails;
  h and w swapped in the MP_PLAN_UPSAMPLE2X case of mp_plan_run: test_plan_replay_on_non_square_maps fails.
"""
import functools

import pytest
import torch

import elementwise_ref as er
from test_conv_admitted_shapes_gpu import _acc, _acc_of, _check_ss, _gn_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional
EPS = 1e-5


def _id(row):
    return "x".join(str(v) for v in row)


def _check_stats(what, acc, y, seed):
    """The accumulator a launch was given -> (scale, shift) of a GroupNorm(32, C), against the float64 moments of the
    tensor that launch wrote."""
    from monoport_amd import ops
    gn = _gn_params(y.shape[1], seed)
    got = ops.gn_reference_ss(acc, gn, (y.shape[1] // 32) * y.shape[2] * y.shape[3])
    _check_ss(what, got, er.scale_shift(y, 32, gn.weight, gn.bias, gn.eps))


def _refused(call):
    from monoport_amd import _lib
    with pytest.raises(_lib.MonoportError):
        call()
    torch.cuda.synchronize()


# ---- avgpool2_gn ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", er.AVGPOOL_ROWS, ids=_id)
def test_avgpool2_gn_over_its_predicate(row):
    from monoport_amd import ops
    n, c, h, w = row
    x = er.values(row, er.row_seed(row)).to(DEV)
    acc = _acc(n)
    y = ops.avgpool2_gn(x, acc)
    ref = er.avgpool2(x)
    xmax = x.abs().max().item()
    err = (y.double() - ref).abs().max().item()
    print("avgpool2_gn %s: max|d| vs fp64 %.3g = %.3g max|x| (bar %.3g)" % (row, err, err / xmax, 2.0 ** -22))
    assert y.shape == ref.shape and y.dtype == torch.float32 and err <= 2.0 ** -22 * xmax
    _check_stats("avgpool2_gn %s" % (row,), acc, y, 51)
    assert torch.equal(ops.avgpool2_gn(x), y)  # the same values without an accumulator


def test_avgpool2_gn_refusals():
    from monoport_amd import ops
    for shape in ((1, 32, 3, 8), (1, 32, 2, 12), (1, 32, 2, 4), (1, 48, 2, 8)):  # H = 3, W = 12, W = 4, C = 48
        x = torch.zeros(shape, device=DEV)
        acc = _acc(1)
        _refused(lambda: ops.avgpool2_gn(x, acc))
        assert (acc == 0).all()


# ---- upsample_add_gn, upsample_bicubic2x ------------------------------------------------------------------------

def _upsample_check(what, got, x, add, bar=4e-6):
    """got against bicubic2x(x, add); prints the error of torch's own float32 interpolate on the GPU next to it."""
    ref = er.bicubic2x(x, add)
    scale = max(1.0, ref.abs().max().item())
    err = (got.double() - ref).abs().max().item() / scale
    t32 = F.interpolate(x, scale_factor=2, mode="bicubic", align_corners=True)
    e_torch = ((t32 if add is None else add + t32).double() - ref).abs().max().item() / scale
    print("%s: max|d| vs fp64 %.3g of scale %.3g (bar %.3g); torch float32 interpolate on the GPU %.3g"
          % (what, err, scale, bar, e_torch))
    assert got.shape == ref.shape and got.dtype == torch.float32, what
    assert err <= bar, "%s: %g (torch: %g)" % (what, err, e_torch)


@pytest.mark.parametrize("row", er.UPSAMPLE_ROWS, ids=_id)
def test_upsample_add_gn_over_its_predicate(row):
    """Both kernels of mp_upsample_bicubic2x_gn: the value of every output, the kernel the launcher takes, the third
    kernel's bits, the statistics.  Measured maxima: the module docstring."""
    from monoport_amd import ops
    n, c, h, w, route, _ = row
    assert ops.upsample_banded(c, h, w) == (route == "banded") and er.upsample_route(c, h, w) == route
    x, add = (t.to(DEV) for t in er.upsample_inputs(row[:4]))
    for skip in (add, None) if row[:4] in er.UPSAMPLE_NO_ADD else (add,):
        what = "upsample_add_gn %s %s%s" % (route, row[:4], "" if skip is not None else " add=None")
        acc = _acc(n)
        u = ops.upsample_add_gn(x, skip, acc)
        _upsample_check(what, u, x, skip)
        assert torch.equal(u, ops.upsample_bicubic2x(x, add=skip)), what
        _check_stats(what, acc, u, 52)
        assert torch.equal(ops.upsample_add_gn(x, skip), u)


def test_upsample_add_gn_refusals():
    from monoport_amd import ops
    for shape in ((1, 32, 4, 3), (1, 48, 4, 4)):  # W = 3, C = 48
        x = torch.zeros(shape, device=DEV)
        acc = _acc(1)
        _refused(lambda: ops.upsample_add_gn(x, None, acc))
        assert (acc == 0).all() and not ops.upsample_banded(*shape[1:])


@pytest.mark.parametrize("shape", er.UPSAMPLE_PLAIN, ids=_id)
def test_upsample_bicubic2x_on_odd_maps(shape):
    from monoport_amd import ops
    x, add = (t.to(DEV) for t in er.upsample_inputs(shape))
    _upsample_check("upsample_bicubic2x %s" % (shape,), ops.upsample_bicubic2x(x), x, None)
    _upsample_check("upsample_bicubic2x %s + add" % (shape,), ops.upsample_bicubic2x(x, add=add), x, add)


# ---- gn_apply ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", er.GN_APPLY_ROWS, ids=_id)
def test_gn_apply_over_its_predicate(row):
    """Input as (accumulator, module) and as a (scale, shift) table, with and without ReLU and residual; on the
    2^20-values-per-group row one mode (hand-over, ReLU, residual), with torch's own float32 figure next to it."""
    from monoport_amd import ops
    n, c, h, w = row
    flush = h * w >= 1 << 20
    x = er.values(row, er.row_seed(row)).to(DEV)
    res = er.noise(row, er.row_seed(row) + 1).to(DEV)
    gn = _gn_params(c, 53)
    acc_x = _acc_of(x)
    table = ops.gn_reference_ss(acc_x, gn, (c // 32) * h * w)
    modes = [("hand-over", (acc_x, gn), True, res)] if flush else [
        (name, arg, relu, r) for name, arg in (("hand-over", (acc_x, gn)), ("table", table))
        for relu in (False, True) for r in (None, res)]
    for name, arg, relu, r in modes:
        what = "gn_apply %s %s relu %d res %d" % (row, name, relu, r is not None)
        acc_z = _acc(n)
        z = ops.gn_apply(x, arg, relu, res=r, stats=acc_z)
        ref = er.group_norm(x, 32, gn.weight, gn.bias, gn.eps, relu=relu, res=r)
        scale = max(1.0, ref.abs().max().item())
        err = (z.double() - ref).abs().max().item()
        print("%s: max|d| vs fp64 %.3g (bar %.3g)" % (what, err, 5e-5 * scale))
        if flush:
            with torch.no_grad():
                t32 = torch.relu(gn(x)) + r
            e32 = (t32.double() - ref).abs().max().item()
            print("%s: torch float32 relu(GroupNorm) + res on the GPU vs fp64 %.3g" % (what, e32))
            del t32
        assert z.shape == ref.shape and z.dtype == torch.float32 and err <= 5e-5 * scale, what
        del ref
        _check_stats(what, acc_z, z, 54)


def test_gn_apply_refusals():
    from monoport_amd import ops
    for shape in ((1, 32, 2, 3), (1, 48, 2, 2)):  # H * W = 6, C = 48
        x = torch.zeros(shape, device=DEV)
        ident = torch.ones((1, shape[1], 2), device=DEV)
        acc = _acc(1)
        _refused(lambda: ops.gn_apply(x, ident, False, stats=acc))
        assert (acc == 0).all()


# ---- group_norm, gn_stats + gn_finalize -------------------------------------------------------------------------

@pytest.mark.parametrize("row", er.GROUP_NORM_ROWS, ids=_id)
def test_group_norm_over_its_predicate(row):
    """mp_group_norm at group counts other than 32 (1, 2, 3, 40), groups of four values, and the 2^20-values-per-group
    row on which gn_partial_kernel moves its float32 sums to double; mp_gn_stats + mp_gn_finalize on the same rows."""
    from monoport_amd import ops
    n, c, h, w, groups = row
    x = (er.noise(row[:4], er.row_seed(row)) * 3 + 1.5).to(DEV)
    g = torch.Generator().manual_seed(55)
    weight, bias = (torch.rand(c, generator=g) + 0.5).to(DEV), (torch.rand(c, generator=g) - 0.5).to(DEV)
    ref = er.group_norm(x, groups, weight, bias, EPS)
    scale = max(1.0, ref.abs().max().item())
    y = ops.group_norm(x, groups, weight, bias, EPS, relu=False)
    err = (y.double() - ref).abs().max().item()
    print("group_norm %s: max|d| vs fp64 %.3g (bar %.3g)" % (row, err, 2e-5 * scale))
    if h * w >= 1 << 20:
        e32 = (F.group_norm(x, groups, weight, bias, EPS).double() - ref).abs().max().item()
        print("group_norm %s: torch float32 group_norm on the GPU vs fp64 %.3g" % (row, e32))
    assert y.shape == ref.shape and y.dtype == torch.float32 and err <= 2e-5 * scale
    assert torch.equal(ops.group_norm(x, groups, weight, bias, EPS, relu=True), torch.relu(y))
    assert c // groups <= 64
    stats = ops.gn_stats(x, groups)
    ss = ops.gn_finalize(stats, n, c, groups, (c // groups) * h * w, weight, bias, EPS)
    _check_ss("gn_stats + gn_finalize %s" % (row,), ss, er.scale_shift(x, groups, weight, bias, EPS))


# ---- bit for bit against float32 torch on the CPU -----------------------------------------------------------------

@pytest.mark.parametrize("n,chans,hw", [(1, (1, 1, 1), (1, 4)), (3, (5, 3, 7), (2, 6)), (2, (128, 64, 64), (8, 40))])
def test_concat3_add_on_narrow_segments(n, chans, hw):
    from monoport_amd import ops
    g = torch.Generator().manual_seed(56 + n)
    a, b, c = (torch.randn((n, k) + hw, generator=g) * 1.7 + 0.2 for k in chans)
    sc = torch.randn((n, sum(chans)) + hw, generator=g)
    got = ops.concat3_add(a.to(DEV), b.to(DEV), c.to(DEV), sc.to(DEV))
    assert torch.equal(got.cpu(), torch.cat((a, b, c), 1) + sc)


def test_pack_features_off_the_tile():
    """40 + 24 channels of a 5 x 7 map: neither C nor H * W is a multiple of the 32 x 32 tile, the second map lands at
    channel offset 40; every element of the destination is written, nothing on either side of it."""
    from monoport_amd import ops
    a, b = er.values((1, 40, 5, 7), 57), er.values((1, 24, 5, 7), 58)
    guard, sentinel = 256, -12345.0
    buf = torch.full((guard + 5 * 7 * 64 + guard,), sentinel, device=DEV)
    out = buf[guard:guard + 5 * 7 * 64].view(5, 7, 64)
    got = ops.pack_features([a.to(DEV), b.to(DEV)], out=out)
    torch.cuda.synchronize()
    want = torch.cat((a, b), 1)[0].permute(1, 2, 0).contiguous()
    assert got.data_ptr() == out.data_ptr() and not (want == sentinel).any()
    assert torch.equal(out.cpu(), want)
    assert (buf[:guard] == sentinel).all() and (buf[guard + 5 * 7 * 64:] == sentinel).all()
    assert torch.equal(ops.pack_features([a.to(DEV), b.to(DEV)]).cpu(), want)


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (3, 5, 2, 6)], ids=_id)
def test_scale_shift_add_small(shape):
    from monoport_amd import ops
    n, c = shape[:2]
    t, res = er.values(shape, 59).to(DEV), er.noise(shape, 60).to(DEV)
    g = torch.Generator().manual_seed(61)
    ss = torch.stack((torch.rand((n, c), generator=g) + 0.5, torch.randn((n, c), generator=g)), 2).to(DEV)
    sc, sh = ss[..., 0, None, None].double(), ss[..., 1, None, None].double()
    ref = res.double() + (t.double() * sc + sh)
    bar = 2.0 ** -22 * ((t.double() * sc).abs() + sh.abs() + res.double().abs()).max().item()
    y = ops.scale_shift_add(t, ss, res)
    err = (y.double() - ref).abs().max().item()
    print("scale_shift_add %s: max|d| vs fp64 %.3g (bar %.3g)" % (shape, err, bar))
    assert y.shape == ref.shape and err <= bar


# ---- plan replay on non-square maps -----------------------------------------------------------------------------

PLAN_SHAPES = {"pool": (2, 96, 10, 24), "banded": (3, 96, 128, 16), "element": (2, 64, 16, 6), "apply": (2, 160, 5, 12)}


@functools.lru_cache(maxsize=None)
def _plan_data(seed):
    d = {}
    for i, (k, s) in enumerate(PLAN_SHAPES.items()):
        d[k] = er.values(s, seed + 10 * i)
        up = k in ("banded", "element")  # add [N,C,2h,2w] of an upsample, res [N,C,H,W] of gn_apply
        d[k + "_add"] = er.noise((s[0], s[1], 2 * s[2], 2 * s[3]) if up else s, seed + 10 * i + 1)
    return d


def _plan_chain(t, accs, gn, ident):
    from monoport_amd import ops
    p = ops.avgpool2_gn(t["pool"], accs[0])
    ub = ops.upsample_add_gn(t["banded"], t["banded_add"], accs[1])
    ue = ops.upsample_add_gn(t["element"], t["element_add"], accs[2])
    ops.gn_apply(t["apply"], ident, relu=False, stats=accs[3])  # the statistics of the input, as _acc_of takes them
    z = ops.gn_apply(t["apply"], (accs[3], gn), True, res=t["apply_add"], stats=accs[4])
    return [p, ub, ue, z]


def test_plan_replay_on_non_square_maps():
    """mp_plan_pool_args / mp_plan_upsample_args / mp_plan_gn_apply_args carry h and w through a struct: a plan recorded
    on one set of inputs and replayed on another gives, bit for bit, what a launch-by-launch pass gives -- outputs and
    accumulators -- on maps where an h / w swap shows, on both upsample kernels."""
    from monoport_amd import ops
    assert ops.upsample_banded(*PLAN_SHAPES["banded"][1:]) and not ops.upsample_banded(*PLAN_SHAPES["element"][1:])
    gn = _gn_params(PLAN_SHAPES["apply"][1], 62)
    ident = torch.zeros(PLAN_SHAPES["apply"][:2] + (2,), device=DEV)
    ident[..., 0] = 1.0
    order = ("pool", "banded", "element", "apply", "apply")
    t = {k: v.to(DEV) for k, v in _plan_data(70).items()}
    accs = [_acc(PLAN_SHAPES[k][0]) for k in order]
    with ops.record_plan(DEV) as rec:
        outs = _plan_chain(t, accs, gn, ident)
    plan = rec.finish()
    torch.cuda.synchronize()
    assert plan.n_cmds == 5
    first = [o.clone() for o in outs]
    for k, v in _plan_data(170).items():  # other data in the same buffers
        t[k].copy_(v)
    for a in accs:
        a.zero_()
    plan.run(DEV)
    torch.cuda.synchronize()
    replay, replay_accs = [o.clone() for o in outs], [a.clone() for a in accs]
    fresh_accs = [_acc(PLAN_SHAPES[k][0]) for k in order]
    fresh = _plan_chain({k: v.to(DEV) for k, v in _plan_data(170).items()}, fresh_accs, gn, ident)
    torch.cuda.synchronize()
    names = ("avgpool2_gn", "upsample banded", "upsample per-element", "gn_apply")
    for name, a, b, c in zip(names, replay, fresh, first):
        assert torch.equal(a, b), name
        assert not torch.equal(a, c), name
    for a, b in zip(replay_accs, fresh_accs):
        assert torch.equal(a, b) and (a != 0).any()
