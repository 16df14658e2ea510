"""The encoder convolutions over the shapes their own predicates admit, not only the ones the stock encoders use:
csrc/conv3x3.hip (large-tile, split-K, f16x3), csrc/conv_wino.hip (64- and 128-channel kernels), csrc/convim2col.hip
(7x7, 3x3 stride 2) and the fused 1x1 against float64 -- ``torch.nn.functional.conv2d`` in float64 on the float64
input, after a float64 two-pass GroupNorm + ReLU where a GroupNorm input is fused.  The statistics a launch hands to
the next GroupNorm are compared with the float64 two-pass moments of the tensor the launch itself wrote, never with
another kernel's.  Needs an MI355X.

The lattice.  mp_conv3x3_supported admits Cin % 16 == 0 (<= 512), Cout % 32 == 0, H >= 8 and W >= 32 powers of two.
``ROWS`` is a covering subset of that product, picked by this rule: every required Cin (16, 48, 80, 96, 160, 272, 512:
odd and even counts of 16-channel K chunks, 3 and 5 channels per input group, the upper limit), every required Cout
(32, 96, 160, 192, 320, 384 and the power-of-two controls 64, 128, 256 next to them), every required map (8x32,
8x1024, 512x32, 16x64, 64x64, 32x256), every N (1, 3, 7, and 320 / 512 images of 8x32, past the 512- and
2048-workgroup thresholds of conv_plan / wino_use64) and every Ctot (128, 256, 512) appears in at least one row, a
failing-prone Cout shares its map with a control, and each row runs on EVERY route that admits its Cout (auto, large
tiles, split-K, the direct heuristic, Winograd K64 for Cout % 64 == 0, K128 for Cout % 128 == 0, f16x3) -- so each
route sees each class at least once while the float64 reference is computed once per row.

Statistics of the convolution's own output are served where Cout / 32 divides 32 (Cout 32, 64, 128, 256, 512, 1024:
the epilogues fold whole groups out of a workgroup's 32- / 64- / 128-channel block); for any other Cout the launchers
refuse the request (MP_ERR_UNSUPPORTED) and still serve y, the block tail and the tail's statistics.  The tests
assert that refusal, and everything else at those Cout.  (The launcher's "map too small for a tile" refusal has no
case: with H >= 8 no tile conv_plan picks is taller than the map.)

Bars: the project's existing ones, unchanged -- direct kernels and f16x3 2e-5 * max(1, max|ref|)
(test_conv_gpu.py), Winograd 1e-5 * the same scale (test_conv_wino_gpu.py), (scale, shift) 2e-5 * max(1, max|ref|)
(test_encoder_dataflow_gpu.py), convk 2e-5 / 5e-5 with a GroupNorm input, 1x1 2e-5 / 5e-5.  They were set at
Cin <= 256; at Cin = 272 and 512 each case also prints the error of torch's own float32 conv2d (on the GPU and on the
CPU) against the same float64 reference.  Measured on an MI355X the existing bars hold there with a factor of 9 or
more to spare (figures in ``test_conv3x3_admitted_lattice``), so they are kept."""
import ctypes
import functools
import types

import pytest
import torch

from elementwise_ref import scale_shift

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional

# route -> (mp_conv3x3_tune word, weight precision)
ROUTES = {"auto": (0, "f32"), "large": (0x100, "f32"), "splitk": (0x200, "f32"), "direct": (0x400, "f32"),
          "k64": (0x800, "f32"), "k128": (0x1000, "f32"), "f16x3": (0, "f16x3")}
WINO = ("k64", "k128")


def _stats_served(cout):
    """The launchers' rule for statistics of the convolution's own output: Cout / 32 divides 32."""
    return 32 % (cout // 32) == 0


def _gn_params(c, seed):
    g = torch.Generator().manual_seed(seed)
    gn = torch.nn.GroupNorm(32, c)
    with torch.no_grad():
        gn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        gn.bias.copy_(torch.rand(c, generator=g) - 0.5)
    return gn.to(DEV).requires_grad_(False)


def _acc(n):
    from monoport_amd import ops
    return ops.gn_acc_zeros(DEV, n)


def _acc_of(x):
    """Accumulator holding the statistics of x (mp_gn_apply with an identity scale / shift)."""
    from monoport_amd import ops
    ident = torch.zeros((x.shape[0], x.shape[1], 2), device=DEV)
    ident[..., 0] = 1.0
    acc = _acc(x.shape[0])
    ops.gn_apply(x, ident, relu=False, stats=acc)
    return acc


def _ss64(t, cpg, weight, bias, eps):
    """(scale, shift) [N,C,2] in float64 of a GroupNorm with cpg channels per group over t, from the definition."""
    return scale_shift(t, t.shape[1] // cpg, weight, bias, eps)


def _gn_relu64(x, gn):
    ss = _ss64(x, x.shape[1] // 32, gn.weight, gn.bias, gn.eps)
    return torch.relu(x.double() * ss[..., 0, None, None] + ss[..., 1, None, None])


def _check_ss(what, got, ref, tol=2e-5):
    err = (got.double() - ref).abs().max().item()
    print("%s: (scale, shift) off by %.3g" % (what, err))
    assert got.shape == ref.shape and err <= tol * max(1.0, ref.abs().max().item()), "%s: ss off by %g" % (what, err)


def _check_own_stats(what, acc, y, gn):
    """The accumulator of y's producer -> (scale, shift) of GroupNorm(32, C), per channel, all groups."""
    from monoport_amd import ops
    cpg = y.shape[1] // 32
    got = ops.gn_reference_ss(acc, gn, cpg * y.shape[2] * y.shape[3])
    _check_ss(what, got, _ss64(y, cpg, gn.weight, gn.bias, gn.eps))


def _check_tail_stats(what, acc_o, out, gn_o, off, cout):
    """The groups of the wide tensor this launch filled ([off, off + cout)) against the moments of out there; the
    accumulator words of every other group still zero."""
    from monoport_amd import ops
    ctot = out.shape[1]
    cpg = ctot // 32
    got = ops.gn_reference_ss(acc_o, gn_o, cpg * out.shape[2] * out.shape[3])[:, off:off + cout]
    ref = _ss64(out[:, off:off + cout], cpg, gn_o.weight[off:off + cout], gn_o.bias[off:off + cout], gn_o.eps)
    _check_ss(what, got, ref)
    assert (acc_o[:, :, :off // cpg] == 0).all() and (acc_o[:, :, (off + cout) // cpg:] == 0).all(), what


# ---- 3x3, stride 1 ------------------------------------------------------------------------------

# (N, Cin, Cout, H, W, Ctot, off, reflect, gn): gn = fuse a GroupNorm(32, Cin) + ReLU input (needs Cin % 32 == 0)
ROWS = [
    (1, 16, 32, 8, 32, 128, 96, False, False),      # one K chunk, the smallest map, one workgroup row
    (3, 48, 96, 8, 32, 128, 32, True, False),       # 3 chunks; Cout / 32 = 3
    (7, 96, 96, 16, 64, 256, 160, False, True),     # 3 channels per input group
    (7, 96, 64, 16, 64, 256, 192, False, True),     # control of the row above
    (3, 160, 160, 64, 64, 512, 352, True, True),    # 5 channels per input group, Cout / 32 = 5
    (3, 160, 128, 64, 64, 512, 384, True, True),    # control
    (1, 272, 192, 32, 256, 256, 64, False, False),  # 17 chunks; Cout / 32 = 6: three 64-channel blocks
    (1, 272, 256, 32, 256, 256, 0, False, False),   # control
    (1, 512, 320, 16, 64, 512, 192, False, True),   # the ss_in table's limit; Cout / 32 = 10
    (1, 512, 64, 16, 64, 512, 448, True, True),     # control
    (3, 80, 384, 8, 1024, 512, 128, False, False),  # 5 chunks; three 128-channel blocks; 32 tiles in one row
    (3, 80, 128, 8, 1024, 512, 0, True, False),     # control
    (1, 48, 192, 512, 32, 256, 0, True, False),     # one tile per row, 64 (Winograd) / 128 (split-K) tile rows
    (7, 16, 128, 512, 32, 128, 0, False, False),    # control, tall, N = 7
    (1, 96, 384, 64, 64, 512, 0, False, False),     # plain input although Cin % 32 == 0
    (1, 32, 512, 8, 32, 512, 0, False, True),       # 16 channels per output group: the widest Cout in reach of Ctot
    (320, 48, 96, 8, 32, 128, 0, False, False),     # 1920 large-tile workgroups on a non-square map
    (512, 16, 256, 8, 32, 256, 0, False, False),    # 2048 128-channel Winograd workgroups: wino_use64 flips
]


def _routes_of(cout):
    return [r for r in ROUTES if (r != "k64" or cout % 64 == 0) and (r != "k128" or cout % 128 == 0)]


LATTICE = [(row, route) for row in ROWS for route in _routes_of(row[2])]


@functools.lru_cache(maxsize=1)
def _row(row):
    """Inputs of a row (seeded CPU generator) and its float64 reference; kept for the row's routes."""
    n, cin, cout, h, w, ctot, off, reflect, gn = row
    g = torch.Generator().manual_seed(cin * 7 + cout * 3 + h + w + n)
    x = (torch.randn((n, cin, h, w), generator=g) * 2 + 0.3).to(DEV)
    res = torch.randn((n, ctot, h, w), generator=g).to(DEV)
    wt = (torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).to(DEV)
    gn_in = _gn_params(cin, 1) if gn else None
    with torch.no_grad():
        v = _gn_relu64(x, gn_in) if gn else x.double()
        v = torch.nn.ReflectionPad2d(1)(v) if reflect else F.pad(v, (1, 1, 1, 1))
        ref = F.conv2d(v, wt.double())
        e32 = None
        if cin > 256:  # what torch's own float32 convolution makes of the same inputs, on the GPU and on the CPU
            v32 = v.float()
            e32 = ((F.conv2d(v32, wt).double() - ref).abs().max().item(),
                   (F.conv2d(v32.cpu(), wt.cpu()).double() - ref.cpu()).abs().max().item())
    acc_x = _acc_of(x) if gn else None
    return x, res, wt, gn_in, acc_x, ref, e32


def _launch(tune, x, gn_arg, packed, relu, reflect, res, off, ctot, want_stats):
    from monoport_amd import _lib, ops
    lib = _lib.load()
    n = x.shape[0]
    out = torch.full((n, ctot, x.shape[2], x.shape[3]), 7.0, device=DEV)
    acc_y, acc_o = _acc(n), _acc(n)
    lib.mp_conv3x3_tune(tune)
    try:
        y = ops.conv3x3_fused(x, gn_arg, packed, relu=relu, reflect=reflect, stats=acc_y if want_stats else None, out=out,
                              res=res, out_off=off, out_stats=acc_o)
    finally:
        lib.mp_conv3x3_tune(0)
    torch.cuda.synchronize()
    return y, out, acc_y, acc_o


@pytest.mark.parametrize("row,route", LATTICE, ids=["%s-%s" % ("x".join(str(int(v)) for v in r), m) for r, m in LATTICE])
def test_conv3x3_admitted_lattice(row, route):
    """One launch of mp_conv3x3_ex per (row, route): y, the pyramid tail, both sets of statistics, determinism.

    Cin = 272 / 512 (float32 sums of 2448 / 4608 products), measured on an MI355X, max|d| against float64:
      Cin 272 (scale 14 .. 15.5): large tiles 2.8e-5 .. 3.0e-5, split-K 1.1e-5 .. 1.3e-5, f16x3 1.9e-5 .. 2.0e-5,
        Winograd 9.3e-6 .. 9.6e-6; torch's float32 conv2d 1.1e-5 .. 1.2e-5 on the GPU, 3.9e-6 .. 4.4e-6 on the CPU;
      Cin 512 (scale 4.7 .. 4.9): large tiles 7.3e-6 .. 9.6e-6, split-K 3.2e-6 .. 3.4e-6, f16x3 7.1e-6 .. 8.7e-6,
        Winograd 3.2e-6 .. 4.6e-6; torch 1.1e-6 .. 3.3e-6 on the GPU, 1.1e-6 .. 1.2e-6 on the CPU.
    The large-tile kernel (one float32 chain over all of K per accumulator) is up to 3x torch's GPU error and past
    twice it; the existing bars (2e-5 * scale = 9.5e-5 .. 3.1e-4, Winograd half of that) hold at 272 and 512 with a
    factor of 9 or more to spare, so they are kept as they are."""
    from monoport_amd import _lib, ops
    n, cin, cout, h, w, ctot, off, reflect, gn = row
    tune, precision = ROUTES[route]
    x, res, wt, gn_in, acc_x, ref, e32 = _row(row)
    assert ops.conv3x3_supported(cin, cout, h, w)
    packed = ops.PackedConv3x3(wt, precision)
    if route in WINO:
        assert packed.wino is not None and _lib.load().mp_conv3x3_wino_supported(cin, cout, h, w) == 1
    gn_arg = (acc_x, gn_in) if gn else None
    served = _stats_served(cout)
    if not served:  # statistics of y for a Cout whose groups straddle the workgroups' channel blocks: refused, loudly
        with pytest.raises(_lib.MonoportError, match="statistics"):
            _launch(tune, x, gn_arg, packed, gn, reflect, res, off, ctot, True)
    y, out, acc_y, acc_o = _launch(tune, x, gn_arg, packed, gn, reflect, res, off, ctot, served)
    what = "conv3x3 %s %s" % (route, row[:5])
    scale = max(1.0, ref.abs().max().item())
    err = (y.double() - ref).abs().max().item()
    bar = (1e-5 if route in WINO else 2e-5) * scale
    print("%s: max|d| vs fp64 %.3g (bar %.3g, scale %.3g)" % (what, err, bar, scale))
    if e32 is not None:
        print("%s: torch float32 conv2d vs fp64: GPU %.3g, CPU %.3g; twice the larger %.3g" % (what, e32[0], e32[1], 2 * max(e32)))
    assert y.shape == ref.shape and err <= bar
    if route in WINO:  # it IS the other algorithm
        assert not torch.equal(y, _launch(0x400, x, gn_arg, packed, gn, reflect, res, off, ctot, False)[0])
    # pyramid-block tail: exactly y + res on this launch's channels, nothing else written
    assert torch.equal(out[:, off:off + cout], y + res[:, off:off + cout])
    untouched = torch.ones(ctot, dtype=torch.bool)
    untouched[off:off + cout] = False
    assert (out[:, untouched] == 7.0).all()
    # the statistics the next GroupNorms get, against the float64 moments of what this launch wrote
    if served:
        _check_own_stats(what + " y", acc_y, y, _gn_params(cout, 2))
    else:
        assert (acc_y == 0).all()
    _check_tail_stats(what + " y + res", acc_o, out, _gn_params(ctot, 3), off, cout)
    # deterministic (integer statistics, fixed summation order)
    y2, out2, acc_y2, acc_o2 = _launch(tune, x, gn_arg, packed, gn, reflect, res, off, ctot, served)
    assert torch.equal(y, y2) and torch.equal(out, out2) and torch.equal(acc_y, acc_y2) and torch.equal(acc_o, acc_o2)
    if route in WINO:
        return
    # the legacy entry points (mp_conv3x3_gn / _gn16: precomputed (scale, shift) in, partial sums out)
    ss_in = ops.gn_reference_ss(acc_x, gn_in, (cin // 32) * h * w) if gn else None
    lib = _lib.load()
    lib.mp_conv3x3_tune(tune)
    try:
        if not served:
            with pytest.raises(_lib.MonoportError, match="statistics"):
                ops.conv3x3_gn(x, ss_in, packed, relu=gn, want_stats=True, reflect=reflect)
        yl, st = ops.conv3x3_gn(x, ss_in, packed, relu=gn, want_stats=served, reflect=reflect)
    finally:
        lib.mp_conv3x3_tune(0)
    if route == "auto":  # the hand-over launch may have taken the Winograd kernel, the legacy form never does
        assert (yl.double() - ref).abs().max().item() <= bar
    else:
        assert torch.equal(yl, y)  # hand-over and precomputed (scale, shift) agree bit for bit
    if served:
        gy = _gn_params(cout, 2)
        ss = ops.gn_finalize(st, n, cout, 32, (cout // 32) * h * w, gy.weight, gy.bias, gy.eps)
        _check_ss(what + " legacy", ss, _ss64(yl, cout // 32, gy.weight, gy.bias, gy.eps))


def _raw_conv3x3(x, packed, out=None, res=None, ctot=0, off=0, ss=None, acc_y=None, y=None, wino=True):
    """mp_conv3x3_ex called directly; returns (rc, message)."""
    from monoport_amd import _lib, ops
    lib = _lib.load()
    a = _lib.Conv3x3Args()
    a.x, a.n, a.cin, a.h, a.w, a.cout = x.data_ptr(), x.shape[0], x.shape[1], x.shape[2], x.shape[3], packed.cout
    a.packed = packed.data.data_ptr()
    if wino and packed.wino is not None:
        a.packed_wino = packed.wino.data_ptr()
    if y is not None:
        a.y = y.data_ptr()
    if out is not None:
        a.y2, a.res, a.y2_channels, a.y2_offset = out.data_ptr(), res.data_ptr(), ctot, off
    if ss is not None:
        a.gn.ss = ss.data_ptr()
        a.relu = 1
    if acc_y is not None:
        a.fin.acc = acc_y.data_ptr()
    ctx = ops.get_encoder_context(torch.device(DEV))
    rc = lib.mp_conv3x3_ex(ctx.handle, ctypes.byref(a), None)
    torch.cuda.synchronize()
    return rc, lib.mp_last_error(ctx.handle).decode()


# (Cin, Cout, H, W, words the message must carry)
REFUSED = [(528, 64, 16, 64, ("at most 512", "528")), (48, 48, 16, 64, ("Cout % 32", "48 -> 48")),
           (64, 64, 4, 32, ("H >= 8", "4x32")), (64, 64, 48, 80, ("powers of two", "48x80")),
           (64, 64, 16, 16, ("W >= 32", "16x16")), (24, 64, 16, 64, ("Cin % 16", "24 -> 64"))]


@pytest.mark.parametrize("cin,cout,h,w,words", REFUSED)
def test_conv3x3_refuses_what_the_predicate_excludes(cin, cout, h, w, words):
    """mp_conv3x3_ex with the Winograd weights given: a non-zero status, a message naming the reason, y and the tail
    buffer untouched.  48 x 80 passes the Winograd predicate (H % 8 == 0, W % 16 == 0) -- it is only reachable behind
    mp_conv3x3_supported, and this pins that nobody widens one without the other."""
    from monoport_amd import _lib, ops
    lib = _lib.load()
    assert lib.mp_conv3x3_supported(cin, cout, h, w) == (1 if cin == 528 else 0)  # Cin > 512: the launcher's limit
    if (h, w) == (48, 80):
        assert lib.mp_conv3x3_wino_supported(cin, cout, h, w) == 1
    x = torch.zeros((2, cin, h, w), device=DEV)
    if cin % 16 or cout % 32:  # the packing kernels refuse such weights themselves; the launcher sees a stand-in
        with pytest.raises(_lib.MonoportError, match="Cin % 16 == 0 and Cout % 32 == 0"):
            ops.PackedConv3x3(torch.zeros((cout, cin, 3, 3), device=DEV))
        packed = types.SimpleNamespace(cout=cout, cin=cin, precision="f32", wmax=None, wino=None,
                                       data=torch.zeros((cout * cin * 9,), device=DEV))
    else:
        packed = ops.PackedConv3x3(torch.zeros((cout, cin, 3, 3), device=DEV))
    y = torch.full((2, cout, h, w), 7.0, device=DEV)
    out = torch.full((2, 128, h, w), 7.0, device=DEV)
    for tune in (0, 0x400, 0x800):
        lib.mp_conv3x3_tune(tune)
        try:
            rc, msg = _raw_conv3x3(x, packed, out=out, res=torch.zeros_like(out), ctot=128, off=0, y=y)
        finally:
            lib.mp_conv3x3_tune(0)
        assert rc != 0 and all(wd in msg for wd in words), (rc, msg)
        assert (y == 7.0).all() and (out == 7.0).all()
    with pytest.raises(_lib.MonoportError):
        ops.conv3x3_fused(x, None, packed, relu=False)
    with pytest.raises(_lib.MonoportError):
        ops.conv3x3_gn(x, None, packed, relu=False)


def test_conv3x3_refuses_bad_groupnorm_and_tail_requests():
    """A GroupNorm input on Cin % 32 != 0, a wide tensor whose Ctot / 32 does not divide 32, an offset inside a group,
    a launch that would run past Ctot, and statistics of y at a Cout / 32 that does not divide 32: MP_ERR_ARG /
    MP_ERR_UNSUPPORTED with the reason, nothing written.  With (Ctot / 32) | 32 | Cout and an offset on a group
    boundary, [off, off + Cout) always ends on a group boundary of the wide tensor: no admitted request ends inside
    a group."""
    from monoport_amd import ops
    n, h, w = 2, 16, 64
    x48 = torch.randn((n, 48, h, w), device=DEV)
    p48 = ops.PackedConv3x3(torch.randn((64, 48, 3, 3), device=DEV))
    ss = torch.ones((n, 48, 2), device=DEV)
    y = torch.full((n, 64, h, w), 7.0, device=DEV)
    rc, msg = _raw_conv3x3(x48, p48, ss=ss, y=y)
    assert rc != 0 and "Cin % 32" in msg and (y == 7.0).all()
    x = torch.randn((n, 64, h, w), device=DEV)
    for cout, ctot, off in ((96, 384, 0), (96, 512, 8), (160, 512, 24), (192, 256, 128), (192, 256, 68), (96, 128, 64)):
        packed = ops.PackedConv3x3(torch.randn((cout, 64, 3, 3), device=DEV))
        out = torch.full((n, ctot, h, w), 7.0, device=DEV)
        y = torch.full((n, cout, h, w), 7.0, device=DEV)
        rc, msg = _raw_conv3x3(x, packed, out=out, res=torch.zeros_like(out), ctot=ctot, off=off, y=y)
        assert rc != 0 and "bad fused-tail request (%d channels at offset %d of %d)" % (cout, off, ctot) in msg, (rc, msg)
        assert (y == 7.0).all() and (out == 7.0).all()
    for cout in (96, 160, 192, 320, 384):
        packed = ops.PackedConv3x3(torch.randn((cout, 64, 3, 3), device=DEV))
        y = torch.full((n, cout, h, w), 7.0, device=DEV)
        acc = _acc(n)
        for wino in (True, False):
            rc, msg = _raw_conv3x3(x, packed, acc_y=acc, y=y, wino=wino)
            assert rc != 0 and "statistics" in msg and "Cout / 32" in msg, (rc, msg)
            assert (y == 7.0).all() and (acc == 0).all()
        assert not ops.conv3x3_stats_supported(cout)
    assert all(ops.conv3x3_stats_supported(c) for c in (32, 64, 128, 256, 512))


# ---- 7x7 and 3x3 stride 2 (csrc/convim2col.hip) -------------------------------------------------

# (ks, stride, N, Cin, Cout, H, W, reflect, gn)
CONVK = [(7, 1, 1, 3, 64, 2, 64, False, False), (7, 1, 3, 3, 64, 6, 192, False, False), (7, 1, 2, 3, 64, 14, 64, True, False),
         (7, 2, 3, 3, 64, 2, 128, False, False), (7, 2, 1, 3, 64, 6, 384, False, False), (7, 2, 2, 3, 64, 14, 128, True, False),
         (3, 2, 1, 16, 128, 2, 128, False, False), (3, 2, 3, 48, 256, 6, 384, False, False),
         (3, 2, 2, 48, 384, 14, 128, False, False), (3, 2, 1, 16, 384, 6, 384, True, False),
         (3, 2, 2, 48, 128, 14, 384, True, False), (3, 2, 3, 16, 256, 2, 128, False, False),
         (3, 2, 2, 96, 256, 6, 128, False, True), (3, 2, 1, 160, 384, 14, 128, False, True)]


@pytest.mark.parametrize("ks,stride,n,cin,cout,h,w,reflect,gn", CONVK)
def test_convk_over_its_predicate(ks, stride, n, cin, cout, h, w, reflect, gn):
    """mp_convk at map heights that are no powers of two (H % stride == 0), output widths 64 and 192, odd counts of
    16-channel chunks, Cout = 384 (three 128-channel blocks), 3 and 5 channels per input group; bias, both paddings,
    statistics against the float64 moments of y."""
    from monoport_amd import _lib, ops
    assert ops.convk_supported(cin, cout, ks, stride, h, w)
    g = torch.Generator().manual_seed(ks * 100 + cin + cout + h + w)
    x = (torch.randn((n, cin, h, w), generator=g) * 2 + 0.3).to(DEV)
    wt = (torch.randn((cout, cin, ks, ks), generator=g) * (2.0 / (ks * ks * cin)) ** 0.5).to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    gn_in = _gn_params(cin, 4) if gn else None
    gn_arg = (_acc_of(x), gn_in) if gn else None
    pad = ks // 2
    with torch.no_grad():
        v = _gn_relu64(x, gn_in) if gn else x.double()
        if reflect:
            v = torch.nn.ReflectionPad2d(pad)(v)
        else:
            v = F.pad(v, (pad, pad, pad, pad))
        ref = F.conv2d(v, wt.double(), bias.double(), stride=stride)
    packed = ops.PackedConvK(wt, bias)
    served = _stats_served(cout)
    what = "convk %dx%d s%d %s" % (ks, ks, stride, (n, cin, cout, h, w))
    if not served:
        with pytest.raises(_lib.MonoportError, match="statistics"):
            ops.convk(x, gn_arg, gn, packed, stride, reflect=reflect, stats=_acc(n))
    acc = _acc(n)
    y = ops.convk(x, gn_arg, gn, packed, stride, reflect=reflect, stats=acc if served else None)
    err = (y.double() - ref).abs().max().item()
    bar = (5e-5 if gn else 2e-5) * max(1.0, ref.abs().max().item())
    print("%s: max|d| vs fp64 %.3g (bar %.3g)" % (what, err, bar))
    assert y.shape == ref.shape and err <= bar
    if served:
        _check_own_stats(what, acc, y, _gn_params(cout, 5))
    acc2 = _acc(n)
    y2 = ops.convk(x, gn_arg, gn, packed, stride, reflect=reflect, stats=acc2 if served else None)
    assert torch.equal(y, y2) and torch.equal(acc, acc2)


def test_convk_refusals():
    from monoport_amd import _lib, ops
    assert not ops.convk_supported(3, 64, 7, 2, 7, 128)     # H % stride
    assert not ops.convk_supported(3, 64, 7, 1, 8, 96)      # output width % 64
    assert not ops.convk_supported(16, 96, 3, 2, 8, 128)    # Cout % 128
    assert not ops.convk_supported(24, 128, 3, 2, 8, 128)   # Cin % 16
    x = torch.randn((1, 48, 6, 128), device=DEV)
    packed = ops.PackedConvK(torch.randn((128, 48, 3, 3), device=DEV))
    with pytest.raises(_lib.MonoportError, match="Cin % 32"):
        ops.convk(x, torch.ones((1, 48, 2), device=DEV), True, packed, 2)
    with pytest.raises(_lib.MonoportError, match="output width"):
        ops.convk(torch.randn((1, 48, 6, 96), device=DEV), None, False, packed, 2)
    # reflection padding wants a map larger than the padding (as nn.ReflectionPad2d does): 7x7 on 2 or 3 rows
    stem = ops.PackedConvK(torch.randn((64, 3, 7, 7), device=DEV))
    for h in (2, 3):
        with pytest.raises(_lib.MonoportError, match="reflection padding"):
            ops.convk(torch.randn((1, 3, h, 64), device=DEV), None, False, stem, 1, reflect=True)
    assert ops.convk(torch.randn((1, 3, 4, 64), device=DEV), None, False, stem, 1, reflect=True).shape == (1, 64, 4, 64)


# ---- fused 1x1 ----------------------------------------------------------------------------------

# (N, C1, C2, Cout, H, W, gn): segment sizes at odd multiples of 64 and the limit, one workgroup per image (hw = 64)
# and pixel counts that are no powers of two
CONV1X1 = [(1, 64, 0, 256, 8, 8, False), (5, 192, 0, 256, 8, 24, True), (1, 320, 64, 256, 24, 40, True),
           (5, 448, 192, 256, 8, 8, True), (1, 512, 320, 256, 8, 24, True), (5, 512, 0, 128, 8, 8, True),
           (1, 192, 448, 128, 24, 40, False), (5, 64, 0, 128, 8, 24, False)]


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("mrw", [0, 1, 2])
@pytest.mark.parametrize("n,c1,c2,cout,h,w,gn", CONV1X1)
def test_conv1x1_over_its_predicate(n, c1, c2, cout, h, w, gn, mrw, precision):
    """mp_conv1x1_ex: GroupNorm input with 2 .. 16 channels per group, second K segment, bias, residual; 256 output
    channels with statistics (against the float64 moments of y) and the channels-last copy, 128 without -- where
    statistics or a channels-last output are refused."""
    from monoport_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(c1 + c2 + cout + h * w + n)
    x1 = (torch.randn((n, c1, h, w), generator=g) * 1.5 + 0.2).to(DEV)
    x2 = torch.randn((n, c2, h, w), generator=g).to(DEV) if c2 else None
    res = torch.randn((n, cout, h, w), generator=g).to(DEV)
    w1 = (torch.randn((cout, c1), generator=g) * (1.0 / c1) ** 0.5).to(DEV)
    w2 = (torch.randn((cout, c2), generator=g) * (1.0 / c2) ** 0.5).to(DEV) if c2 else None
    b1 = torch.randn(cout, generator=g).to(DEV)
    gn_in = _gn_params(c1, 6) if gn else None
    gn_arg = (_acc_of(x1), gn_in) if gn else None
    with torch.no_grad():
        v = _gn_relu64(x1, gn_in) if gn else x1.double()
        ref = F.conv2d(v, w1.double()[:, :, None, None], b1.double()) + res.double()
        if c2:
            ref = ref + F.conv2d(x2.double(), w2.double()[:, :, None, None])
    packed = ops.PackedConv1x1(w1, b1, w2, None, precision=precision)
    wide = cout == 256
    hwc = torch.full((n, h, w, 256), 7.0, device=DEV)
    what = "conv1x1 %s mrw %d %s" % (precision, mrw, (n, c1, c2, cout, h, w))
    lib.mp_conv3x3_tune(mrw << 12)
    try:
        if not wide:
            with pytest.raises(_lib.MonoportError, match="built for 256 channels"):
                ops.conv1x1_fused(x1, gn_arg, gn, x2, packed, res=res, stats=_acc(n))
            with pytest.raises(_lib.MonoportError, match="built for 256 channels"):
                ops.conv1x1_fused(x1, gn_arg, gn, x2, packed, res=res, y_hwc=hwc)
            assert (hwc == 7.0).all()
        acc, acc2 = _acc(n), _acc(n)
        y = ops.conv1x1_fused(x1, gn_arg, gn, x2, packed, res=res, y_hwc=hwc if wide else None, stats=acc if wide else None)
        y2 = ops.conv1x1_fused(x1, gn_arg, gn, x2, packed, res=res, stats=acc2 if wide else None)
    finally:
        lib.mp_conv3x3_tune(0)
    err = (y.double() - ref).abs().max().item()
    bar = (5e-5 if gn else 2e-5) * max(1.0, ref.abs().max().item())
    print("%s: max|d| vs fp64 %.3g (bar %.3g)" % (what, err, bar))
    assert y.shape == ref.shape and err <= bar
    assert torch.equal(y, y2) and torch.equal(acc, acc2)
    if wide:
        assert torch.equal(hwc, y.permute(0, 2, 3, 1).contiguous())
        _check_own_stats(what, acc, y, _gn_params(cout, 7))


@pytest.mark.parametrize("c1,c2,cout,hw,words", [(576, 0, 256, 64, ("at most 512", "576")), (64, 0, 192, 64, ("128 or 256", "-> 192")),
                                                 (96, 0, 256, 64, ("multiples of 64", "96 + 0")), (64, 96, 256, 64, ("multiples of 64", "64 + 96")),
                                                 (64, 0, 256, 96, ("H*W a multiple of 64", ", 96)"))])
def test_conv1x1_refusals(c1, c2, cout, hw, words):
    """mp_conv1x1_ex called directly (PackedConv1x1 itself refuses other Cout): status, reason, y untouched."""
    from monoport_amd import _lib, ops
    lib = _lib.load()
    n = 2
    x1 = torch.zeros((n, c1, hw), device=DEV)
    x2 = torch.zeros((n, max(c2, 1), hw), device=DEV)
    wp = torch.zeros((cout * (c1 + c2),), device=DEV)
    wmax = torch.zeros((1,), device=DEV)
    y = torch.full((n, cout, hw), 7.0, device=DEV)
    for f16 in (0, 1):
        a = _lib.Conv1x1Args()
        a.x1, a.n, a.c1, a.c2, a.cout, a.hw = x1.data_ptr(), n, c1, c2, cout, hw
        if c2:
            a.x2 = x2.data_ptr()
        a.packed, a.wmax, a.f16, a.y = wp.data_ptr(), wmax.data_ptr(), f16, y.data_ptr()
        ctx = ops.get_encoder_context(torch.device(DEV))
        rc = lib.mp_conv1x1_ex(ctx.handle, ctypes.byref(a), None)
        torch.cuda.synchronize()
        msg = lib.mp_last_error(ctx.handle).decode()
        assert rc != 0 and all(wd in msg for wd in words), (rc, msg)
        assert (y == 7.0).all()


# ---- the modules at widths whose statistics are not served ---------------------------------------

def _seeded(module, seed):
    from monoport_amd import synthetic as syn
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict({k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(shapes, seed).items()})
    return module.to(DEV).eval()


@pytest.mark.parametrize("c_in,c_out", [(384, 384), (128, 384)])
def test_convblock_at_a_width_without_served_statistics(monkeypatch, c_in, c_out):
    """ConvBlock(., 384): convolutions of 192, 96 and 96 output channels.  Every shape passes mp_conv3x3_supported, but
    the statistics bn2 / bn3 need are not served there, so the block stays on the torch ops -- and gives the float64
    module's output (1e-4, the encoders' feature bar)."""
    import copy
    from monoport_amd import ops
    from monoport_amd.modeling import backbones
    monkeypatch.setattr(backbones, "ENCODER_CONV", "hip")
    monkeypatch.setattr(backbones, "ENCODER_CONV_MIN_H", 32)
    blk = _seeded(backbones.ConvBlock(c_in, c_out), 5)
    x = torch.randn((2, c_in, 32, 64), generator=torch.Generator().manual_seed(c_in)).to(DEV)
    assert all(ops.conv3x3_supported(c.in_channels, c.out_channels, 32, 64) for c in (blk.conv1, blk.conv2, blk.conv3))
    with torch.no_grad():
        assert not blk._fused_ok(x)
        got = blk(x)
        ref = copy.deepcopy(blk).double()(x.double())
    err = (got.double() - ref).abs().max().item()
    print("ConvBlock(%d, %d): max|d| vs the float64 module %.3g (max|ref| %.3g)" % (c_in, c_out, err, ref.abs().max().item()))
    assert got.shape == ref.shape and err <= 1e-4
    ctl = _seeded(backbones.ConvBlock(256, 256), 5)  # the control: the stock width stays on the fused kernels
    with torch.no_grad():
        assert ctl._fused_ok(torch.zeros((2, 256, 32, 64), device=DEV))


@pytest.mark.parametrize("last", [False, True])
def test_resblock_at_a_width_without_served_statistics(monkeypatch, last):
    """The residual block of a ResnetFilter(ngf = 48): two reflect-padded 192 -> 192 convolutions with a GroupNorm
    between them.  The shape passes mp_conv3x3_supported, its statistics are not served: the block stays on the torch
    ops and gives the float64 module's output."""
    import copy
    from monoport_amd import ops
    from monoport_amd.modeling import backbones
    monkeypatch.setattr(backbones, "ENCODER_CONV", "hip")
    blk = _seeded(backbones._ResBlock(192, last=last), 6)
    x = torch.randn((2, 192, 32, 64), generator=torch.Generator().manual_seed(7)).to(DEV)
    assert ops.conv3x3_supported(192, 192, 32, 64)
    with torch.no_grad():
        assert not blk._fused_ok(x)
        got = blk(x)
        ref = copy.deepcopy(blk).double()(x.double())
    err = (got.double() - ref).abs().max().item()
    print("_ResBlock(192, last=%s): max|d| vs the float64 module %.3g (max|ref| %.3g)" % (last, err, ref.abs().max().item()))
    assert got.shape == ref.shape and err <= 1e-4
    with torch.no_grad():
        assert _seeded(backbones._ResBlock(256, last=last), 6)._fused_ok(torch.zeros((2, 256, 32, 64), device=DEV))
