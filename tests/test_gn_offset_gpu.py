"""GroupNorm statistics of groups far from zero mean (csrc/gn_tail.h): every producer that turns f32
values into a group's (sum, sum of squares) -- the 3x3 kernels (direct, split-K, Winograd K64 / K128,
f32 and f16x3; raw output and block tail), the fused 1x1, the stems / stride-2 convolutions, the
elementwise producers, gn_stats -- fed groups with |mean| / std in {0, 10, 100, 1e3, 1e4}, both signs,
std 1 and 1e-2.  The accumulator's mean / rstd, decoded in double as gn_mean_rstd does before its
cast, against the float64 two-pass statistics of the tensor the kernel itself wrote, within the
bars of oracle/gn_stats.py (derivation there; tests/test_gn_stats_cpu.py).  Then the consumers'
GroupNorm prologues on inputs at |mean| / std = 1e3.  Needs an MI355X.

Every case keeps each group's sum of squares below 2^46 (gn_fixed and the int64 hi word need it);
``_check`` asserts that precondition."""
import math

import numpy as np
import pytest

from oracle import gn_stats as gs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

# (ratio, sign, std) per group, cycled over the 32 groups; std alternates, so shifting by an even
# number of groups keeps each group's std and changes its mean
GRID = [(r, s, sd) for r in (0.0, 10.0, 100.0, 1e3, 1e4) for s in (1.0, -1.0) for sd in (1.0, 1e-2)]
LARGE, SPLITK, K64, K128 = 0x100, 0x200, 0x800, 0x1000


def _plan(c, shift=0):
    """(mean, std) per channel of a c-channel tensor: group g gets GRID[(g + shift) % 20]."""
    mean, std = np.zeros(32), np.zeros(32)
    for g in range(32):
        r, s, sd = GRID[(g + shift) % len(GRID)]
        mean[g], std[g] = s * r * sd, sd
    cpg = c // 32
    return np.repeat(mean, cpg), np.repeat(std, cpg)


def _offset(n, c, h, w, seed, shift=0):
    """[N,C,H,W] f32 with the plan's mean / std per group."""
    g = torch.Generator().manual_seed(seed)
    mean, std = _plan(c, shift)
    z = torch.randn((n, c, h, w), generator=g, dtype=torch.float64)
    x = torch.from_numpy(mean)[None, :, None, None] + torch.from_numpy(std)[None, :, None, None] * z
    return x.float().to(DEV)


def _rows(cout, fan_in, seed, std):
    """Random weight rows [cout, fan_in] of unit L2 norm, row co scaled by std[co]."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, fan_in), generator=g, dtype=torch.float64)
    w = w / w.norm(dim=1, keepdim=True) * torch.from_numpy(std)[:, None]
    return w


def _acc(n):
    from monoport_amd import ops
    return ops.gn_acc_zeros(DEV, n)


def _decode(acc, count, eps=gs.EPS):
    """mean / rstd [N,32] from an accumulator [R,N,32,4], in double (gn_mean_rstd before its cast)."""
    a = acc.sum(0).cpu().numpy()  # integer adds of the replicas (wrapping, as the atomics)
    s = a[..., 0].astype(np.float64) / 65536.0 + a[..., 1].view(np.uint64).astype(np.float64) / 2.0 ** 64
    q = a[..., 2].astype(np.float64) / 65536.0 + a[..., 3].view(np.uint64).astype(np.float64) / 2.0 ** 64
    mean = s / count
    var = np.maximum(q / count - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + eps)


def _truth(t, eps=gs.EPS):
    """float64 two-pass mean / rstd / |mean| / std / sum of squares per (image, group) of t."""
    n = t.shape[0]
    v = t.double().reshape(n, 32, -1)
    mean = v.mean(2)
    var = ((v - mean[..., None]) ** 2).mean(2)
    sumsq = (v * v).sum(2)
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    ratio = np.abs(mean) / np.maximum(np.sqrt(var), 1e-300)
    return mean, 1.0 / np.sqrt(var + eps), ratio, sumsq.cpu().numpy()


def _decade(r):
    return 0.0 if r < 1.0 else 10.0 ** round(math.log10(r))


def _check(what, got, t, eps=gs.EPS):
    """got = (mean, rstd) [N,32] in double; t = the tensor the kernel wrote.  Prints the worst errors
    per decade of |mean| / std, then holds every group to the bars."""
    mean, rstd = got
    m64, r64, ratio, sumsq = _truth(t, eps)
    assert sumsq.max() < gs.SUMSQ_LIMIT, "%s: a group's sum of squares %.3g is past what gn_fixed holds" % (what, sumsq.max())
    er = np.abs(rstd / r64 - 1.0)
    em = np.abs(mean - m64) * r64
    dec = np.vectorize(_decade)(ratio)
    for d in sorted(set(dec.ravel().tolist())):
        sel = dec == d
        print("gn-offset %-28s ratio %-7g rstd %.2e mean %.2e" % (what, d, er[sel].max(), em[sel].max()))
    i = np.unravel_index(np.argmax(er / gs.RSTD_BAR + em / gs.MEAN_BAR), er.shape)
    assert er.max() <= gs.RSTD_BAR and em.max() <= gs.MEAN_BAR, (
        "%s: rstd %.3g (bar %.1g), mean %.3g (bar %.1g); worst group %s at |mean|/std %.3g"
        % (what, er.max(), gs.RSTD_BAR, em.max(), gs.MEAN_BAR, i, ratio[i]))


def _check_acc(what, acc, t, channels=None):
    if channels is not None:
        t = t[:, channels]
    count = (t.shape[1] // 32) * t.shape[2] * t.shape[3]
    _check(what, _decode(acc, count), t)


# ---- producers ---------------------------------------------------------------------------------

def _conv3x3_inputs(n, cin, cout, h, w, seed, dc, std=None):
    """x: channel 0 = 1, the others N(0, 1); weights: channel 0 only on the centre tap (= the plan's mean
    per output channel when ``dc``), the others random rows of norm std -- so y = mean + noise of ~std in
    every pixel, zero padding included."""
    mean, std_plan = _plan(cout)
    std = std_plan if std is None else std
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, cin, h, w), generator=g)
    x[:, 0] = 1.0
    wt = torch.zeros((cout, cin, 3, 3), dtype=torch.float64)
    wt[:, 1:] = _rows(cout, (cin - 1) * 9, seed + 1, std).reshape(cout, cin - 1, 3, 3)
    if dc:
        wt[:, 0, 1, 1] = torch.from_numpy(mean)
    return x.to(DEV), wt.float().to(DEV)


def _conv3x3_run(tune, x, packed, res):
    from monoport_amd import _lib, ops
    lib = _lib.load()
    n = x.shape[0]
    out = torch.empty((n, packed.cout, x.shape[2], x.shape[3]), device=DEV)
    acc_y, acc_o = _acc(n), _acc(n)
    lib.mp_conv3x3_tune(tune)
    try:
        y = ops.conv3x3_fused(x, None, packed, relu=False, stats=acc_y, out=out, res=res, out_off=0, out_stats=acc_o)
    finally:
        lib.mp_conv3x3_tune(0)
    torch.cuda.synchronize()
    return y, out, acc_y, acc_o


# (precision, tune); f16x3 has no Winograd kernel
CONV3X3 = [("f32", LARGE), ("f32", SPLITK), ("f32", K64), ("f32", K128), ("f16x3", LARGE), ("f16x3", SPLITK)]


SHAPES3X3 = [(2, 32, 128, 32, 32), (1, 16, 128, 8, 32), (3, 64, 64, 16, 64)]  # (N, Cin, Cout, H, W); 8 x 32: smallest map


@pytest.mark.parametrize("precision,tune,n,cin,cout,h,w",
                         [v + s for v in CONV3X3 for s in SHAPES3X3 if v[1] != K128 or s[2] % 128 == 0])
def test_conv3x3_statistics_of_offset_groups(precision, tune, n, cin, cout, h, w):
    """y (``stats``): the offset comes through the weights of a constant input channel (f32 only: the f16x3
    weight split would round the noise rows of a 1e4-scaled weight set); y + res (``out_stats``): through a
    per-channel constant in res."""
    from monoport_amd import ops
    f32 = precision == "f32"
    x, wt = _conv3x3_inputs(n, cin, cout, h, w, 7 * cin + cout + h, dc=f32)
    packed = ops.PackedConv3x3(wt, precision)
    if tune in (K64, K128):
        assert packed.wino is not None
    mean_y = _plan(cout)[0] if f32 else np.zeros(cout)
    mean_o = _plan(cout, shift=6)[0]
    res = torch.from_numpy(mean_o - mean_y).float()[None, :, None, None].expand(n, cout, h, w).contiguous().to(DEV)
    y, out, acc_y, acc_o = _conv3x3_run(tune, x, packed, res)
    what = "conv3x3 %s %s %s" % (precision, hex(tune), (n, cin, cout, h, w))
    _check_acc(what + " y", acc_y, y)
    _check_acc(what + " y+res", acc_o, out)
    assert torch.equal(out, y + res)


def test_conv3x3_batch_images_are_independent():
    """Image 0 offset by 1e3, image 1 centred: image 1's statistics are the bits of image 1 alone."""
    from monoport_amd import ops
    n, cin, cout, h, w = 2, 32, 128, 32, 32
    x, wt = _conv3x3_inputs(n, cin, cout, h, w, 5, dc=False, std=np.ones(cout))
    x[0, 0] = 1e3
    wt[:, 0, 1, 1] = 1.0  # y of image 0 = 1e3 + noise, of image 1 = 1 + noise
    packed = ops.PackedConv3x3(wt)
    res = torch.zeros((n, cout, h, w), device=DEV)
    res[1] = -1.0
    for tune in (LARGE, K64):
        y, out, acc_y, acc_o = _conv3x3_run(tune, x, packed, res)
        y1, out1, acc_y1, acc_o1 = _conv3x3_run(tune, x[1:].contiguous(), packed, res[1:].contiguous())
        assert torch.equal(y[1:], y1) and torch.equal(acc_y[:, 1:], acc_y1) and torch.equal(acc_o[:, 1:], acc_o1)
        _check_acc("conv3x3 batch %s y" % hex(tune), acc_y, y)
        _check_acc("conv3x3 batch %s y+res" % hex(tune), acc_o, out)


def test_conv3x3_tail_of_a_constant_group():
    """Zero weights: y + res = res, one constant per group (both signs) -- var = 0, rstd = 1 / sqrt(eps)."""
    from monoport_amd import ops
    n, cin, cout, h, w = 2, 32, 128, 32, 32
    packed = ops.PackedConv3x3(torch.zeros((cout, cin, 3, 3), device=DEV))
    x = torch.randn((n, cin, h, w), device=DEV)
    consts = torch.tensor([3.7, -100.3, 1234.5, -0.013] * 8).repeat_interleave(cout // 32)
    res = consts.float()[None, :, None, None].expand(n, cout, h, w).contiguous().to(DEV)
    for tune in (LARGE, SPLITK, K64, K128):
        _, out, _, acc_o = _conv3x3_run(tune, x, packed, res)
        mean, rstd = _decode(acc_o, (cout // 32) * h * w)
        assert np.array_equal(mean, np.tile(consts.float().double().numpy()[::cout // 32], (n, 1)))
        assert np.abs(rstd * math.sqrt(gs.EPS) - 1.0).max() <= 1e-6, hex(tune)


@pytest.mark.parametrize("n,h,w", [(2, 32, 32), (1, 8, 8)])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_conv1x1_statistics_of_offset_groups(precision, n, h, w):
    """The plan's mean enters as the bias (added after the f16x3 rescale, in f32)."""
    from monoport_amd import ops
    c1, cout = 64, 256  # the statistics epilogue is built for the 256-channel outputs
    mean, std = _plan(cout)
    wt = _rows(cout, c1, 3, std).float().to(DEV)
    g = torch.Generator().manual_seed(4)
    x = torch.randn((n, c1, h, w), generator=g).to(DEV)
    packed = ops.PackedConv1x1(wt, torch.from_numpy(mean).float().to(DEV), precision=precision)
    acc = _acc(n)
    y = ops.conv1x1_fused(x, None, False, None, packed, stats=acc)
    _check_acc("conv1x1 %s %s" % (precision, (n, h, w)), acc, y)


@pytest.mark.parametrize("ks,stride,cin,cout,h,w", [(7, 2, 3, 64, 8, 128), (7, 1, 3, 64, 4, 64), (3, 2, 16, 128, 4, 128),
                                                    (3, 2, 64, 256, 32, 128)])
def test_convk_statistics_of_offset_groups(ks, stride, cin, cout, h, w):
    """The 7x7 stem and the stride-2 3x3, the plan's mean as the bias."""
    from monoport_amd import ops
    n = 2
    mean, std = _plan(cout)
    wt = _rows(cout, cin * ks * ks, 8, std).reshape(cout, cin, ks, ks).float().to(DEV)
    g = torch.Generator().manual_seed(9)
    x = torch.randn((n, cin, h, w), generator=g).to(DEV)
    acc = _acc(n)
    y = ops.convk(x, None, False, ops.PackedConvK(wt, torch.from_numpy(mean).float().to(DEV)), stride, stats=acc)
    _check_acc("convk %dx%d s%d %s" % (ks, ks, stride, (cin, cout, h, w)), acc, y)


def _identity(n, c):
    ss = torch.zeros((n, c, 2), device=DEV)
    ss[..., 0] = 1.0
    return ss


@pytest.mark.parametrize("n,c,h,w", [(2, 64, 2, 2), (2, 256, 64, 64), (3, 32, 4, 12)])
def test_elementwise_statistics_of_offset_groups(n, c, h, w):
    """gn_apply (identity scale / shift: y = x), avgpool2_gn, upsample_add_gn (both kernels: the banded one
    and the per-element one for maps it does not serve), smallest maps included (idle lanes)."""
    from monoport_amd import ops
    x = _offset(n, c, h, w, 11)
    acc = _acc(n)
    y = ops.gn_apply(x, _identity(n, c), relu=False, stats=acc)
    assert torch.equal(y, x)
    _check_acc("gn_apply %s" % ((n, c, h, w),), acc, y)
    if h % 2 == 0 and (w // 2) % 4 == 0:
        acc_p = _acc(n)
        p = ops.avgpool2_gn(x, acc_p)
        _check_acc("avgpool2_gn %s" % ((n, c, h, w),), acc_p, p)
    if h <= 64:
        skip = _offset(n, c, 2 * h, 2 * w, 12, shift=4)
        centred = x - torch.from_numpy(_plan(c)[0]).float()[None, :, None, None].to(DEV)
        acc_u = _acc(n)
        u = ops.upsample_add_gn(centred, skip, acc_u)
        _check_acc("upsample_add_gn %s" % ((n, c, h, w),), acc_u, u)


def test_upsample_add_banded_kernel():
    """upsample_add_gn_kernel (Cout / 32 * 2H a multiple of 256, 2W dividing 256): offsets in x and in add."""
    from monoport_amd import ops
    n, c, h, w = 2, 128, 32, 32
    x = _offset(n, c, h, w, 13)
    skip = _offset(n, c, 2 * h, 2 * w, 14, shift=2) * 0.5
    acc = _acc(n)
    u = ops.upsample_add_gn(x, skip, acc)
    _check_acc("upsample_add_gn banded", acc, u)


def test_elementwise_constant_group_and_batch_independence():
    from monoport_amd import ops
    n, c, h, w = 2, 64, 32, 32
    consts = torch.tensor([3.7, -100.3, 1234.5, -0.013] * 8).repeat_interleave(c // 32)
    x = consts.float()[None, :, None, None].expand(n, c, h, w).contiguous().to(DEV)
    acc = _acc(n)
    ops.gn_apply(x, _identity(n, c), relu=False, stats=acc)
    mean, rstd = _decode(acc, (c // 32) * h * w)
    assert np.array_equal(mean, np.tile(consts.float().double().numpy()[::c // 32], (n, 1)))
    assert np.abs(rstd * math.sqrt(gs.EPS) - 1.0).max() <= 1e-6
    # image 0 offset by 1e3, image 1 centred: image 1's words are those of image 1 alone
    g = torch.Generator().manual_seed(15)
    z = torch.randn((n, c, h, w), generator=g).to(DEV)
    z[0] += 1e3
    acc2, acc1 = _acc(n), _acc(1)
    ops.gn_apply(z, _identity(n, c), relu=False, stats=acc2)
    ops.gn_apply(z[1:].contiguous(), _identity(1, c), relu=False, stats=acc1)
    assert torch.equal(acc2[:, 1:], acc1)
    _check_acc("gn_apply batch", acc2, z)
    accp2, accp1 = _acc(n), _acc(1)
    p = ops.avgpool2_gn(z, accp2)
    ops.avgpool2_gn(z[1:].contiguous(), accp1)
    assert torch.equal(accp2[:, 1:], accp1)
    _check_acc("avgpool2_gn batch", accp2, p)


def test_accumulator_near_two_to_the_44():
    """One group's sum of squares near 2^44 (|mean| 1.6e4, std 1.6, 8 x 128 x 128 values): the limit of the
    format is 2^46 (gn_fixed's |x| < 2^46 and the int64 hi word of the whole group)."""
    from monoport_amd import ops
    n, c, h, w = 1, 256, 128, 128
    g = torch.Generator().manual_seed(16)
    x = (1.6e4 + 1.6 * torch.randn((n, c, h, w), generator=g)).to(DEV)
    acc = _acc(n)
    ops.gn_apply(x, _identity(n, c), relu=False, stats=acc)
    sumsq = _truth(x)[3]
    assert 2.0 ** 43 < sumsq.max() < 2.0 ** 45
    _check_acc("gn_apply near 2^44", acc, x)


def test_gn_stats_and_finalize_of_offset_groups():
    """The legacy path: gn_stats' double partials (decoded as gn_finalize does) and gn_finalize's rstd."""
    from monoport_amd import ops
    for n, c, h, w in ((2, 256, 32, 32), (1, 64, 2, 2)):
        x = _offset(n, c, h, w, 17)
        partial, s = ops.gn_stats(x, 32)
        p = partial.reshape(n, 32, s, 2).sum(2).cpu().numpy()
        count = (c // 32) * h * w
        mean = p[..., 0] / count
        rstd = 1.0 / np.sqrt(np.maximum(p[..., 1] / count - mean * mean, 0.0) + gs.EPS)
        _check("gn_stats %s" % ((n, c, h, w),), (mean, rstd), x)
        ss = ops.gn_finalize((partial, s), n, c, 32, count, torch.ones(c, device=DEV), torch.zeros(c, device=DEV), gs.EPS)
        rstd32 = ss[..., 0].reshape(n, 32, c // 32)[..., 0].double().cpu().numpy()
        r64 = _truth(x)[1]
        assert np.abs(rstd32 / r64 - 1.0).max() <= gs.RSTD_BAR + 2.0 ** -23, "gn_finalize rstd"


# ---- consumers ---------------------------------------------------------------------------------

def _gn(c, seed):
    g = torch.Generator().manual_seed(seed)
    gn = torch.nn.GroupNorm(32, c)
    with torch.no_grad():
        gn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        gn.bias.copy_(torch.rand(c, generator=g) - 0.5)
    return gn.to(DEV)


def _gn64(x, gn):
    n, c = x.shape[:2]
    v = x.double().reshape(n, 32, -1)
    mean = v.mean(2, keepdim=True)
    var = ((v - mean) ** 2).mean(2, keepdim=True)
    v = ((v - mean) / torch.sqrt(var + gn.eps)).reshape(x.shape)
    return v * gn.weight.double()[None, :, None, None] + gn.bias.double()[None, :, None, None]


def _consumer_input(n, c, h, w, seed):
    """Every group at |mean| / std = 1e3, both signs, std 1 and 1e-2."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.tensor([1.0, 1.0, -1.0, -1.0] * 8, dtype=torch.float64).repeat_interleave(c // 32)
    std = torch.tensor([1.0, 1e-2] * 16, dtype=torch.float64).repeat_interleave(c // 32)
    x = (sign * 1e3 * std)[None, :, None, None] + std[None, :, None, None] * torch.randn((n, c, h, w), generator=g, dtype=torch.float64)
    return x.float().to(DEV)


def _acc_of(x):
    from monoport_amd import ops
    acc = _acc(x.shape[0])
    ops.gn_apply(x, _identity(x.shape[0], x.shape[1]), relu=False, stats=acc)
    return acc


def test_consumers_normalise_offset_groups():
    """gn_apply with the hand-over and ops.group_norm against float64 GroupNorm of the same f32 tensor; the
    bar is 2x the error of torch's own f32 nn.GroupNorm on the GPU + 1e-6."""
    from monoport_amd import ops
    for n, c, h, w in ((2, 256, 32, 32), (2, 64, 8, 8)):
        x = _consumer_input(n, c, h, w, 21)
        gn = _gn(c, 22)
        with torch.no_grad():
            ref = _gn64(x, gn)
            bar = 2.0 * (gn(x).double() - ref).abs().max().item() + 1e-6
        y = ops.gn_apply(x, (_acc_of(x), gn), relu=False)
        e = (y.double() - ref).abs().max().item()
        print("gn-offset consumer gn_apply %s: %.3g (bar %.3g)" % ((n, c, h, w), e, bar))
        assert e <= bar
        y2 = ops.group_norm(x, 32, gn.weight, gn.bias, gn.eps)
        e2 = (y2.double() - ref).abs().max().item()
        print("gn-offset consumer group_norm %s: %.3g (bar %.3g)" % ((n, c, h, w), e2, bar))
        assert e2 <= bar


def _conv_bar(scale_bar, conv64, x, gn, ref):
    """The kernel's existing scale-relative bar + 2x what torch's f32 GroupNorm error becomes through the same
    convolution (the f32 input of the conv carries |mean| / std 1e3 rounding no kernel can remove)."""
    with torch.no_grad():
        e_t = (conv64(torch.relu(gn(x).double())) - ref).abs().max().item()
    return scale_bar * max(1.0, ref.abs().max().item()) + 2.0 * e_t


def test_conv_consumers_normalise_offset_groups():
    from monoport_amd import _lib, ops
    lib = _lib.load()
    n, c, h, w = 2, 64, 32, 32
    x = _consumer_input(n, c, h, w, 23)
    gn = _gn(c, 24)
    acc = _acc_of(x)
    v64 = torch.relu(_gn64(x, gn))
    F = torch.nn.functional
    g = torch.Generator().manual_seed(25)
    # 3x3, direct and Winograd
    wt = (torch.randn((128, c, 3, 3), generator=g) * (2.0 / (9 * c)) ** 0.5).to(DEV)
    packed = ops.PackedConv3x3(wt)
    conv64 = lambda v: F.conv2d(v, wt.double(), padding=1)  # noqa: E731
    ref = conv64(v64)
    for tune, sbar in ((0x400 | LARGE, 3e-5), (0x400 | SPLITK, 3e-5), (K64, 1e-5), (K128, 1e-5)):
        lib.mp_conv3x3_tune(tune)
        try:
            y = ops.conv3x3_fused(x, (acc, gn), packed, relu=True)
        finally:
            lib.mp_conv3x3_tune(0)
        e, bar = (y.double() - ref).abs().max().item(), _conv_bar(sbar, conv64, x, gn, ref)
        print("gn-offset consumer conv3x3 %s: %.3g (bar %.3g)" % (hex(tune), e, bar))
        assert e <= bar
    # 1x1
    w1 = (torch.randn((128, c), generator=g) * (1.0 / c) ** 0.5).to(DEV)
    b1 = torch.randn(128, generator=g).to(DEV)
    p1 = ops.PackedConv1x1(w1, b1)
    conv64 = lambda v: F.conv2d(v, w1.double()[:, :, None, None], b1.double())  # noqa: E731
    ref = conv64(v64)
    y = ops.conv1x1_fused(x, (acc, gn), True, None, p1)
    e, bar = (y.double() - ref).abs().max().item(), _conv_bar(5e-5, conv64, x, gn, ref)
    print("gn-offset consumer conv1x1: %.3g (bar %.3g)" % (e, bar))
    assert e <= bar
    # 3x3 stride 2 (im2col kernel)
    xk = _consumer_input(n, c, h, 128, 26)
    acck = _acc_of(xk)
    wk = (torch.randn((128, c, 3, 3), generator=g) * (2.0 / (9 * c)) ** 0.5).to(DEV)
    conv64 = lambda v: F.conv2d(v, wk.double(), stride=2, padding=1)  # noqa: E731
    ref = conv64(torch.relu(_gn64(xk, gn)))
    y = ops.convk(xk, (acck, gn), True, ops.PackedConvK(wk), 2)
    e, bar = (y.double() - ref).abs().max().item(), _conv_bar(5e-5, conv64, xk, gn, ref)
    print("gn-offset consumer convk 3x3 s2: %.3g (bar %.3g)" % (e, bar))
    assert e <= bar
