"""The kernels between the convolutions (csrc/encoder_ops.hip) restated from their definitions in float64; with them
what their CPU and GPU tests share: a float32 model of the bicubic kernel's op order, the admission rule of the banded
upsample kernel restated, the shape lattices and the seeded inputs.  tests/test_elementwise_ref_cpu.py holds the
restatements to torch's float64 CPU ops; tests/test_elementwise_admitted_shapes_gpu.py holds the kernels to the
restatements.  torch and numpy only, CPU or GPU tensors, no HIP."""
import numpy as np
import torch

BICUBIC_A = -0.75


# ---- the operations -----------------------------------------------------------------------------------------------

def avgpool2(x):
    """avg_pool2d(x, 2, stride 2) of x [..., H, W] (H, W even): the float64 mean of each 2 x 2 window."""
    v = x.double()
    return (v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2]) * 0.25


def cubic_weights(t):
    """The four cubic-convolution weights (A = -0.75) of the taps at -1, 0, 1, 2 for a fraction t, in t's own
    precision; op order of upsample_get_cubic_coefficients."""
    a = t.dtype.type(BICUBIC_A)
    one, two, three, four, five, eight = (t.dtype.type(v) for v in (1, 2, 3, 4, 5, 8))
    x0, x1, x2, x3 = t + one, t, one - t, two - t
    return np.stack((((a * x0 - five * a) * x0 + eight * a) * x0 - four * a,
                     ((a + two) * x1 - (a + three)) * x1 * x1 + one,
                     ((a + two) * x2 - (a + three)) * x2 * x2 + one,
                     ((a * x3 - five * a) * x3 + eight * a) * x3 - four * a), 1)


def bicubic_axis(n_in):
    """One axis of interpolate(scale_factor=2, mode="bicubic", align_corners=True) on a float32 tensor: (clamped tap
    indices int64 [2 n_in, 4], fraction float32 [2 n_in]).  The source coordinate is the float32 product of the float32
    scale (in - 1) / (out - 1) and the output index -- part of the operation; floor and fraction split it exactly."""
    n_out = 2 * n_in
    scale = np.float32(n_in - 1) / np.float32(n_out - 1)
    r = scale * np.arange(n_out, dtype=np.float32)
    assert r.dtype == np.float32
    f = np.floor(r)
    idx = np.clip(f.astype(np.int64)[:, None] + np.arange(-1, 3)[None], 0, n_in - 1)
    return idx, r - f


def bicubic2x(x, add=None):
    """[add +] interpolate(x [..., H, W], scale_factor=2, mode="bicubic", align_corners=True) as torch defines it for a
    float32 x: float32 source coordinates (bicubic_axis), weights, the 16 clamped taps and the addition in float64."""
    h, w = x.shape[-2:]
    v = x.double()
    (iy, ty), (ix, tx) = bicubic_axis(h), bicubic_axis(w)
    wy = torch.from_numpy(cubic_weights(ty.astype(np.float64))).to(v.device)
    wx = torch.from_numpy(cubic_weights(tx.astype(np.float64))).to(v.device)
    iy, ix = torch.from_numpy(iy).to(v.device), torch.from_numpy(ix).to(v.device)
    rows = sum(v[..., iy[:, j], :] * wy[:, j, None] for j in range(4))  # [..., 2H, W]
    out = sum(rows[..., ix[:, i]] * wx[:, i] for i in range(4))         # [..., 2H, 2W]
    return out if add is None else out + add.double()


def bicubic2x_f32_model(x, add=None):
    """The same operation evaluated in float32 in the op order of bicubic2x_at (csrc/encoder_ops.hip), every product
    and sum rounded on its own (no FMA): what a correct float32 kernel computes.  numpy [..., H, W] float32."""
    x = np.asarray(x, np.float32)
    h, w = x.shape[-2:]
    (iy, ty), (ix, tx) = bicubic_axis(h), bicubic_axis(w)
    wy, wx = cubic_weights(ty), cubic_weights(tx)
    assert wy.dtype == np.float32 and wx.dtype == np.float32
    acc = np.zeros(x.shape[:-2] + (2 * h, 2 * w), np.float32)
    for j in range(4):
        src = x[..., iy[:, j], :]
        row = np.zeros_like(acc)
        for i in range(4):
            row += src[..., ix[:, i]] * wx[:, i]
        acc += row * wy[:, j, None]
    return acc if add is None else np.asarray(add, np.float32) + acc


def _moments(t, groups):
    """float64 two-pass mean / biased variance per (image, group) of t [N,C,H,W]."""
    n = t.shape[0]
    v = t.double().reshape(n, groups, -1)
    mean = v.mean(2)
    var = ((v - mean[..., None]) ** 2).mean(2)
    return mean, var


def scale_shift(x, groups, weight, bias, eps):
    """(scale, shift) [N,C,2] in float64 of GroupNorm(groups, C) over x [N,C,H,W], from the definition:
    scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    cpg = x.shape[1] // groups
    mean, var = _moments(x, groups)
    rstd = 1.0 / torch.sqrt(var + eps)
    sc = rstd.repeat_interleave(cpg, 1) * weight.double()[None]
    sh = bias.double()[None] - mean.repeat_interleave(cpg, 1) * sc
    return torch.stack((sc, sh), 2)


def group_norm(x, groups, weight, bias, eps, relu=False, res=None):
    """[res +] relu?(GroupNorm(groups, C)(x)) in float64, two passes."""
    cpg = x.shape[1] // groups
    mean, var = _moments(x, groups)
    mean = mean.repeat_interleave(cpg, 1)[..., None, None]
    rstd = (1.0 / torch.sqrt(var + eps)).repeat_interleave(cpg, 1)[..., None, None]
    y = (x.double() - mean) * rstd * weight.double()[None, :, None, None] + bias.double()[None, :, None, None]
    if relu:
        y = torch.relu(y)
    return y if res is None else y + res.double()


# ---- the inputs ---------------------------------------------------------------------------------------------------

def values(shape, seed):
    """0.2 + 1.7 N(0, 1), float32, from a seeded CPU generator."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 1.7 + 0.2


def noise(shape, seed):
    """N(0, 1), float32, from a seeded CPU generator: the ``add`` / ``res`` operands."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def row_seed(row):
    return 1000 + sum((i + 1) * int(v) for i, v in enumerate(row))


def upsample_inputs(shape):
    """(x [N,C,h,w], add [N,C,2h,2w]) of an upsample row, CPU float32."""
    n, c, h, w = shape
    return values(shape, row_seed(shape)), noise((n, c, 2 * h, 2 * w), row_seed(shape) + 1)


# ---- the lattices (tests/test_elementwise_admitted_shapes_gpu.py states the covering rules) ------------------------

AVGPOOL_ROWS = [(1, 32, 2, 8), (3, 96, 6, 8), (2, 96, 10, 24), (1, 160, 2, 1024), (1, 64, 1024, 8), (5, 32, 24, 40),
                (2, 256, 64, 64)]

# (N, C, h, w, route, class): the kernel launch_upsample_add_gn takes and the clause of its rule that decides
UPSAMPLE_ROWS = [
    (1, 512, 8, 2, "banded", "banded"), (2, 1024, 8, 128, "banded", "banded"), (1, 32, 128, 8, "banded", "banded"),
    (3, 96, 128, 16, "banded", "banded"), (1, 256, 16, 64, "banded", "banded"), (2, 128, 32, 32, "banded", "banded"),
    (1, 32, 8, 8, "element", "slice"), (1, 96, 64, 16, "element", "slice"),
    (1, 256, 4, 64, "element", "band"), (1, 256, 12, 32, "element", "band"),
    (2, 64, 16, 6, "element", "width"), (1, 32, 3, 2, "element", "band"), (1, 32, 2, 2, "element", "band"),
    (1, 32, 16, 256, "element", "wide"), (1, 32, 256, 256, "element", "wide"),
]
UPSAMPLE_CLASSES = ("banded", "wide", "width", "band", "slice")
UPSAMPLE_NO_ADD = [(1, 512, 8, 2), (1, 32, 8, 8)]  # add = None: the first row of each route
UPSAMPLE_PLAIN = [(1, 1, 2, 2), (2, 3, 2, 129), (2, 3, 129, 2)]  # upsample_bicubic2x: any C, odd sizes

GN_APPLY_ROWS = [(1, 32, 2, 2), (3, 96, 3, 4), (2, 160, 5, 12), (1, 512, 1, 4), (7, 64, 8, 1024), (1, 32, 1024, 1024)]

# (N, C, H, W, groups)
GROUP_NORM_ROWS = [(1, 32, 2, 2, 32), (2, 24, 6, 10, 1), (2, 24, 6, 10, 3), (3, 40, 2, 2, 40), (1, 2, 1024, 1024, 2)]


# 256 (kGnThreads), 16 (kUpBand) and 256 (kGnSlices * kUpBand) of csrc/encoder_ops.hip are restated here as literals: if
# one of them changes, test_library_predicate_is_the_restated_rule (test_elementwise_ref_cpu.py) is what shows it.
def upsample_class(c, h, w):
    """The first clause of launch_upsample_add_gn's admission rule a [N,c,h,w] input misses, in the order the rule
    states them -- "wide": 2W > 256; "width": 2W does not divide 256; "band": 2H % 16 != 0; "slice":
    (C / 32 * 2H) % 256 != 0 -- or "banded" if it misses none."""
    ho, wo = 2 * h, 2 * w
    if wo > 256:
        return "wide"
    if 256 % wo:
        return "width"
    if ho % 16:
        return "band"
    if (c // 32 * ho) % 256:
        return "slice"
    return "banded"


def upsample_route(c, h, w):
    """"banded" (upsample_add_gn_kernel) or "element" (ew_gn_kernel<UpsampleAddOp>): mp_upsample_gn_banded restated."""
    return "banded" if upsample_class(c, h, w) == "banded" else "element"
