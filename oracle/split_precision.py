"""Float64 model of the split-precision query kernels (monoport_amd/csrc/query16.hip) -- TEST
INFRASTRUCTURE ONLY.

``oracle.query`` evaluates MonoPortNet.query exactly; the f16 kernels deliberately do not.  This
module restates the arithmetic each of them CLAIMS to do -- every operand rounding at the point the
kernel rounds it -- and evaluates the rest in float64 (``acc="f64"``) or with float32 sums in the
kernel's k16 order (``acc="f32"``).  The distance between the two modes is the CPU-side estimate of
accumulation noise; a kernel that computes a different arithmetic sits much further from the model
than that (tests/test_split_precision_cpu.py measures how much further).

What the kernels round, and where (file:line as of this module's writing)
-------------------------------------------------------------------------
* Weights (pack.hip:115-119, :130-133): v = f32(W * S) with S = 2^e per layer (``layer_scales``,
  api.hip:377-386), split hi = f16(v), lo = f16(v - hi).  S is a power of two, so W * S is exact in
  f32 and lo stays out of the f16 subnormals for every weight above 2^-14 max|W|.
* Products (query16.hip:91-92, seg_main16 :154-173): TERMS = 3 ("f16x3") hi*hi + hi*lo + lo*hi
  (weight part first), TERMS = 2 ("f16w") Wh*xh + Wh*xl, TERMS = 1 ("f16") Wh*xh.  Each product of
  two halves is exact in f32; MFMA sums 16 of them into an f32 accumulator (modelled: one f32
  rounding per k16 group and term, term-major inside a group).
* Activations -- sampled features (:418-424), hidden units (:273-288, :294-308): the f32 value is
  split the same way, hi = f16(x), lo = f16(x - hi).  For TERMS = 1 the lo half is never read.
* z column (ZPair, :201-231, :429-437, :766-770): z_feat = f32(z * z_scale) is split into (hi, lo)
  like any activation and enters as one more k16 group with the layer's z weights (scaled and split
  like the others) -- so for "f16" z_feat is rounded to f16 too.
* Biases (init_from_bias16, :233-241): accumulators start at f32 bias * S -- exact, the bias is
  never rounded to f16.
* 1/S (finish16 :244-250, convert_store_q128 :273-288): y = acc * f32(1/S), exact (a power of
  two), then leaky ReLU max(y, 0.01 y) in f32.
* Layer 4 (:599-669): f32 on the VALU with the f32 weights: hidden units of layer 3 as f32 (never
  split), the features as (float)xh + (float)xl (:640) -- the 22-bit value of the split, for every
  precision including "f16" -- and z_feat in f32 (:662).  Then sigmoid / tanh, exact 0 outside
  the image (:663).

``table=True`` models pifu_query16_tab_kernel (:676-999), the kernel MONOPORT_TAB16=all routes every
precision to: every product of a weight with the sampled feature comes from the f32 skip table
(skip_table_kernel, f32 weights, f32 sums) blended with the bilinear tap weights.  So:
* layer 0 (:795-806) is f32 on the VALU, b0 + z_feat w0z + blend(T0) with unscaled f32 weights,
  leaky ReLU, then split for layer 1 -- no f16 weight and no S in layer 0;
* the skip rows of layers 1-3 (init_skip :822-832) enter as S * bias + S * blend(T_l) in f32;
* still on f16 MFMA: the hidden segments of layers 1-3 and their z columns (gemm_z16 :877, :909,
  :939), with the same weight split, TERMS and 1/S as the plain kernel;
* layer 4 (:945-996): hidden part as in the plain kernel, the feature part is the exact f32 table
  row (not the 22-bit split), z_feat in f32.
The model takes the table's products in float64 (``acc="f64"``) or as one float32 GEMM
(``acc="f32"``); blending before or after the product is the same number up to f32 rounding.

Projection and sampling reuse pifu_oracle.orthogonal / sample in f32: bit-identical to the kernels'
project() / make_taps() / blend() (query_common.h), checked against the reference's goldens.

Out of scope: activations above 65504 (they saturate in f16) and heads with max|W| >= 2^29.
"""
import math

import numpy as np

from oracle import pifu_oracle as orc

TERMS = {"f16x3": 3, "f16w": 2, "f16": 1, "f64": 1}
HIDDEN = (1024, 512, 256, 128)  # kHidden (mp_internal.h): the netG head these kernels are built for
C = 256


def layer_scales(layers):
    """S per hidden layer 0-3: the largest power of two with max|W| * S <= 2^14, the exponent
    clamped to [-14, 14] (api.hip:377-386; max|W| over the whole weight matrix, not the bias)."""
    out = []
    for w, _ in layers[:4]:
        wmax = float(np.abs(np.asarray(w, np.float32)).max())
        e = 0
        if 0.0 < wmax < 3.0e38:
            e = 14 - math.frexp(wmax)[1]  # wmax = f 2^e', f in [0.5, 1)
        e = min(max(e, -14), 14)
        out.append(math.ldexp(1.0, e))
    return out


def split(v):
    """(hi, lo) of the f16 pair of v: hi = f16(v), lo = f16(v - hi), as float64 arrays.  v is a
    float32 array (the kernels split f32 values) or float64 (the model's own activations)."""
    v = np.asarray(v)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(v.dtype)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _exact(v):
    """precision "f64": the operand itself as the hi part, no rounding at all."""
    v = np.asarray(v, np.float64)
    return v, np.zeros_like(v)


def _terms(wpair, xpair, t):
    (wh, wl), (xh, xl) = wpair, xpair
    return [(wh, xh), (wh, xl), (wl, xh)][:t]


def _gemm(acc, segs, t, mode):
    """acc += sum over segments (wpair [R,K], xpair [K,N]) of the t-term product.  f64: exact
    float64 sums.  f32: one float32 rounding per k16 group and term, segments in order, groups in
    order, term-major inside a group (seg_main16 / gemm_z16)."""
    if mode == "f64":
        for wpair, xpair in segs:
            for w, x in _terms(wpair, xpair, t):
                acc = acc + w @ x
        return acc
    for wpair, xpair in segs:
        k = wpair[0].shape[1]
        ops = [(w.astype(np.float32), x.astype(np.float32)) for w, x in _terms(wpair, xpair, t)]
        for g in range(0, k, 16):
            for w, x in ops:
                acc = acc + w[:, g:g + 16] @ x[g:g + 16]  # float32 throughout
    return acc


def _lrelu(y, mode):
    if mode == "f64":
        return np.where(y > 0, y, 0.01 * y)
    y = y.astype(np.float32)
    return np.maximum(y, (y * np.float32(0.01)).astype(np.float32))


def query_emulated(feat, points, calib, layers, last_op, z_scale, precision, table=False, acc="f64",
                   layer_terms=None, inv_scale_mult=None):
    """The arithmetic of query16.hip for one head: [Cout, N] float64 (``acc="f64"``) or float32.

    feat [256,H,W] f32; points [3,N] f32; calib [>=3,4]; layers = [(W[out,in], b[out])] x 5 (netG
    shapes, Cout 1 or 3); last_op 1 sigmoid / 2 tanh; precision "f16x3" / "f16w" / "f16", or "f64"
    for no operand rounding at all (MonoPortNet.query in float64 on the kernels' f32 sampling);
    table=True models the skip-table kernel.  ``layer_terms`` (4 ints) and ``inv_scale_mult`` (4
    floats) override TERMS and the 1/S factor per layer -- the "wrong kernels" of the sensitivity
    tests; leave them None for the kernel's own arithmetic."""
    assert acc in ("f64", "f32") and precision in TERMS
    feat = np.ascontiguousarray(feat, np.float32)
    points = np.ascontiguousarray(points, np.float32)
    assert feat.shape[0] == C and len(layers) == 5
    terms = list(layer_terms) if layer_terms is not None else [TERMS[precision]] * 4
    mult = list(inv_scale_mult) if inv_scale_mult is not None else [1.0] * 4
    f64 = acc == "f64"
    ftype = np.float64 if f64 else np.float32
    xyz = orc.orthogonal(points, calib, "f32")
    inside = (xyz[0] >= -1) & (xyz[0] <= 1) & (xyz[1] >= -1) & (xyz[1] <= 1)
    x32 = orc.sample(feat, xyz[:2], "f32")                       # [C, N], the kernels' blend bits
    z32 = (xyz[2] * np.float32(z_scale)).astype(np.float32)[None]  # [1, N]
    sp = _exact if precision == "f64" else split
    xpair, zpair = sp(x32), sp(z32)
    scales = layer_scales(layers)

    a = None  # activations of the previous layer (float64, or float32 in the f32 mode)
    for l in range(4):
        w32 = np.asarray(layers[l][0], np.float32)
        b32 = np.asarray(layers[l][1], np.float32)
        kh = w32.shape[1] - C - 1
        wx = w32[:, kh:kh + C]
        if table and l == 0:
            # f32 VALU: b0 + z w0z + blend(T0), no S, no f16 weights (l0_finish)
            if f64:
                pre = b32[:, None] + w32[:, C:C + 1].astype(np.float64) * z32 + wx.astype(np.float64) @ x32
            else:
                pre = (b32[:, None] + w32[:, C:C + 1] * z32).astype(np.float32) + (wx @ x32).astype(np.float32)
            a = _lrelu(pre.astype(ftype), acc)
            continue
        s = scales[l]
        ws = (w32 * np.float32(s)).astype(np.float32)
        segs = []
        if kh:
            segs.append((sp(ws[:, :kh]), sp(a)))
        if not table:
            segs.append((sp(ws[:, kh:kh + C]), xpair))
        segs.append((sp(ws[:, kh + C:]), zpair))
        n = x32.shape[1]
        init = np.broadcast_to(b32[:, None] * np.float32(s), (w32.shape[0], n)).astype(ftype)
        if table:  # S * bias + S * blend(T_l)
            skip = wx.astype(np.float64) @ x32 if f64 else (wx @ x32).astype(np.float32)
            init = (init + skip * ftype(s)).astype(ftype)
        accum = _gemm(init, segs, terms[l], acc)
        y = (accum * ftype((1.0 / s) * mult[l])).astype(ftype)
        a = _lrelu(y, acc)

    w4 = np.asarray(layers[4][0], np.float32)
    b4 = np.asarray(layers[4][1], np.float32)
    kh = w4.shape[1] - C - 1
    xs = x32.astype(np.float64) if table or precision == "f64" else xpair[0] + xpair[1]  # (float)xh + (float)xl, exact in f32
    if f64:
        v = (b4[:, None] + w4[:, :kh].astype(np.float64) @ a + w4[:, kh:kh + C].astype(np.float64) @ xs
             + w4[:, kh + C:].astype(np.float64) * z32)
        out = 1.0 / (1.0 + np.exp(-v)) if last_op == 1 else np.tanh(v) if last_op == 2 else v
    else:
        v = (b4[:, None] + w4[:, :kh] @ a + (w4[:, kh:kh + C] @ xs.astype(np.float32))).astype(np.float32)
        v = (v + w4[:, kh + C:] * z32).astype(np.float32)
        with np.errstate(over="ignore"):
            out = (np.float32(1) / (np.float32(1) + np.exp(-v)) if last_op == 1 else np.tanh(v) if last_op == 2
                   else v)
    return np.where(inside[None], out, 0.0).astype(ftype)
