"""The float64 model of the f16 query kernels (oracle/split_precision.py) and the bars the GPU tests
(tests/test_query16_gpu.py) hold the kernels to.  CPU only.

How the bars were fixed: for every case of the GPU sweep (``sweep_case``: a random and a body head,
Cout 1 sigmoid and Cout 3 tanh, plain and skip-table kernel, the same points) the model was run with
float64 sums and with float32 sums in the kernel's k16 order; the largest |f64 - f32| per precision and
Cout is the accumulation-noise spread, and each bar is a round number between 1x and 4x of it.
``test_bars_are_a_small_multiple_of_the_accumulation_spread`` re-measures that.  The max bar
catches a wrong term anywhere; the median bar (same rule, on the median over points) catches a wrong
arithmetic that only moves every point a little.  The sensitivity tests then check that each
"nearest wrong kernel" -- f16w with one layer's lo term dropped, with one layer's 1/S off by 2, f16
in place of f16w -- lands >= 5x a bar away from the model on the same inputs.

Where the rule cannot be met -- plain f16 against f16w by the MAX bar: the f32 sums of a plain-f16
kernel move some pre-activations across an f16 rounding boundary, so single activations flip by a
whole f16 ulp and the max spread is of the same order as the whole f16-vs-f16w difference.  The
MEDIAN separates them (most points see no flip); that is what the f16 sensitivity test checks, and
the max bar stays a 4x-of-spread bar for f16 as for the others.
"""
import math

import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn
from test_oracle_golden import query_inputs

N_SWEEP = 1200  # points of every sweep case (about 2 % of them outside the image)

# max |kernel - model| and median over points of it, by (precision, Cout)
BAR = {("f16x3", 1): 5e-7, ("f16x3", 3): 2e-5,
       ("f16w", 1): 5e-7, ("f16w", 3): 2e-5,
       ("f16", 1): 1e-4, ("f16", 3): 5e-4}
BAR_MEDIAN = {("f16x3", 1): 5e-8, ("f16x3", 3): 2e-7,
              ("f16w", 1): 5e-8, ("f16w", 3): 2e-7,
              ("f16", 1): 1e-7, ("f16", 3): 3e-7}
PRECISIONS = ("f16x3", "f16w", "f16")


def three_output(layers):
    """A Cout = 3 tanh head from a netG head: output 0 keeps the head's own row, outputs 1-2 are
    random rows over the same hidden units and features (as test_three_output_head_through_the_skip_table)."""
    rs = np.random.RandomState(5)
    w4, b4 = layers[-1]
    w = rs.uniform(-0.1, 0.1, (3, w4.shape[1])).astype(np.float32)
    b = rs.uniform(-0.1, 0.1, (3,)).astype(np.float32)
    w[0] += w4[0]
    b[0] += b4[0]
    return layers[:-1] + [(w, b)]


def sweep_case(head, cout):
    """(layers, last_op, feat, points, calib) of one GPU sweep case."""
    if head == "body":
        layers, feat = syn.body_mlp("G", noise=0.05, seed=13), syn.body_feat(256, 128, 128, 23)
    else:
        layers, feat = syn.rand_mlp("G", 11, 2.0), syn.rand_feat(256, 128, 128, 21)
    if cout == 3:
        layers = three_output(layers)
    pts = syn.rand_points(N_SWEEP, 31, 1.1)
    calib = syn_calib(40)
    return layers, (1 if cout == 1 else 2), feat, pts, calib


def syn_calib(step):
    from oracle import pifu_oracle
    return pifu_oracle.pifu_calib(*syn.scene_camera(step))[0]


def range_head():
    """Weight ranges where S matters: layer 0 spans 1e-3 .. 40 (columns scaled up), layer 1's max|W|
    is exactly 0.5 (S exact at a power of two), layer 2's weights are ~1e-6 (S clamped at 2^14, the
    lo halves in the f16 subnormals), layer 3 plain."""
    layers = syn.rand_mlp("G", 21, 2.0)
    w0, b0 = layers[0]
    w0 = w0.copy()
    w0[:, :8] *= np.float32(700.0)
    w0[:4, 256] = np.float32(40.0)
    w1, b1 = layers[1]
    w1 = w1.copy()
    w1[3, 7] = np.float32(-0.5)
    w2, b2 = layers[2]
    w2 = (w2 * np.float32(1e-6 / np.abs(w2).max())).astype(np.float32)
    return [(w0, b0), (w1, b1), (w2, b2)] + layers[3:]


def range_case():
    return range_head(), 1, syn.rand_feat(256, 128, 128, 21), syn.rand_points(N_SWEEP, 32, 1.1), syn_calib(60)


@pytest.fixture(scope="module")
def sp(oracle):
    from oracle import split_precision
    return split_precision


def _run(sp, case, precision, table, acc="f64", **kw):
    layers, last_op, feat, pts, calib = case
    return sp.query_emulated(feat, pts, calib, layers, last_op, syn.Z_SCALE, precision, table=table, acc=acc, **kw)


# ---------------------------------------------------------------------------------------------
def test_layer_scales_rule(sp):
    def head(wmaxes):
        return [(np.full((2, 3), m, np.float32), np.zeros(2, np.float32)) for m in wmaxes] + [None]
    s = sp.layer_scales(head([1.0, 0.5, 40.0, 3e-3]))
    assert s == [2.0 ** 13, 2.0 ** 14, 2.0 ** 8, 2.0 ** 14]  # 3e-3 hits the upper clamp
    # a power-of-two maximum is scaled exactly to 2^13 (frexp(2^k) = 0.5 * 2^(k+1)), not to 2^14
    for k in range(-1, 28):
        (sk,) = sp.layer_scales([(np.array([[2.0 ** k, -0.25 * 2.0 ** k]], np.float32), None)])
        assert sk * 2.0 ** k == 2.0 ** 13, k
    # clamps: tiny and huge weights, all-zero layers
    assert sp.layer_scales([(np.array([[1e-7]], np.float32), None)]) == [2.0 ** 14]
    assert sp.layer_scales([(np.array([[3e8]], np.float32), None)]) == [2.0 ** -14]
    assert sp.layer_scales([(np.zeros((2, 2), np.float32), None)]) == [1.0]
    rs = np.random.RandomState(0)
    for _ in range(200):
        w = (rs.standard_normal((4, 4)) * 10.0 ** rs.uniform(0.5, 7.5)).astype(np.float32)  # inside the clamps
        (s1,) = sp.layer_scales([(w, None)])
        assert np.abs(w).max() * s1 <= 2.0 ** 14 < np.abs(w).max() * s1 * 2
        assert math.log2(s1) == int(math.log2(s1))


def test_scaling_lifts_tiny_weights_out_of_the_f16_subnormals(sp):
    rs = np.random.RandomState(1)
    w = (rs.uniform(0.5, 1.0, 4096) * 1e-7 * rs.choice([-1, 1], 4096)).astype(np.float32)
    f16_min_normal = 2.0 ** -14
    assert (np.abs(w) < f16_min_normal).all()  # unscaled: every one subnormal (or zero) in f16
    (s,) = sp.layer_scales([(w[None], None)])
    hi, lo = sp.split((w * np.float32(s)).astype(np.float32))
    assert (np.abs(hi) >= f16_min_normal).all()
    # S is clamped at 2^14, so lo (~1e-3 2^-11) still sits in the f16 subnormals: the pair is exact to
    # half a subnormal step, 2^-25 / S -- about 2^-16 relative here, where f16(w) alone is off by ~30 %
    err = np.abs((hi + lo) / s - w).max()
    assert err <= 2.0 ** -25 / s
    assert np.abs(w.astype(np.float16).astype(np.float64) - w).max() >= 1000 * err


def test_f16x3_model_is_f32_class_on_the_goldens(sp, oracle):
    """f16x3 drops only lo*lo (2^-22 relative per product): against the fp64 oracle within the
    existing f16x3 bar of 2e-5.  The body golden's fp64 oracle also samples in f64 (3.2e-5 away from
    the f32 sampling every kernel does, k = 40 amplifies it), so there the model is held to 2e-5
    against the exact float64 MLP on the kernels' f32 samples, and the golden's f32 reference output."""
    for name in ("query_G_rand", "query_G_body"):
        g = load_golden(name)
        kind, layers, f, p = query_inputs(name)
        p = p[:, :3000]
        cal = g["calib"][0]
        for table in (False, True):
            m = sp.query_emulated(f, p, cal, layers, 1, syn.Z_SCALE, "f16x3", table=table)
            exact = sp.query_emulated(f, p, cal, layers, 1, syn.Z_SCALE, "f64", table=table)
            ref64 = oracle.query(f, p, cal, layers, 1, syn.Z_SCALE, precision="f64")
            e_exact, e64, e_gold = (np.abs(m - r).max() for r in (exact, ref64, g["out"][:, :3000]))
            print("%s table=%d: |f16x3 model - exact| %.3g, - fp64 oracle %.3g, - reference %.3g"
                  % (name, table, e_exact, e64, e_gold))
            assert e_exact <= 2e-5 and e_gold <= 2e-5
            if name == "query_G_rand":
                assert e64 <= 2e-5
            xyz = oracle.orthogonal(p, cal)
            outside = np.minimum(1 - np.abs(xyz[0]), 1 - np.abs(xyz[1])) < 0
            assert (m[:, outside] == 0).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cout", [1, 3])
def test_bars_are_a_small_multiple_of_the_accumulation_spread(sp, precision, cout):
    """spread <= BAR <= 4 x spread, spread = max over the sweep heads and paths of |model(f64 sums) -
    model(f32 sums)|; the same for the median bar.  The weight-range head (Cout 1) must sit inside
    the Cout-1 bars too (its GPU test uses them)."""
    spreads, medians = [], []
    cases = [sweep_case(h, cout) for h in ("rand", "body")] + ([range_case()] if cout == 1 else [])
    for i, case in enumerate(cases):
        for table in (False, True):
            d = np.abs(_run(sp, case, precision, table) - _run(sp, case, precision, table, acc="f32"))
            if i < 2:
                spreads.append(d.max())
                medians.append(np.median(d))
            else:
                assert d.max() <= BAR[precision, cout] and np.median(d) <= BAR_MEDIAN[precision, cout]
    s, m = max(spreads), max(medians)
    print("%s Cout %d: spread max %.3g -> bar %.3g (%.1fx); median %.3g -> bar %.3g (%.1fx)"
          % (precision, cout, s, BAR[precision, cout], BAR[precision, cout] / s, m,
             BAR_MEDIAN[precision, cout], BAR_MEDIAN[precision, cout] / m))
    assert s <= BAR[precision, cout] <= 4 * s
    assert m <= BAR_MEDIAN[precision, cout] <= 4 * m


def _distances(sp, case, table, precision, **wrong):
    ref = _run(sp, case, precision, table)
    d = np.abs(_run(sp, case, wrong.pop("as_precision", precision), table, **wrong) - ref)
    return d.max(), np.median(d)


@pytest.mark.parametrize("head", ["rand", "body"])
@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
def test_wrong_f16w_kernels_are_5x_the_bar_away(sp, head, table):
    """f16w with one layer's lo term dropped (layers 0-3; the table kernel has no f16 layer 0), with one
    layer's 1/S off by 2, and f16 in place of f16w: each >= 5 x BAR away by the max over points."""
    case = sweep_case(head, 1)
    bar = BAR["f16w", 1]
    variants = {"f16": dict(as_precision="f16")}
    for l in range(1 if table else 0, 4):
        variants["lo%d" % l] = dict(layer_terms=[1 if k == l else 2 for k in range(4)])
        variants["1/S x2 layer %d" % l] = dict(inv_scale_mult=[2.0 if k == l else 1.0 for k in range(4)])
    for name, kw in variants.items():
        dmax, _ = _distances(sp, case, table, "f16w", **kw)
        print("f16w %s %s: bar %.3g, wrong kernel '%s' at %.3g (%.0fx)" % (head, "table" if table else "plain",
                                                                        bar, name, dmax, dmax / bar))
        assert dmax >= 5 * bar, name


@pytest.mark.parametrize("head", ["rand", "body"])
@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
def test_f16x3_and_f16_are_separated_from_f16w(sp, head, table):
    """f16x3 vs its nearest wrong kernel (f16w: lo*hi dropped) by the max bar on the random head (the
    body head's weights are f16-exact up to 1e-8 of output, there the two ARE the same arithmetic).
    f16 vs f16w: by the median bar on the random head (see the module docstring: not by the max); the
    body head saturates most points, so there only the max is checked where it separates (the plain
    kernel)."""
    case = sweep_case(head, 1)
    dmax, _ = _distances(sp, case, table, "f16x3", as_precision="f16w")
    print("f16x3 %s: bar %.3g, f16w at %.3g (%.0fx)" % (head, BAR["f16x3", 1], dmax, dmax / BAR["f16x3", 1]))
    if head == "rand":
        assert dmax >= 5 * BAR["f16x3", 1]
    dmax, dmed = _distances(sp, case, table, "f16", as_precision="f16w")
    print("f16 %s: max bar %.3g, f16w at %.3g (%.1fx); median bar %.3g, f16w at %.3g (%.0fx)"
          % (head, BAR["f16", 1], dmax, dmax / BAR["f16", 1], BAR_MEDIAN["f16", 1], dmed,
             dmed / BAR_MEDIAN["f16", 1]))
    if head == "rand":
        assert dmed >= 5 * BAR_MEDIAN["f16", 1]
    elif not table:
        assert dmax >= 5 * BAR["f16", 1]
