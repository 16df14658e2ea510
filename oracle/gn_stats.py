"""Float64 model of the GroupNorm statistics the encoder kernels hand on (csrc/gn_tail.h) -- TEST
INFRASTRUCTURE ONLY.

What every producer does with the f32 values it writes (conv3x3.hip conv_epilogue / conv1x1_kernel,
conv_wino.hip, convim2col.hip, encoder_ops.hip gn_partial_kernel / ew_gn_kernel /
upsample_add_gn_kernel):
  * a RUN of L values -- the pixels one lane or one half-wave adds up before anything goes to
    double -- is summed in f32 around a pivot K shared by the whole run (one of the run's own
    values): s1 = sum(x - K), s2 = sum fma(x - K, x - K, .);
  * the fold to double restores the plain sums, sum x = s1 + n K, sum x^2 = s2 + 2 K s1 + n K^2,
    with n the count of REAL values of the run (a masked lane adds 0 to s1 / s2, not K / K^2);
  * each workgroup's double sums go through gn_fixed (value = hi 2^-16 + lo 2^-64) and are added as
    integers (exact, order-independent);
  * the consumer (gn_mean_rstd) decodes them, mean = s / count, var = max(q / count - mean^2, 0),
    rstd = 1 / sqrt(var + eps) -- all in double before the cast to float.
``pivot=False`` is the arithmetic before the pivot was introduced (K = 0): the f32 sum of squares
of a group with |mean| / std = r carries about r^2 times more magnitude than its variance, so its
rounding error swamps the variance from r ~ 100 on.

The model sums each run SEQUENTIALLY in f32 (the kernels add in trees of DPP / shuffle steps, which
round less): it is an upper-bound model of the kernels' error, not a bit-exact one.

The bars (RSTD_BAR, MEAN_BAR) -- what tests/test_gn_offset_gpu.py holds every producer to, against
the float64 two-pass statistics of the tensor the kernel wrote:
  * error of the pivoted arithmetic: the run's f32 sums see only x - K, a few std in size, so s2 has
    a relative error of order sqrt(L) 2^-24 of sum (x - K)^2 -- no dependence on |mean| / std; the
    cross term 2 K s1 moves sum x^2 by 2 K e(s1) while e(s1) moves sum x by the same e(s1), so the
    variance only sees 2 (K - mean) e(s1) / count: again of the size of the std, not of the mean.
    The one place |mean| / std enters is double rounding of n K^2 and of mean^2 (2^-53 relative),
    i.e. 1e-16 r^2 on var: 1e-8 at r = 1e4.
  * measured (tests/test_gn_stats_cpu.py ``sweep``): |mean| / std in {0, 1, 10, 100, 1e3, 1e4},
    both signs, std 1 and 1e-2, L in {32, 64, 256, 1024}, 8 x 128 x 128 values per group: the worst
    |rstd / rstd64 - 1| is 1.2e-6 (r = 1e4, L = 1024) and the worst |mean - mean64| rstd64 is 7e-8
    (L = 1024).  The bars are 3-4x that: RSTD_BAR = 4e-6, MEAN_BAR = 2.5e-7.
  * the unpivoted arithmetic misses RSTD_BAR by > 10x at |mean| / std = 100 with runs of 256 or
    more (2e-4 at L = 256, std 1; ``test_unpivoted_model_misses_the_bar``) -- the bar has teeth.
Validity: every group's sum of squares below 2^46 (gn_fixed needs |x| < 2^46 and the int64 hi
word of the sum of ALL workgroups must not wrap); above 2^36 per workgroup gn_fixed rounds to
multiples of 2^-16, far below the bars for counts of the encoders' size.
"""
import numpy as np

RSTD_BAR = 4e-6  # |rstd / rstd64 - 1|
MEAN_BAR = 2.5e-7  # |mean - mean64| * rstd64
EPS = 1e-5       # nn.GroupNorm's default, the encoders' eps
SUMSQ_LIMIT = 2.0 ** 46


def run_partials(x, L, pivot=True, mask=None):
    """f32 run sums of x (1-D float32, producer order) in runs of L values: (s1, s2, n, K) per run.
    ``mask`` (bool, like x): False = a padded / masked position, which contributes nothing."""
    x = np.asarray(x, np.float32).ravel()
    m = np.ones(x.shape, bool) if mask is None else np.asarray(mask, bool).ravel()
    runs = -(-x.size // L)
    pad = runs * L - x.size
    xr = np.concatenate([x, np.zeros(pad, np.float32)]).reshape(runs, L)
    mr = np.concatenate([m, np.zeros(pad, bool)]).reshape(runs, L)
    if pivot:
        # the first real value of each run (0 for a run with none: it adds nothing anyway)
        first = np.argmax(mr, axis=1)
        K = np.where(mr.any(1), xr[np.arange(runs), first], np.float32(0)).astype(np.float32)
    else:
        K = np.zeros(runs, np.float32)
    d = np.where(mr, (xr - K[:, None]).astype(np.float32), np.float32(0)).astype(np.float32)
    s1 = np.zeros(runs, np.float32)
    s2 = np.zeros(runs, np.float32)
    for i in range(L):
        di = d[:, i]
        s1 = (s1 + di).astype(np.float32)
        # fmaf(d, d, s2): the product of two floats is exact in double; one rounding to f32 (up to double rounding)
        s2 = (s2.astype(np.float64) + di.astype(np.float64) * di.astype(np.float64)).astype(np.float32)
    return s1, s2, mr.sum(1).astype(np.float64), K


def fold(s1, s2, n, K):
    """The fold to double: (sum x, sum x^2) of each run."""
    s1, s2, K = np.float64(s1), np.float64(s2), np.float64(K)
    return s1 + n * K, s2 + 2.0 * K * s1 + n * K * K


def gn_fixed(v):
    """csrc/gn_tail.h gn_fixed on an array of doubles: (hi int64, lo uint64 < 2^48)."""
    xs = np.asarray(v, np.float64) * 65536.0
    fl = np.floor(xs)
    return fl.astype(np.int64), ((xs - fl) * 281474976710656.0).astype(np.uint64)


def acc_sum(values):
    """Integer adds of the fixed-point words (wrapping, as the atomics), decoded as the consumer does."""
    hi, lo = gn_fixed(values)
    with np.errstate(over="ignore"):
        h = np.sum(hi.astype(np.uint64), dtype=np.uint64).astype(np.int64)
        l = np.sum(lo, dtype=np.uint64)
    return float(h) / 65536.0 + float(l) / 18446744073709551616.0


def consumer(s, q, count, eps=EPS):
    """gn_mean_rstd before the cast to float."""
    mean = s / count
    var = max(q / count - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + eps)


def model(x, L, pivot=True, mask=None, eps=EPS):
    """(mean, rstd) the consumer derives from the producers' arithmetic, one group, each run one workgroup's add."""
    s1, s2, n, K = run_partials(x, L, pivot, mask)
    a, b = fold(s1, s2, n, K)
    count = float(n.sum())
    return consumer(acc_sum(a), acc_sum(b), count, eps)


def truth(x, eps=EPS):
    """Two-pass float64 statistics of the f32 values x (biased variance)."""
    v = np.asarray(x, np.float64).ravel()
    mean = v.mean()
    var = np.mean((v - mean) ** 2)
    return mean, 1.0 / np.sqrt(var + eps)


def errors(got, want):
    """(|rstd / rstd64 - 1|, |mean - mean64| rstd64) -- the two quantities the bars bound."""
    (m, r), (m64, r64) = got, want
    return abs(r / r64 - 1.0), abs(m - m64) * r64
