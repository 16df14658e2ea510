"""The float64 model of the GroupNorm statistics producers hand on (oracle/gn_stats.py) and the bars
tests/test_gn_offset_gpu.py holds the kernels to.  CPU only.

The bars are 3-4x the pivoted model's worst case over ``sweep`` (derivation: oracle/gn_stats.py);
``test_bars_are_a_small_multiple_of_the_pivoted_worst_case`` re-measures that, and the teeth test
checks that the arithmetic without a pivot -- what the kernels did before -- misses them by >= 10x
from |mean| / std = 100 on."""
import math

import numpy as np
import pytest

from oracle import gn_stats as gs

RATIOS = (0.0, 1.0, 10.0, 100.0, 1e3, 1e4)
STDS = (1.0, 1e-2)
LENGTHS = (32, 64, 256, 1024)
GROUP = 8 * 128 * 128  # one GroupNorm(32, 256) group of a 128 x 128 map


def _group(ratio, sign, std, seed=0):
    z = np.random.RandomState(seed).randn(GROUP)
    return (sign * ratio * std + std * z).astype(np.float32)


def sweep(pivot, ratios=RATIOS, lengths=LENGTHS):
    """Worst (rstd, mean) error of the model per ratio over both signs, STDS and ``lengths``."""
    worst = {}
    for r in ratios:
        er = em = 0.0
        for std in STDS:
            for sign in (1, -1):
                x = _group(r, sign, std)
                want = gs.truth(x)
                for L in lengths:
                    a, b = gs.errors(gs.model(x, L, pivot), want)
                    er, em = max(er, a), max(em, b)
        worst[r] = (er, em)
    return worst


@pytest.mark.parametrize("sign_k", (1, -1))
@pytest.mark.parametrize("sign_m", (1, -1))
def test_pivot_algebra_is_exact(sign_k, sign_m):
    """sum x = s1 + n K, sum x^2 = s2 + 2 K s1 + n K^2: exact up to double rounding when s1 / s2 are exact."""
    rs = np.random.RandomState(3)
    x = (sign_m * 300.0 + rs.randn(1000)).astype(np.float64)
    for K in (sign_k * 297.5, sign_k * 1e-3, 0.0, sign_k * 1e4):
        d = x - K
        a, b = gs.fold(math.fsum(d), math.fsum(d * d), float(x.size), K)
        # double rounding of n K, n K^2 and 2 K s1: a few ulps of the largest term
        big = x.size * (abs(K) + 300.0) ** 2
        assert abs(a - math.fsum(x)) <= 4 * 2.0 ** -52 * x.size * (abs(K) + 300.0)
        assert abs(b - math.fsum(x * x)) <= 8 * 2.0 ** -52 * big


def test_run_sums_use_the_run_pivot_and_the_real_count():
    x = np.array([5.0, 6.0, 7.0, 9.0, -2.0, -1.0], np.float32)
    s1, s2, n, K = gs.run_partials(x, 4)
    assert K.tolist() == [5.0, -2.0] and n.tolist() == [4.0, 2.0]
    assert s1.tolist() == [0 + 1 + 2 + 4, 0 + 1] and s2.tolist() == [0 + 1 + 4 + 16, 0 + 1]
    a, b = gs.fold(s1, s2, n, K)
    assert a.tolist() == [27.0, -3.0] and b.tolist() == [25 + 36 + 49 + 81, 4 + 1]


def test_masked_positions_contribute_nothing():
    """A padded / masked lane adds 0 -- not K and K^2: n counts the real values only, and a run whose
    first lanes are masked takes its pivot from a real one."""
    rs = np.random.RandomState(5)
    x = (1e3 + rs.randn(4096)).astype(np.float32)
    mask = rs.rand(4096) > 0.3
    mask[:64] = False  # whole leading runs and the head of the next one masked
    padded = np.where(mask, x, np.float32(0))
    for L in (32, 100, 256):
        got = gs.model(padded, L, mask=mask)
        r, m = gs.errors(got, gs.truth(x[mask]))
        assert r <= gs.RSTD_BAR and m <= gs.MEAN_BAR
        s1, s2, n, K = gs.run_partials(padded, L, mask=mask)
        assert n.sum() == mask.sum() and np.all(K[n > 0] != 0)
    # counting the masked lanes as real values (the mistake the mask guards against) is far off
    wrong = gs.model(padded, 256)
    assert gs.errors(wrong, gs.truth(x[mask]))[0] > 1e3 * gs.RSTD_BAR


def test_pivoted_model_meets_the_bars():
    for r, (er, em) in sweep(True).items():
        assert er <= gs.RSTD_BAR and em <= gs.MEAN_BAR, "ratio %g: rstd %.3g mean %.3g" % (r, er, em)


def test_bars_are_a_small_multiple_of_the_pivoted_worst_case():
    w = sweep(True)
    er = max(v[0] for v in w.values())
    em = max(v[1] for v in w.values())
    print("pivoted model, worst: rstd %.3g, mean %.3g" % (er, em))
    assert 2.5 * er <= gs.RSTD_BAR <= 5 * er
    assert 2.5 * em <= gs.MEAN_BAR <= 5 * em


def test_unpivoted_model_misses_the_bar():
    """Teeth: K = 0 (the kernels' arithmetic before the pivot) at |mean| / std = 100 with the run
    lengths of the elementwise producers (256) and longer: >= 10x over the rstd bar, worse above."""
    w = sweep(False, ratios=(100.0, 1e3, 1e4), lengths=(256, 1024))
    for r, (er, em) in w.items():
        print("unpivoted ratio %g: rstd %.3g mean %.3g" % (r, er, em))
        assert er >= 10 * gs.RSTD_BAR
    assert w[1e3][0] >= 1e3 * gs.RSTD_BAR and w[1e3][1] >= 10 * gs.MEAN_BAR


def test_constant_group_gives_one_over_sqrt_eps():
    for c in (3.7, -100.3, 1234.5):
        x = np.full(GROUP, c, np.float32)
        mean, rstd = gs.model(x, 256)
        assert mean == np.float64(np.float32(c)) and rstd == pytest.approx(1.0 / np.sqrt(gs.EPS), rel=1e-9)


def test_accumulator_round_trip_near_the_limit():
    """Sum of squares of one group near 2^44 (the bars hold; the format needs < 2^46)."""
    x = _group(1e4, 1, 1.6)[:65536]
    q = float(np.sum(x.astype(np.float64) ** 2))
    assert 2.0 ** 43 < q < 2.0 ** 45 < gs.SUMSQ_LIMIT
    r, m = gs.errors(gs.model(x, 256), gs.truth(x))
    assert r <= gs.RSTD_BAR and m <= gs.MEAN_BAR
