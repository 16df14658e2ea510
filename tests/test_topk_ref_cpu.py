"""The numpy restatement of the fixed-budget octree refinement (tests/topk_ref.py) against brute force and against
dense evaluation; the constructor contract of Seg3dTopk.  No GPU."""
import numpy as np
import pytest

import topk_ref
from oracle import pifu_oracle as po

BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]


def _volume(seed=7, r=17):
    """Random 17^3 volume with planted plateaus of exact ties, NaNs and an evaluated mask."""
    rng = np.random.default_rng(seed)
    cur = rng.random((r, r, r), dtype=np.float32)
    cur[3:6, :, 2:9] = 0.625
    cur[10, 4:12, :] = 0.375   # the same distance from 0.5 as the plateau above
    cur[12:, 12:, 12:] = 0.5   # u == 0
    cur[rng.random((r, r, r)) < 0.02] = np.nan
    evaluated = rng.random((r, r, r)) < 0.3
    return cur, evaluated


def _brute(cur, evaluated, k, max_dist=None, balance=0.5):
    u = np.abs(cur - np.float32(balance)).reshape(-1)
    index = np.arange(u.size)
    cand = ~evaluated.reshape(-1) & ~np.isnan(u)
    if max_dist is not None:
        cand &= np.nan_to_num(u, nan=np.inf) <= np.float32(max_dist)
    index, u = index[cand], u[cand]
    return index[np.lexsort((index, u))[:k]]


@pytest.mark.parametrize("k", [0, 1, 5, 40, 150, 151, 152, 1000, 17 ** 3])
def test_select_topk_equals_brute_force(k):
    cur, evaluated = _volume()
    got = topk_ref.select_topk(cur, evaluated, k)
    assert np.array_equal(got, _brute(cur, evaluated, k))
    n_cand = int((~evaluated & ~np.isnan(cur)).sum())
    assert got.size == min(k, n_cand) and np.unique(got).size == got.size
    assert not evaluated.reshape(-1)[got].any() and not np.isnan(cur.reshape(-1)[got]).any()
    u = np.abs(cur.reshape(-1)[got] - np.float32(0.5))
    assert (np.diff(u) >= 0).all()
    ties = np.flatnonzero(np.diff(u) == 0)
    assert (got[ties] < got[ties + 1]).all()  # ties in u: the smaller linear index first


def test_select_topk_ties_plateaus_and_bounds():
    cur, evaluated = _volume()
    n_cand = int((~evaluated & ~np.isnan(cur)).sum())
    n_zero = int((~evaluated & (cur == 0.5)).sum())
    assert n_zero > 20
    # the u == 0 plateau comes first, in linear index order, whatever k cuts out of it
    first = topk_ref.select_topk(cur, evaluated, n_zero // 2)
    assert np.array_equal(first, np.flatnonzero((~evaluated & (cur == 0.5)).reshape(-1))[:n_zero // 2])
    assert topk_ref.select_topk(cur, evaluated, 0).size == 0
    assert topk_ref.select_topk(cur, evaluated, n_cand + 10).size == n_cand
    assert topk_ref.select_topk(cur, evaluated, 10 ** 9).size == n_cand
    # max_dist cuts below k; the two plateaus at distance 0.125 lie exactly on the bound and stay in
    near = topk_ref.select_topk(cur, evaluated, n_cand, max_dist=0.125)
    u = np.abs(cur - np.float32(0.5))
    want = ~evaluated & (np.nan_to_num(u, nan=np.inf) <= np.float32(0.125))
    assert 0 < near.size == int(want.sum()) < n_cand
    assert np.array_equal(np.sort(near), np.flatnonzero(want.reshape(-1)))
    assert np.array_equal(near, _brute(cur, evaluated, n_cand, max_dist=0.125))
    assert np.array_equal(topk_ref.select_topk(cur, evaluated, 7, max_dist=np.inf), _brute(cur, evaluated, 7))
    # another balance
    assert np.array_equal(topk_ref.select_topk(cur, evaluated, 300, balance=0.3),
                          _brute(cur, evaluated, 300, balance=0.3))


def _sphere(p):  # [3,N] f32 -> [N] f32
    d = np.sqrt((p.astype(np.float32) ** 2).sum(0, dtype=np.float32))
    return (1.0 / (1.0 + np.exp(-(np.float32(0.6) - d) * np.float32(12)))).astype(np.float32)


def test_seg3d_topk_full_budgets_equal_dense_evaluation():
    res = [9, 17, 33]
    stats = []
    vol = topk_ref.seg3d_topk(_sphere, BMIN, BMAX, res, [r ** 3 for r in res], stats=stats)
    assert np.array_equal(vol.view(np.uint32), po.dense_volume(_sphere, BMIN, BMAX, 33).view(np.uint32))
    # every node exactly once: a level evaluates what the coarser ones left
    assert stats == [9 ** 3, 17 ** 3 - 9 ** 3, 33 ** 3 - 17 ** 3]


def test_seg3d_topk_stats_budgets_and_empty():
    res = [9, 17, 33]
    stats = []
    vol = topk_ref.seg3d_topk(_sphere, BMIN, BMAX, res, [123456, 300, 0], stats=stats)
    assert stats == [9 ** 3, 300, 0]  # entry 0 is ignored, k == 0 only upsamples
    level1 = vol[::2, ::2, ::2]  # even nodes are copies of the level before
    assert np.array_equal(vol, po.upsample2x(level1))
    dense = po.dense_volume(_sphere, BMIN, BMAX, 17, 33)
    exact = level1 == dense
    assert exact[::2, ::2, ::2].all() and exact.sum() == 9 ** 3 + 300
    # the 300 evaluated nodes are the ones closest to the threshold among those level 0 left
    u = np.abs(po.upsample2x(dense[::2, ::2, ::2]) - np.float32(0.5))
    fresh = exact.copy()
    fresh[::2, ::2, ::2] = False
    rest = ~exact
    assert u[fresh].max() <= u[rest].min()
    # a bound per level: only nodes within 0.05 of the threshold, fewer than the budget
    stats = []
    topk_ref.seg3d_topk(_sphere, BMIN, BMAX, res, [0, 17 ** 3, 33 ** 3], max_dist=[None, 0.05, 0.05], stats=stats)
    assert 0 < stats[1] < 17 ** 3 - 9 ** 3 and 0 < stats[2] < 33 ** 3 - 17 ** 3
    # empty level 0: None, and only level 0 in the stats
    stats = []
    assert topk_ref.seg3d_topk(lambda p: np.zeros(p.shape[1], np.float32), BMIN, BMAX, res, [0, 10, 10],
                               stats=stats) is None
    assert stats == [9 ** 3]
    with pytest.raises(ValueError):
        topk_ref.seg3d_topk(_sphere, BMIN, BMAX, res, [0, 10])
    with pytest.raises(ValueError):
        topk_ref.seg3d_topk(_sphere, BMIN, BMAX, [9, 18], [0, 10])


def test_seg3d_topk_constructor_contract():
    """Seg3dTopk constructs (the stub raised), checks its arguments and shares the engine base with Seg3dLossless."""
    pytest.importorskip("torch")
    from monoport_amd.implicit_seg import functional as F
    box = dict(query_func=lambda **kw: None, b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]),
               resolutions=[9, 17, 33])
    eng = F.Seg3dTopk(num_points=[0, 100, 200], use_cuda_impl=True, faster=True, debug=True, **box)
    assert eng.num_points == [0, 100, 200] and eng.max_dist is None and eng.validate == "always"
    assert isinstance(eng, F._Seg3dEngine) and issubclass(F.Seg3dLossless, F._Seg3dEngine)
    assert F.Seg3dTopk.forward is F.Seg3dLossless.forward  # one validation / trust logic
    eng = F.Seg3dTopk(num_points=[0, 100, 200], clip_mins=[None, -0.25, -0.0], validate="first", **box)
    assert eng.max_dist == [float("inf"), 0.25, 0.0]
    with pytest.warns(UserWarning, match="clamped"):
        eng = F.Seg3dTopk(num_points=[10 ** 6, 17 ** 3 + 1, 33 ** 3], **box)
    assert eng.num_points == [9 ** 3, 17 ** 3, 33 ** 3]
    for bad in (dict(num_points=[0, 100]), dict(num_points=[0, 1, 2], clip_mins=[0.0, 0.0]),
                dict(num_points=[0, -1, 2]), dict(num_points=[0, 1, 2], clip_mins=[None, 0.5, None]),
                dict(num_points=[0, 1, 2], validate="never")):
        with pytest.raises(ValueError):
            F.Seg3dTopk(**box, **bad)
    for bad in (dict(align_corners=True), dict(visualize=True), dict(use_shadow=True), dict(channels=2),
                dict(fuse_views=True)):
        with pytest.raises(NotImplementedError):
            F.Seg3dTopk(num_points=[0, 1, 2], **box, **bad)
    with pytest.raises(NotImplementedError):
        F.Seg3dTopk(num_points=[0, 1], **{**box, "resolutions": [9, 19]})
    with pytest.warns(UserWarning, match="ignoring unknown arguments"):
        F.Seg3dTopk(num_points=[0, 1, 2], no_such_flag=1, **box)
    with pytest.raises(NotImplementedError, match="needs query_func, b_min, b_max, resolutions, num_points"):
        F.Seg3dTopk()  # upstream's required arguments
    with pytest.raises(NotImplementedError, match="needs num_points"):
        F.Seg3dTopk(**box)
