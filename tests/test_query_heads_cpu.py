"""Conditions on the inputs of tests/test_query_heads_gpu.py (tests/head_cases.py), checked without a GPU.  They are
not measurements of the kernels: they keep the GPU tests from hiding a failure -- enough points inside and outside
the image, logits that neither saturate sigmoid / tanh nor blow up, corner points both precisions agree on, two
float64 references that agree with each other, and yardsticks (the oracle's own float32 error) that stay small."""
import numpy as np
import pytest

import head_cases as hc
from monoport_amd import synthetic as syn
from oracle import pifu_oracle as orc

torch = pytest.importorskip("torch")

NORTH_STAR = 1e-4  # the project's bar against the reference: no yardstick may exceed it


def test_head_layers_draw_as_rand_mlp():
    """head_layers on the reference's own pairings IS syn.rand_mlp; the other pairings only change the widths."""
    for kind, (c, cout) in (("G", (256, 1)), ("C", (512, 3))):
        for (w, b), (w0, b0) in zip(hc.head_layers(c, cout, 17, 1.5), syn.rand_mlp(kind, 17, 1.5)):
            assert np.array_equal(w, w0) and np.array_equal(b, b0)
    for c, cout in hc.PAIRS:
        layers = hc.layers_of(c, cout)
        d = hc.head_dims(c, cout)
        assert [w.shape for w, _ in layers] == [(d[l + 1], d[l] + (d[0] if l else 0)) for l in range(5)]
        assert all(w.dtype == np.float32 and b.shape == (w.shape[0],) for w, b in layers)
    assert [w.shape for w, _ in hc.layers_of(256, 1)] == [tuple(s) for s in syn.layer_shapes("G")]
    assert [w.shape for w, _ in hc.layers_of(512, 3)] == [tuple(s) for s in syn.layer_shapes("C")]


@pytest.mark.parametrize("c", hc.CS)
def test_scene_shapes_corners_and_masks(c):
    f, p, calibs = hc.scene_views(c)
    assert f.shape == (hc.MAX_V, c, hc.H, hc.W) and (hc.H * hc.W) % 64 == 0  # a skip table is admitted
    assert p.shape == (3, 257) and 257 == 4 * 64 + 1 == 8 * 32 + 1
    assert calibs.shape == (hc.MAX_V, 4, 4) and len({cal.tobytes() for cal in calibs}) == hc.MAX_V
    # the first four points: exactly on the corners for the float32 projection of the kernels, inside for float64
    x32 = orc.orthogonal(p[:, :4], calibs[0], "f32")
    assert np.array_equal(x32[:2].T, np.array(hc.CORNERS, np.float32))
    x64 = hc.project64(p[:, :4], calibs[0])
    assert (np.abs(x64[:2]) < 1).all() and (np.abs(x64[:2]) > 1 - 1e-7).all()
    for v in range(hc.MAX_V):
        m32, m64 = hc.in_image(c, v), hc.in_image(c, v, "f64")
        assert np.array_equal(m32, m64)  # no point whose mask depends on the precision of the projection
        xy = hc.project64(p, calibs[v])[:2]
        border = np.abs(1 - np.abs(xy)).min(0)
        assert (border[4:] > 1e-5).all() and (v == 0 or (border[:4] > 1e-5).all())
        print("C = %d view %d: %d of 257 points in the image" % (c, v, int(m32.sum())))
        assert m32.mean() >= 0.5 and (~m32).mean() >= 0.1


@pytest.mark.parametrize("pair", hc.PAIRS, ids=hc.head_id)
def test_logits_neither_saturate_nor_blow_up(pair):
    c, cout = pair
    inside = hc.in_image(c)
    logit = hc.ref_query(c, cout, 0, "f64")
    assert logit.shape == (cout, 257) and (logit[:, ~inside] == 0).all()
    small = (np.abs(logit[:, inside]) < 2).all(0).mean()
    big = float(np.abs(logit).max())
    print("%s: %.1f %% of the in-image points have |logit| < 2, max |logit| %.3g" % (hc.head_id(pair), 100 * small, big))
    assert small >= 0.5 and big <= 20
    assert np.abs(logit[:, inside]).min(0).max() > 0.5  # ... and the field is not flat
    for i in range(cout):
        for j in range(i + 1, cout):  # the channels of a three-channel head differ
            assert np.abs(logit[i, inside] - logit[j, inside]).max() > 0.5
    # the bounded activations see both signs
    assert (logit[:, inside] > 0.2).any() and (logit[:, inside] < -0.2).any()


@pytest.mark.parametrize("head", hc.HEADS, ids=hc.head_id)
def test_views_restatement_with_one_view_is_the_oracle(head):
    """cpu_views / mlp_views (tests/test_query_views_cpu.py) at float64 with V = 1 against oracle.query at float64.
    The oracle hands its float64 result back as float32, so the restatement is rounded the same way first; after
    that the two agree to 1e-12 (in fact bit for bit)."""
    c, cout, last_op = head
    got = hc.ref_views(c, cout, last_op, 1, "f64")
    assert got.dtype == np.float64 and got.shape == (1, cout, 257)
    want = hc.ref_query(c, cout, last_op, "f64")
    err = float(np.abs(got[0].astype(np.float32).astype(np.float64) - want).max())
    print("%s: |cpu_views (V = 1) - oracle| at float64 = %.3g" % (hc.head_id(head), err))
    assert err <= 1e-12
    assert np.abs(got[0] - want).max() <= 2.0 ** -24 * max(1.0, np.abs(want).max())  # unrounded: half an ulp of float32
    # mlp_views alone, on explicit float64 features, against the numpy restatement of the direct form
    from test_query_views_cpu import mlp_views
    x = hc.direct_features(c).astype(np.float64)
    with torch.no_grad():
        y = mlp_views(hc.layers64(hc.layers_of(c, cout)), torch.from_numpy(x)[None], last_op).numpy()
    assert np.abs(y[0] - hc.mlp_numpy(hc.layers_of(c, cout), x, last_op)).max() <= 1e-12


@pytest.mark.parametrize("head", hc.HEADS, ids=hc.head_id)
def test_yardsticks(head):
    """y32 = |oracle float32 - oracle float64| per case, and the same for the multi-view and direct references: what
    the GPU tests scale their bars with.  None may exceed the project's 1e-4."""
    c, cout, last_op = head
    y = hc.y32(c, cout, last_op)
    yv = {v_n: hc.y32_views(c, cout, last_op, v_n) for v_n in (2, 3)}
    yd = float(np.abs(hc.ref_direct(c, cout, last_op, "f32") - hc.ref_direct(c, cout, last_op, "f64")).max())
    print("%s: y32 %.3g, views V=2 %.3g V=3 %.3g, direct %.3g" % (hc.head_id(head), y, yv[2], yv[3], yd))
    assert 0 < y <= NORTH_STAR and all(0 < e <= NORTH_STAR for e in yv.values()) and 0 < yd <= NORTH_STAR
    if last_op == 0:
        assert y <= hc.y0(c) <= NORTH_STAR and yv[2] <= hc.y0_views(c, 2) and yv[3] <= hc.y0_views(c, 3)


@pytest.mark.parametrize("c", hc.CS)
def test_views_differ_from_one_view(c):
    """The multi-view field is not the single-view one: a kernel that ignored the further views would be seen."""
    one = hc.ref_views(c, 1, 0, 1)[0]
    for v_n in (2, 3):
        many = hc.ref_views(c, 1, 0, v_n)
        assert many.shape == (v_n, 1, 257)
        both = hc.in_image(c, 0) & hc.in_image(c, 1)
        assert np.abs(many[0][:, both] - one[:, both]).max() > 0.1
        for v in range(v_n):  # row v carries view v's mask
            assert (many[v][:, ~hc.in_image(c, v)] == 0).all() and (many[v][:, hc.in_image(c, v)] != 0).all()


def test_body_head_has_a_surface():
    """The analytic (512, 1, sigmoid) head of the octree test: the oracle's dense 9^3 lattice has nodes on both sides
    of 0.5, and the widened weights are syn.body_mlp's on the shared rows."""
    layers = hc.body_layers(512)
    f, calib = hc.body_scene(512)
    ref = syn.body_mlp("C", noise=0.05, seed=0)
    for l in range(4):
        assert np.array_equal(layers[l][0][:2], ref[l][0][:2]) and np.array_equal(layers[l][1][:2], ref[l][1][:2])
    vol = orc.dense_volume(lambda q: orc.query(f, q, calib, layers, 1, syn.Z_SCALE, precision="f32")[0],
                           [-1, -1, -1], [1, 1, 1], 9, 33)
    assert (vol > 0.5).any() and (vol < 0.5).any()
