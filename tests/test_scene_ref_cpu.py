"""The definitions of mp_texture_mips / mp_picture_texture / mp_picture_composite as tests/scene_ref.py restates them,
held to hand-made cases without a GPU: pyramid sizes against the library's own host-side count, level selection, the uv
seam rule, the wraps, the uncovered pixels and the composite's truth table.  And what FrameSlot(pictures={"scene": ...,
"composite": ...}) and the recon calls refuse before anything is allocated (device "cpu")."""
import itertools
import os
import re

import numpy as np
import pytest

import scene_ref as ref
from test_views_slot_cpu import _net

torch = pytest.importorskip("torch")
SIZES = [(1, 1), (2, 2), (5, 3), (64, 64), (8, 1)]
F = np.float32


@pytest.fixture(scope="module")
def lib():
    from monoport_amd import _lib, build
    build.build()
    return _lib.load()


def test_enums_match_the_header():
    from monoport_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "monoport_hip.h")).read()
    for name, ours, theirs in (("MP_WRAP_REPEAT", ref.WRAP_REPEAT, _lib.WRAP_REPEAT),
                               ("MP_WRAP_CLAMP", ref.WRAP_CLAMP, _lib.WRAP_CLAMP),
                               ("MP_COMPOSITE_OVER", ref.OVER, _lib.COMPOSITE_OVER),
                               ("MP_COMPOSITE_DEPTH", ref.DEPTH, _lib.COMPOSITE_DEPTH),
                               ("MP_NEAREST_MAX_Z", ref.MAX_Z, _lib.NEAREST_MAX_Z),
                               ("MP_NEAREST_MIN_Z", ref.MIN_Z, _lib.NEAREST_MIN_Z)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, header).group(1)) == ours == theirs, name


@pytest.mark.parametrize("ht,wt", SIZES)
def test_pyramid_sizes_and_offsets(lib, ht, wt):
    from monoport_amd import ops
    full = ref.max_levels(ht, wt)
    assert full == ops.texture_levels(ht, wt)
    assert ref.level_sizes(ht, wt, full)[-1] == (1, 1)
    tex = np.arange(ht * wt * 3, dtype=F).reshape(ht, wt, 3)
    for levels in range(1, full + 1):
        off = ref.level_offsets(ht, wt, levels)
        assert lib.mp_texture_pyramid_floats(ht, wt, levels) == off[-1] == ref.pyramid(tex, levels).size
        assert ops.texture_pyramid_floats(ht, wt, levels) == off[-1]
        assert [b - a for a, b in zip(off, off[1:])] == [3 * h * w for h, w in ref.level_sizes(ht, wt, levels)]
    # one level too many, and sizes out of range: the host-side count answers 0
    assert lib.mp_texture_pyramid_floats(ht, wt, full + 1) == 0
    assert lib.mp_texture_pyramid_floats(ht, wt, 0) == 0
    assert lib.mp_texture_pyramid_floats(0, wt, 1) == 0 and lib.mp_texture_pyramid_floats(ht, 8193, 1) == 0
    with pytest.raises(ValueError, match="levels"):
        ops.texture_pyramid_floats(ht, wt, full + 1)


def test_the_largest_texture_has_fourteen_levels(lib):
    assert ref.max_levels(8192, 8192) == 14 and ref.max_levels(8192, 1) == 14 and ref.max_levels(8191, 3) == 13
    assert lib.mp_texture_pyramid_floats(8192, 8192, 14) == 3 * sum(4 ** k for k in range(14))


def test_mip_levels_by_hand():
    tex = np.zeros((5, 3, 3), F)
    tex[..., 0] = np.arange(15, dtype=F).reshape(5, 3)
    m = ref.mips(tex)
    assert [a.shape[:2] for a in m] == [(5, 3), (2, 1), (1, 1)]
    # level 1 (0, 0): rows 0, 1 x columns 0, 1; (1, 0): rows 2, 3.  Level 2: rows 0, 1 of level 1, column 0 twice
    assert m[1][0, 0, 0] == F((0 + 1 + 3 + 4) * 0.25) and m[1][1, 0, 0] == F((6 + 7 + 9 + 10) * 0.25)
    assert m[2][0, 0, 0] == ((m[1][0, 0, 0] + m[1][0, 0, 0]) + (m[1][1, 0, 0] + m[1][1, 0, 0])) * F(0.25)
    # an odd size clamps: 3 x 3 -> 1 x 1 never reads row / column 2 twice, 1 x n repeats its one row
    one = ref.mips(np.arange(8 * 3, dtype=F).reshape(8, 1, 3))
    assert [a.shape[:2] for a in one] == [(8, 1), (4, 1), (2, 1), (1, 1)]
    assert one[1][0, 0, 0] == F((0 + 0 + 3 + 3) * 0.25)


@pytest.mark.parametrize("ht,wt", SIZES)
def test_a_constant_texture_stays_constant(ht, wt):
    tex = np.full((ht, wt, 3), F(0.3), F) * np.array([1, 2, 3], F)
    for level in ref.mips(tex):
        assert np.array_equal(level, np.broadcast_to(tex[0, 0], level.shape))


def quad_uv(h, w, ratio, ht=64, wt=64):
    """The UV picture of a fronto-parallel quad: ``ratio`` texels per pixel along both axes (exact in f32)."""
    uv = np.zeros((1, h, w, 3), F)
    uv[0, :, :, 0] = ((np.arange(h, dtype=F) + F(0.5)) * F(ratio) / F(wt))[:, None]
    uv[0, :, :, 1] = ((np.arange(w, dtype=F) + F(0.5)) * F(ratio) / F(ht))[None, :]
    return uv, np.zeros((1, h, w), np.int32)


@pytest.mark.parametrize("ratio,level", [(1, 0), (2, 1), (4, 2), (3, 2)])
def test_nearest_mip_selection(ratio, level):
    uv, face = quad_uv(6, 5, ratio)
    cov, got = ref.select_level(uv, face, 64, 64, 7)
    assert cov.all() and (got == level).all()
    # with fewer levels than that the coarsest one is taken
    assert (ref.select_level(uv, face, 64, 64, 2)[1] == min(level, 1)).all()
    assert (ref.select_level(uv, face, 64, 64, 1)[1] == 0).all()
    # an uncovered neighbour is no neighbour: a lone pixel has rho2 = 0
    face[:] = -1
    face[0, 3, 2] = 0
    cov, got = ref.select_level(uv, face, 64, 64, 7)
    assert cov.sum() == 1 and got[0, 3, 2] == 0


def test_neighbours_stay_inside_their_view():
    """Two views whose uv differ by many texels: the last row of view 0 does not look at the first row of view 1."""
    uv, face = quad_uv(4, 4, 1)
    two = np.concatenate([uv, uv + F(0.5)])
    assert (ref.select_level(two, np.concatenate([face, face]), 64, 64, 7)[1] == 0).all()


def test_a_pixel_beside_a_uv_seam_takes_its_continuous_side():
    uv, face = quad_uv(8, 4, 1)
    uv[0, 4:, :, 0] += F(0.375)  # a packed copy: u jumps by 24 texels between rows 3 and 4
    cov, level = ref.select_level(uv, face, 64, 64, 7)
    assert cov.all() and (level == 0).all()
    jump = (uv[0, 4, 0, 0] - uv[0, 3, 0, 0]) * F(64)
    assert jump * jump > 2 ** 9  # the larger of the two would have chosen level 5
    # a pixel with the seam on both sides along i has no continuous side there
    uv[0, 5:, :, 0] += F(0.375)
    assert (ref.select_level(uv, face, 64, 64, 7)[1][0, 4] == 5).all()


def test_wrap_repeat_against_clamp():
    tex = np.zeros((4, 4, 3), F)
    tex[..., 0] = np.arange(4, dtype=F)[None, :]  # a ramp along u
    tex[..., 1] = np.arange(4, dtype=F)[:, None]  # and along v
    pyr = ref.pyramid(tex, 1)
    uv = np.zeros((1, 2, 1, 3), F)
    uv[0, :, 0, 0] = [-0.25, 1.25]
    uv[0, :, 0, 1] = 0.5  # t = 1.5: halfway between rows 1 and 2
    face = np.zeros((1, 2, 1), np.int32)
    rep = ref.texture(uv, face, pyr, 4, 4, 1, ref.WRAP_REPEAT)
    cla = ref.texture(uv, face, pyr, 4, 4, 1, ref.WRAP_CLAMP)
    # u = -0.25: s = -1.5, columns -2 and -1 -> 2 and 3 (repeat), 0 and 0 (clamp); u = 1.25: s = 4.5, columns 4 and 5
    assert rep[0, :, 0, 0].tolist() == [2.5, 0.5] and cla[0, :, 0, 0].tolist() == [0.0, 3.0]
    assert rep[0, :, 0, 1].tolist() == [1.5, 1.5] and cla[0, :, 0, 1].tolist() == [1.5, 1.5]
    # v wraps the same way
    uv[..., :2] = uv[..., 1::-1].copy()
    assert ref.texture(uv, face, pyr, 4, 4, 1, ref.WRAP_REPEAT)[0, :, 0, 1].tolist() == [2.5, 0.5]
    assert ref.texture(uv, face, pyr, 4, 4, 1, ref.WRAP_CLAMP)[0, :, 0, 1].tolist() == [0.0, 3.0]
    # the paint: clamp(value * scale + bias, lo, hi)
    painted = ref.texture(uv, face, pyr, 4, 4, 1, ref.WRAP_CLAMP, scale=2.0, bias=-1.0, lo=0.0, hi=4.0)
    assert painted[0, :, 0, 1].tolist() == [0.0, 4.0]


def test_uncovered_pixels_get_the_background():
    uv, face = quad_uv(3, 4, 1)
    uv[0, 0, 0, 0] = np.nan
    uv[0, 0, 1, 1] = np.inf
    uv[0, 0, 2, 0] = 65537.0
    uv[0, 0, 3, 1] = -65536.0  # the bound itself is covered
    face[0, 1, 0] = -1
    tex = np.random.RandomState(0).rand(64, 64, 3).astype(F)
    image = ref.texture(uv, face, ref.pyramid(tex), 64, 64, 7, background=0.25)
    want = np.zeros((3, 4), bool)
    want[0, :3] = want[1, 0] = True
    assert np.array_equal((image[0] == F(0.25)).all(-1), want)
    assert np.isfinite(image).all()


@pytest.mark.parametrize("nearest", [ref.MAX_Z, ref.MIN_Z], ids=["max", "min"])
@pytest.mark.parametrize("mode", [ref.OVER, ref.DEPTH], ids=["over", "depth"])
def test_composite_truth_table(mode, nearest):
    depths = [0.5, 1.5, -0.0, np.nan]
    cases = list(itertools.product([True, False], [True, False], depths, depths))  # front covered, back covered, df, db
    n = len(cases)
    front = (np.full((n, 3), F(0.2), F), np.array([c[2] for c in cases], F), np.where([c[0] for c in cases], 7, -1))
    back = (np.full((n, 3), F(0.7), F), np.array([c[3] for c in cases], F), np.where([c[1] for c in cases], 3, -1))
    image, depth, mask = ref.composite(front, back, mode, nearest, background=0.9)
    for k, (fc, bc, df, db) in enumerate(cases):
        if mode == ref.OVER or not bc:
            shows_front = fc
        else:  # ties and NaNs go to front
            shows_front = fc and not ((db < df) if nearest == ref.MIN_Z else (db > df))
        want = 2 if shows_front else (1 if bc else 0)
        assert mask[k] == want, (k, cases[k])
        assert image[k].tolist() == [F({0: 0.9, 1: 0.7, 2: 0.2}[want])] * 3
        bits = {0: F(0.0), 1: F(db), 2: F(df)}[want].view(np.uint32)
        assert depth[k].view(np.uint32) == bits, (k, cases[k])  # the winner's 32-bit pattern: -0.0 and NaN survive
    # both modes see a tie as front, and the depth mode is exercised
    tie = cases.index((True, True, 0.5, 0.5))
    assert mask[tie] == 2
    if mode == ref.DEPTH:
        assert (mask == 1).sum() > sum(1 for c in cases if not c[0] and c[1])


MESH = {"normals": "accumulate", "colors": False}


def refused(match, pictures, mesh=MESH):
    from monoport_amd import pipeline
    with pytest.raises(ValueError, match=match):
        pipeline.FrameSlot(_net("G", 1), "cpu", mesh=mesh, pictures=pictures)


def test_the_new_option_keys_are_refused_before_any_allocation():
    from monoport_amd import pipeline, recon
    scene = object.__new__(recon.Scene)  # validation looks at the type alone
    refused("scene must be a recon.Scene", {"scene": "floor"})
    refused("scene must be a recon.Scene", {"scene": {"verts": None}})
    refused("shade=None renders none", {"scene": scene, "shade": None})
    refused("shade=None renders none", {"scene": scene}, mesh={"normals": None, "colors": False})
    for mode in ("alpha", 1, None):
        refused("composite must be", {"composite": mode})
    refused("composite must be", {"scene": scene, "composite": "under"})
    with pytest.raises(ValueError, match="scene must be a recon.Scene"):
        pipeline.ViewsSlot(_net("G", 2), "cpu", mesh={"normals": "accumulate"}, pictures={"scene": 3})
    got = pipeline._picture_options({"scene": scene, "composite": "over"}, recon.mesh_options("accumulate"))
    assert got.scene is scene and got.composite == "over" and pipeline.PICTURE_KEYS[-2:] == ("scene", "composite")
    assert pipeline._picture_options({}, recon.mesh_options("accumulate"))[-2:] == (None, "depth")


def test_the_recon_calls_refuse_without_a_device():
    from monoport_amd import ops, recon
    scene = object.__new__(recon.Scene)
    with pytest.raises(ValueError, match="scene must be a recon.Scene"):
        recon.render_scene("floor", torch.eye(4))
    with pytest.raises(ValueError, match="scene must be a recon.Scene"):
        recon.render_mesh_many_in_scene([None], None, torch.eye(4))
    with pytest.raises(ValueError, match="shade=None"):
        recon.render_mesh_many_in_scene([None], scene, torch.eye(4), shade=None)
    with pytest.raises(ValueError, match="composite must be"):
        recon.render_mesh_many_in_scene([None], scene, torch.eye(4), composite="alpha")
    with pytest.raises(ValueError, match="wrap must be"):
        recon.Scene(np.zeros((3, 3)), np.zeros((1, 3), int), np.zeros((3, 2)), np.zeros((2, 2, 3), F), wrap="mirror",
                    device="cpu")
    with pytest.raises(ValueError, match="uv must be"):
        recon.Scene(np.zeros((3, 3)), np.zeros((1, 3), int), np.zeros((2, 2)), np.zeros((2, 2, 3), F), device="cpu")
    with pytest.raises(ValueError, match="texture must be"):
        recon.Scene(np.zeros((3, 3)), np.zeros((1, 3), int), np.zeros((3, 2)), np.zeros((2, 2), F), device="cpu")
    with pytest.raises(ValueError, match="three rows per face"):
        recon.Scene.from_packed(np.zeros((4, 3)), np.zeros((4, 2)), np.zeros((2, 2, 3), F), device="cpu")
    assert ops.COMPOSITE_MODES == {"over": 0, "depth": 1} and ops.WRAP_MODES == {"repeat": 0, "clamp": 1}
