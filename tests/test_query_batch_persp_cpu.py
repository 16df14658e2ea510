"""The projection-mode / batched-query surface of the C-ABI and the perspective fixtures, without a GPU."""
import ast
import os
import re

import numpy as np
import torch

from conftest import ROOT, load_golden

NEW_SYMBOLS = ["mp_perspective", "mp_query_batch", "mp_query_counted_batch_proj", "mp_recon_batch_proj"]
QUERY_GOLDENS = ["query_G_persp", "query_G_persp_body", "query_C_persp"]


def _header():
    return open(os.path.join(ROOT, "include", "monoport_hip.h")).read()


def test_new_symbols_in_header_and_binding_table():
    from monoport_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name


def test_projection_enum_matches_python():
    from monoport_amd import _lib, ops
    text = _header()
    vals = {k: int(v) for k, v in re.findall(r"\b(MP_PROJ_[A-Z]+)\s*=\s*(\d+)", text)}
    assert vals == {"MP_PROJ_ORTHOGONAL": _lib.PROJ_ORTHOGONAL, "MP_PROJ_PERSPECTIVE": _lib.PROJ_PERSPECTIVE}
    assert ops.PROJECTIONS == {"orthogonal": vals["MP_PROJ_ORTHOGONAL"], "perspective": vals["MP_PROJ_PERSPECTIVE"]}


def _perspective_np(p, calib):
    """float64 restatement of geometry.perspective (only used for which points are finite / in the image)."""
    c = calib[0].astype(np.float64)
    h = c[:3, :3] @ p.astype(np.float64) + c[:3, 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.concatenate([h[:2] / h[2:3], h[2:3]], 0)


def test_perspective_fixture_self_consistent():
    g = load_golden("perspective")
    out, z = g["out"], g["out"][2]
    assert ((z == 0) == ~np.isfinite(out[:2]).all(0)).all()  # non-finite x / y exactly where z == 0
    assert (z == 0).sum() >= 8 and (z < 0).sum() >= 50
    ref = _perspective_np(g["points"], g["calib"])
    fin = np.isfinite(out[:2]).all(0) & (np.abs(z) > 1e-3)
    assert np.abs(out[:, fin] - ref[:, fin]).max() <= 1e-4 * np.abs(ref[:, fin]).max()


def test_query_fixtures_nan_and_zero_rows():
    for name in QUERY_GOLDENS:
        g = load_golden(name)
        out = g["out"]
        case = ast.literal_eval(str(g["case"][0]))
        from monoport_amd import synthetic as syn
        p = syn.rand_points(*case["pts"][1:])
        p[:, :4] = g["special"]
        xyz = _perspective_np(p, g["calib"])
        r = g["calib"][0, 2].astype(np.float32)  # z_cam in float32 (the rows' op order: exact zeros stay zeros)
        finite = (r[3] + (r[2] * p[2] + (r[1] * p[1] + r[0] * p[0]))) != 0
        assert (~finite).sum() == 4
        # NaN rows only (and exactly) where the projection is non-finite, all channels at once
        assert np.array_equal(np.isnan(out).any(0), ~finite) and np.array_equal(np.isnan(out).all(0), ~finite), name
        # exact zeros in every channel only out of the image (margin: float64 vs the reference's float32 rows)
        margin = np.minimum(1 - np.abs(xyz[0]), 1 - np.abs(xyz[1]))
        zero = (out == 0).all(0)
        if case["mlp"][0] == "rand":
            assert not zero[finite & (margin > 1e-5)].any(), name
        assert zero[finite & (margin < -1e-5)].all(), name


def test_b3_and_dense_fixtures():
    g = load_golden("query_G_b3")
    assert g["out"].shape == (3, 1, 12288) and g["calib"].shape[0] == 3
    assert not np.array_equal(g["out"][0], g["out"][1])
    d = load_golden("persp_dense65")
    assert d["out"].shape == (65, 65, 65) and 0.05 <= (d["out"] > 0.5).mean() <= 0.6


def test_geometry_perspective_cpu_matches_reference():
    from monoport_amd.modeling import geometry
    g = load_golden("perspective")
    out = geometry.perspective(torch.from_numpy(g["points"])[None], torch.from_numpy(g["calib"]))[0].numpy()
    np.testing.assert_array_equal(out, g["out"])
