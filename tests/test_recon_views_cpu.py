"""The multi-view fused reconstruction's surface without a GPU: mp_recon_views is exported and declared with the
agreed signature, the Python entry points exist, and Seg3dLossless refuses bad ``fuse_views`` / ``view``
arguments at construction."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the declaration of the C-ABI entry point, token for token (whitespace and comments aside)
DECLARATION = """
int mp_recon_views(mp_ctx *ctx, int mlp, int n_views, const float *const *feat_hwc, int c, int h, int w,
                   const float *const *calib, int projection, float z_scale,
                   const float *b_min, const float *b_max, const int *resolutions, int n_levels,
                   float balance, int final_level, int view, float *volume, int32_t *status,
                   const mp_recon_early *early, mp_stream stream);
"""


def _tokens(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"[A-Za-z_0-9]+|[^\sA-Za-z_0-9]", text)


def test_header_declares_mp_recon_views():
    text = open(os.path.join(ROOT, "include", "monoport_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mp_recon_views\s*\([^;]*;", text)
    assert m, "include/monoport_hip.h does not declare mp_recon_views"
    assert _tokens(m.group(0)) == _tokens(DECLARATION)


def test_library_exports_mp_recon_views():
    from monoport_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert hasattr(lib, "mp_recon_views")
    restype, argtypes = _lib.SIGNATURES["mp_recon_views"]
    assert restype is _lib.c_int and len(argtypes) == 21
    assert lib.mp_recon_views(*([None] + [0] * 2 + [None] + [0] * 3 + [None, 0, 0.0] + [None] * 3
                                + [0, 0.0, 0, 0] + [None] * 4)) == _lib.load().mp_query(
        None, 0, None, 0, 0, 0, None, 0, 0, 0, None, 0.0, None, None)  # both MP_ERR_ARG for a null context


def test_python_entry_points_exist():
    from monoport_amd import ops
    import importlib
    mpn = importlib.import_module("monoport_amd.modeling.MonoPortNet")
    sig = inspect.signature(ops.recon_views)
    assert list(sig.parameters) == ["mlp", "maps", "calibs", "projection", "z_scale", "b_min", "b_max", "resolutions",
                                    "balance", "final_level", "view", "early", "expect_level0"]
    assert sig.parameters["final_level"].default == "dilate3" and sig.parameters["view"].default == 0
    assert callable(mpn.MonoPortNet.bind_views) and inspect.isclass(mpn.ViewsBinding)
    assert "views" in inspect.signature(mpn.record_query.__init__).parameters
    assert inspect.signature(mpn.record_query.__init__).parameters["views"].default is False


def _engine(**kw):
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    return Seg3dLossless(query_func=lambda **_: None, b_min=np.array([[-1.0, -1, -1]]),
                         b_max=np.array([[1.0, 1, 1]]), resolutions=[17, 33, 65], balance_value=0.5, **kw)


def test_constructor_argument_errors():
    import warnings
    with pytest.raises(NotImplementedError, match="fuse_views"):
        _engine(faster=False, fuse_views=True)
    with pytest.raises(ValueError, match="view"):
        _engine(faster=True, fuse_views=True, view=-1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a known argument: no "ignoring unknown arguments" warning
        eng = _engine(faster=True, fuse_views=True, view=2)
        assert eng.fuse_views is True and eng.view == 2
        eng = _engine(faster=True)
        assert eng.fuse_views is False and eng.view == 0


def test_bind_views_refuses_single_view_heads():
    from monoport_amd.modeling import PIFuNetG
    net = PIFuNetG().eval()
    with pytest.raises(NotImplementedError, match="num_views"):
        net.bind_views([[None]], None)
