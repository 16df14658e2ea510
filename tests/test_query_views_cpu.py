"""Multi-view queries without a GPU: the C-ABI surface, MP_MAX_VIEWS, the fixtures' inputs and a torch-CPU restatement
of the multi-view semantics (heads/SurfaceClassifier.py:60-66, MonoPortNet.py:48-91) that reproduces the reference
fixtures (tools/gen_golden_query_views.py), and the host-side argument errors."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mp_query_views", "mp_mlp_forward_views"]


def _gpu_helpers():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_views_gpu_helpers", os.path.join(ROOT, "tests", "test_query_views_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_symbols_in_header_bindings_and_exports():
    from monoport_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "monoport_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    from monoport_amd import ops
    assert callable(ops.query_views) and callable(ops.mlp_forward_views)


def test_max_views_matches_python():
    from monoport_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "monoport_hip.h")).read()
    m = re.search(r"#define MP_MAX_VIEWS (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MAX_VIEWS == ops.MAX_VIEWS == 8


# view-0 image coordinates of the fixtures' border points (tools/gen_golden_query_views.py: border_points)
BORDER_XY = np.array([[1.004, -1.003, 0.25, -0.5, 1.02, 1.2], [0.3, -0.2, 1.002, -1.005, 1.01, 0.1]])

FIXTURES = ["query_views_G_ortho", "query_views_G_persp", "query_views_C_ortho", "views_dense65"]


@pytest.mark.parametrize("name", FIXTURES)
def test_case_regenerates_inputs(name):
    h = _gpu_helpers()
    g = load_golden(name)
    case, layers, f, p, calibs = h.case_inputs(g)
    assert np.array_equal(calibs, g["calib"])
    assert f.shape[0] == case["V"] == calibs.shape[0] and f.shape[1] == h.CHANNELS[case["kind"]][0] - 1
    n = g["out"].size // (case["V"] * h.CHANNELS[case["kind"]][-1]) if name != "views_dense65" else g["out"].size
    assert p.shape == (3, n)
    if "special" in g.files:
        # the special points are what the generator says: view 0 projects them to the intended targets -- z == 0
        # (perspective) and just outside the image border (partial taps)
        sp = np.ascontiguousarray(g["special"])
        k = 0
        xyz0 = _project(sp, calibs[0], case["proj"]).numpy()
        if case["proj"] == "perspective":
            k = 4
            z = _project(sp[:, :k], calibs[0], "orthogonal").numpy()[2]
            assert (z == 0).all() and not np.isfinite(xyz0[:2, :k]).all(0).any()
        assert np.abs(xyz0[:2, k:] - BORDER_XY[:, :sp.shape[1] - k]).max() <= 1e-5


def _project(p, calib, projection):
    c = torch.from_numpy(calib[:3])
    xyz = torch.baddbmm(c[None, :, 3:4], c[None, :, :3], torch.from_numpy(p)[None])[0]
    if projection == "perspective":
        xyz = torch.cat([xyz[:2] / xyz[2:3], xyz[2:3]], 0)
    return xyz


def cpu_views(layers, f, p, calibs, projection, last_op, sample_outside=True):
    """torch-CPU restatement: per view project, grid_sample (zero padding), layers 0-2, means, layers 3-4, masks.
    sample_outside=False: the plain single-view kernel's sampling instead (out-of-image views get zero features).
    Runs at the precision of its inputs: float64 layers, maps, points and calibrations give the float64 model."""
    v_n = f.shape[0]
    feats, masks = [], []
    for v in range(v_n):
        xyz = _project(p, calibs[v], projection)
        s = F.grid_sample(torch.from_numpy(f[v])[None], xyz[:2].T[None, :, None], align_corners=True)[0, :, :, 0]
        if not sample_outside:
            s = s * ((xyz[0] >= -1) & (xyz[0] <= 1) & (xyz[1] >= -1) & (xyz[1] <= 1)).float()[None]
        # z_scale reaches the kernels and the oracle as a float32: the same value when the inputs are float64
        feats.append(torch.cat([s, xyz[2:3] * float(np.float32(syn.Z_SCALE))], 0))
        masks.append(((xyz[0] >= -1) & (xyz[0] <= 1) & (xyz[1] >= -1) & (xyz[1] <= 1)).float())
    return mlp_views(layers, torch.stack(feats), last_op, masks)


def mlp_views(layers, feature, last_op, masks=None):
    """feature [V,C+1,N] -> [1,Cout,N], or [V,Cout,N] masked per view."""
    v_n = feature.shape[0]
    w = [(torch.from_numpy(a), torch.from_numpy(b)) for a, b in layers]
    y = feature
    for i in range(5):
        inp = y if i == 0 else torch.cat([y, tmpy if i > 2 else feature], 1)
        y = torch.einsum("oc,vcn->von", w[i][0], inp) + w[i][1][None, :, None]
        if i != 4:
            y = F.leaky_relu(y)
        if i == 2:
            y = y.view(-1, v_n, y.shape[1], y.shape[2]).mean(1)
            tmpy = feature.view(-1, v_n, feature.shape[1], feature.shape[2]).mean(1)
    if last_op != 0:  # 0: none (SurfaceClassifier(last_op=None)), 1: sigmoid, 2: tanh
        y = torch.sigmoid(y) if last_op == 1 else torch.tanh(y)
    if masks is None:
        return y
    return torch.stack([m[None] * y[0] for m in masks])


@pytest.mark.parametrize("name", ["query_views_G_ortho", "query_views_G_persp", "query_views_C_ortho"])
def test_cpu_restatement_reproduces_fixture(name):
    h = _gpu_helpers()
    g = load_golden(name)
    case, layers, f, p, calibs = h.case_inputs(g)
    m = 2048  # a prefix keeps the CPU time down; it holds every special point
    with torch.no_grad():
        out = cpu_views(layers, f, np.ascontiguousarray(p[:, :m]), calibs, case["proj"], syn.LAST_OP[case["kind"]]).numpy()
    ref = g["out"][:, :, :m]
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    assert float(np.nanmax(np.abs(out - ref))) <= 1e-5
    if case["proj"] == "perspective":
        assert np.isnan(ref[:, :, :4]).all()
    # the partial taps of the border points (just outside view 0) feed the mean: sampling them as zero, as the
    # single-view kernel does for out-of-image points, misses the fixture by far more than the bar in other views
    sp = slice(4 if case["proj"] == "perspective" else 0, g["special"].shape[1])
    with torch.no_grad():
        zeroed = cpu_views(layers, f, np.ascontiguousarray(p[:, sp]), calibs, case["proj"], syn.LAST_OP[case["kind"]],
                           sample_outside=False).numpy()
    seen = (ref[:, :, sp] != 0).any(1)  # rows of views that see the point
    assert seen[1:].any() and float(np.abs(zeroed - ref[:, :, sp])[:, :, seen.any(0)].max()) > 1e-3


def test_cpu_restatement_reproduces_forward_fixture():
    import ast
    g = load_golden("forward_views_G_b2")
    case = ast.literal_eval(str(g["case"][0]))
    rng = np.random.default_rng(case["seed"])
    feat = (rng.standard_normal((case["B"] * case["V"], 257, case["n"])) * case["scale"]).astype(np.float32)
    layers = syn.rand_mlp("G", case["mlp"][1], case["mlp"][2])
    with torch.no_grad():
        out = torch.cat([mlp_views(layers, torch.from_numpy(feat[b:b + case["V"]]), 1)
                         for b in range(0, feat.shape[0], case["V"])]).numpy()
    assert out.shape == g["out"].shape and float(np.abs(out - g["out"]).max()) <= 1e-5


def test_host_side_argument_errors():
    from monoport_amd.modeling import heads
    ch = [257, 1024, 512, 256, 128, 1]
    for bad in (0, 9):
        with pytest.raises(ValueError):
            heads.SurfaceClassifier(ch, bad, False, "sigmoid")
    head = heads.SurfaceClassifier(ch, 8, False, "sigmoid")
    assert head.num_views == 8
    for prec in ("f16x3", "f16w", "f16"):
        with pytest.raises(ValueError):
            head.set_precision(prec)
    head.set_precision("f32")
    assert heads.SurfaceClassifier(ch, 1, False, "sigmoid").set_precision("f16w").precision == "f16w"


def _multi_view_net(kind, v_n):
    from monoport_amd.modeling import PIFuNetC, PIFuNetG, heads
    net = PIFuNetG() if kind == "G" else PIFuNetC()
    ch = [257, 1024, 512, 256, 128, 1] if kind == "G" else [513, 1024, 512, 256, 128, 3]
    net.surface_classifier = heads.SurfaceClassifier(ch, v_n, False, "sigmoid" if kind == "G" else "tanh")
    return net.eval()


def test_single_view_engines_refuse_multi_view_head():
    """bind() (octree engine, colour queries) and the frame pipeline run the single-view kernels: a multi-view head
    is refused there instead of being run as a single-view MLP."""
    from monoport_amd import pipeline
    net_g = _multi_view_net("G", 3)
    with pytest.raises(NotImplementedError, match="num_views"):
        net_g.bind([[torch.zeros(3, 256, 8, 8)]], torch.eye(4)[None].expand(3, 4, 4))
    with pytest.raises(NotImplementedError, match="multi-view"):
        pipeline.FrameSlot(net_g, "cpu")
    from monoport_amd.modeling import PIFuNetG
    with pytest.raises(NotImplementedError, match="netC"):
        pipeline.FrameSlot(PIFuNetG().eval(), "cpu", netC=_multi_view_net("C", 2))


@pytest.mark.parametrize("bad", [2.5, 3.0, True, "3", None])
def test_num_views_must_be_an_integer(bad):
    from monoport_amd.modeling import heads
    with pytest.raises(ValueError):
        heads.SurfaceClassifier([257, 1024, 512, 256, 128, 1], bad, False, "sigmoid")
