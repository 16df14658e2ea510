"""Reference fixtures of multi-view queries (SurfaceClassifier num_views = V > 1, multi-view PIFu).

Run where the reference checkout is available (CPU only):

    python tools/gen_golden_query_views.py

Like tools/gen_golden_query_ext.py it runs the REFERENCE's own modules on the seeded inputs of
monoport_amd/synthetic.py and writes only their outputs, the calibrations and the seeds to tests/golden/.  The
reference net gets a ``SurfaceClassifier(channels, V, False, last_op)`` in place of its head, loaded with the same
state dict.  Every fixture carries ``case``: a literal dict that regenerates its inputs
(tests/test_query_views_cpu.py / _gpu.py: ``case_inputs``); ``special`` holds the points that replace the first
columns of the random ones (border, z == 0), computed here from the calibrations.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import OUT, load_mlp, ref_net  # noqa: E402  (puts the reference on sys.path)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from monoport_amd import synthetic as syn  # noqa: E402
from oracle import pifu_oracle as orc  # noqa: E402

F = 2.0      # perspective focal length, in units of the half image (as gen_golden_query_ext.py)
DEPTH = 3.0  # camera -> box centre
CHANNELS = {"G": ([257, 1024, 512, 256, 128, 1], nn.Sigmoid), "C": ([513, 1024, 512, 256, 128, 3], nn.Tanh)}


def persp_calib_yaw(s, c, focal=F, depth=DEPTH):
    """[4,4] f32 K [R | t] with a yaw of (sin, cos) = (s, c) about y; (0.6, 0.8) is gen_golden_query_ext's camera."""
    r = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]], np.float64)
    k = np.diag([focal, focal, 1.0])
    m = np.eye(4)
    m[:3, :3] = k @ r
    m[:3, 3] = k @ np.array([0.0, 0.0, depth])
    return m.astype(np.float32)


def calibs_of(case):
    if case["proj"] == "orthogonal":
        return np.stack([orc.pifu_calib(*syn.scene_camera(s))[0] for s in case["steps"]])
    return np.stack([persp_calib_yaw(*sc) for sc in case["yaws"]])


def case_inputs(case, special=None):
    """case dict -> (layers, [V,C,H,W] maps, [3,N] points, [V,4,4] calibs); ``special`` replaces the first columns."""
    kind, mlp = case["kind"], case["mlp"]
    layers = syn.rand_mlp(kind, mlp[1], mlp[2]) if mlp[0] == "rand" else syn.body_mlp(kind, noise=mlp[2], seed=mlp[1])
    c = CHANNELS[kind][0][0] - 1
    mk = syn.rand_feat if case["feat"] == "rand" else syn.body_feat
    f = np.stack([mk(c, 128, 128, s) for s in case["feats"]])
    pts = case["pts"]
    if pts[0] == "lattice":  # Seg3dLossless(b_min=-1, b_max=1) final lattice (align_corners=False)
        r = pts[1]
        g = ((np.arange(r, dtype=np.float32) / np.float32(r)) + (np.float32(1.0) / np.float32(r)) / np.float32(2))
        g = g * np.float32(2.0) + np.float32(-1.0)
        zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
        p = np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)]).astype(np.float32)
    else:
        p = syn.rand_points(pts[1], pts[2], pts[3])
    if special is not None:
        p[:, :special.shape[1]] = special
    return layers, f, p, calibs_of(case)


def ref_views_net(kind, v_n, layers, projection):
    from monoport.lib.modeling.heads.SurfaceClassifier import SurfaceClassifier
    from monoport.lib.modeling import geometry
    net = ref_net(kind)
    ch, last = CHANNELS[kind]
    net.surface_classifier = SurfaceClassifier(ch, v_n, False, last()).eval()
    load_mlp(net, layers)
    net.projection = getattr(geometry, projection)
    return net


def ref_query(net, f, p, calibs):
    v_n = f.shape[0]
    feats = [[torch.zeros(v_n, f.shape[1], 2, 2)]] * 3 + [[torch.from_numpy(f)]]
    pts = torch.from_numpy(p)[None].repeat(v_n, 1, 1)
    return net.query(feats, pts, calibs=torch.from_numpy(calibs))[0].numpy()


def project(p, calibs, projection):
    from monoport.lib.modeling import geometry
    v_n = calibs.shape[0]
    fn = getattr(geometry, projection)
    return fn(torch.from_numpy(p)[None].repeat(v_n, 1, 1), torch.from_numpy(calibs)).numpy()


def border_points(calib, projection="orthogonal"):
    """Points whose view-0 projection lies just outside the image (partial taps), from the inverse calibration."""
    inv = np.linalg.inv(calib.astype(np.float64))
    xyz = [(1.004, 0.3, 0.1), (-1.003, -0.2, 0.0), (0.25, 1.002, -0.1), (-0.5, -1.005, 0.2), (1.02, 1.01, 0.0),
           (1.2, 0.1, 0.0)]
    out = []
    for x, y, z in xyz:
        if projection == "perspective":
            d = DEPTH
            out.append(inv @ np.array([x * d, y * d, d, 1.0]))
        else:
            out.append(inv @ np.array([x, y, z, 1.0]))
    return np.array(out)[:, :3].T.astype(np.float32)


def stats(name, out, xyz):
    inside = (np.abs(xyz[:, 0]) <= 1) & (np.abs(xyz[:, 1]) <= 1)  # [V,N]
    some = inside.any(0) & ~inside.all(0)
    none = ~inside.any(0)
    nan = np.isnan(out).all((0, 1))
    print("%-22s %-16s in some-not-all views %5d  in none %5d  NaN %3d  range [%.3g, %.3g]" % (
        name, out.shape, int(some.sum()), int(none.sum()), int(nan.sum()), float(np.nanmin(out)), float(np.nanmax(out))))
    return inside, some, none, nan


QUERY_CASES = {
    "query_views_G_ortho": dict(kind="G", V=3, mlp=("rand", 211, 2.0), feat="rand", feats=[221, 222, 223],
                                pts=("rand", 16384, 231, 1.2), proj="orthogonal", steps=[0, 120, 240]),
    "query_views_G_persp": dict(kind="G", V=3, mlp=("rand", 212, 2.0), feat="rand", feats=[224, 225, 226],
                                pts=("rand", 16384, 232, 1.2), proj="perspective",
                                yaws=[(0.6, 0.8), (0.0, 1.0), (-0.6, 0.8)]),
    "query_views_C_ortho": dict(kind="C", V=2, mlp=("rand", 213, 2.0), feat="rand", feats=[227, 228],
                                pts=("rand", 8192, 233, 1.2), proj="orthogonal", steps=[30, 150]),
}


@torch.no_grad()
def gen_query_views():
    for name, case in QUERY_CASES.items():
        calibs = calibs_of(case)
        special = border_points(calibs[0], case["proj"])
        if case["proj"] == "perspective":
            # exact z == 0 in view 0 (gen_golden_query_ext.py): x = 0, z = -3.75 -> 0.8f * -3.75 + 3 = 0
            zero = np.array([[0.0] * 4, [0.0, 0.5, -0.5, 0.25], [-3.75] * 4], np.float32)
            special = np.concatenate([zero, special], 1)
        layers, f, p, calibs = case_inputs(case, special)
        net = ref_views_net(case["kind"], case["V"], layers, case["proj"])
        out = ref_query(net, f, p, calibs)
        xyz = project(p, calibs, case["proj"])
        inside, some, none, nan = stats(name, out, xyz)
        assert out.shape == (case["V"], CHANNELS[case["kind"]][0][-1], p.shape[1])
        assert some.sum() > 100 and none.sum() > 100
        finite = np.isfinite(xyz[:, :2]).all((0, 1))
        assert (out[:, :, none & finite] == 0).all()
        if case["proj"] == "perspective":
            assert nan[:4].all() and not nan[4:].any() and inside[1:, :4].any()
        else:
            assert not nan.any()
        np.savez_compressed(os.path.join(OUT, name + ".npz"), out=out, calib=calibs, case=np.array([repr(case)]),
                            special=special)


FORWARD_CASE = dict(kind="G", V=3, B=2, mlp=("rand", 241, 2.0), n=4096, seed=242, scale=1.0)


def forward_inputs(case):
    """[B*V, C+1, N] f32 features of the forward fixture."""
    c = CHANNELS[case["kind"]][0][0]
    rng = np.random.default_rng(case["seed"])
    return (rng.standard_normal((case["B"] * case["V"], c, case["n"])) * case["scale"]).astype(np.float32)


@torch.no_grad()
def gen_forward_views():
    case = FORWARD_CASE
    layers = syn.rand_mlp(case["kind"], case["mlp"][1], case["mlp"][2])
    net = ref_views_net(case["kind"], case["V"], layers, "orthogonal")
    out = net.surface_classifier(torch.from_numpy(forward_inputs(case))).numpy()
    assert out.shape == (case["B"], 1, case["n"])
    print("forward_views_G_b2 %s range [%.3g, %.3g]" % (out.shape, float(out.min()), float(out.max())))
    np.savez_compressed(os.path.join(OUT, "forward_views_G_b2.npz"), out=out, case=np.array([repr(case)]))


DENSE_CASE = dict(kind="G", V=3, mlp=("body", 251, 0.05), feat="body", feats=[252, 253, 254], pts=("lattice", 65),
                  proj="orthogonal", steps=[0, 6, 12])


@torch.no_grad()
def gen_views_dense65():
    """Row 0 of the reference's multi-view netG.query on the 65^3 lattice of Seg3dLossless(b_min=-1, b_max=1)."""
    case = DENSE_CASE
    layers, f, p, calibs = case_inputs(case)
    net = ref_views_net(case["kind"], case["V"], layers, case["proj"])
    out = ref_query(net, f, p, calibs)[0, 0]
    frac = float((out > 0.5).mean())
    print("views_dense65 above 0.5: %.4f" % frac)
    assert 0.01 <= frac <= 0.60, frac  # the body fills ~3 % of the box
    r = case["pts"][1]
    np.savez_compressed(os.path.join(OUT, "views_dense65.npz"), out=out.reshape(r, r, r), calib=calibs,
                        case=np.array([repr(case)]))


if __name__ == "__main__":
    gen_query_views()
    gen_forward_views()
    gen_views_dense65()
