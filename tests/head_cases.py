"""Inputs and float64 references for the tests of every head the f32 query kernels admit
(tests/test_query_heads_cpu.py, tests/test_query_heads_gpu.py): C in {256, 512} x Cout in {1, 3} x last_op in
{none, sigmoid, tanh}.  numpy / torch-CPU only; every reference is computed once per process and shared.

One scene per C: a 16 x 24 feature map (384 texels = 6 x 64, so a skip table is admitted), 257 points (4 tiles of
64 + 1, 8 tiles of 32 + 1) in [-1.1, 1.1]^3 of which the first four sit on the image corners, and an orbit-camera
calibration.  The multi-view scenes add maps and calibrations for the further views; view 0 is the single-view scene.
"""
import functools
import math

import numpy as np

from monoport_amd import synthetic as syn
from oracle import pifu_oracle as orc

CS = (256, 512)
COUTS = (1, 3)
LAST_OPS = (0, 1, 2)  # none / sigmoid / tanh (include/monoport_hip.h)
PAIRS = [(c, cout) for c in CS for cout in COUTS]
HEADS = [(c, cout, op) for c, cout in PAIRS for op in LAST_OPS]
HIDDEN = [1024, 512, 256, 128]  # SurfaceClassifier.py:76 / :84

H, W, N = 16, 24, 257
EXTENT = 1.1
MAX_V = 3
# uniform(+-GAIN / sqrt(fan_in)) weights: chosen (tests/test_query_heads_cpu.py asserts it) so that more than half of
# the logits lie inside (-2, 2), none beyond +-20 (measured: 84-97 % inside, the largest 2.7-4.1), and the oracle's own
# float32 evaluation of a linear head stays within 1e-4 of float64 (measured: 3.6e-6 .. 9.5e-6)
GAIN = 2.5
FEAT_SEED = {256: 910, 512: 920}     # + view
POINT_SEED = {256: 930, 512: 931}
# orbit step and yaw (degrees) of views 0, 1, 2; the yaw differs too, because the y row of the calibration depends on
# the yaw alone and view 0's corner points would sit on the border of every view
CAMERA = {256: ((25, 20.0), (140, 35.0), (250, 10.0)), 512: ((40, 20.0), (155, 8.0), (290, 31.0))}
HEAD_SEED = {(256, 1): 940, (256, 3): 941, (512, 1): 942, (512, 3): 943}
CORNERS = ((-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0))


def head_id(head):
    return "C%d-Cout%d-%s" % (head[0], head[1], ("none", "sigmoid", "tanh")[head[2]]) if len(head) == 3 \
        else "C%d-Cout%d" % head


def head_dims(c, cout):
    return [c + 1] + HIDDEN + [cout]


def head_layers(c, cout, seed, gain):
    """[(W[out,in] f32, b[out] f32)] with the skip-concat widths of syn.layer_shapes for any admitted (c, cout),
    drawn as syn.rand_mlp draws them: uniform(+-gain / sqrt(fan_in)), weight then bias, layer by layer."""
    d = head_dims(c, cout)
    rs = np.random.RandomState(seed)
    layers = []
    for l in range(len(d) - 1):
        out_c, in_c = d[l + 1], d[l] + (d[0] if l > 0 else 0)
        bound = gain / math.sqrt(in_c)
        w = rs.uniform(-bound, bound, size=(out_c, in_c)).astype(np.float32)
        b = rs.uniform(-bound, bound, size=(out_c,)).astype(np.float32)
        layers.append((w, b))
    return layers


@functools.lru_cache(maxsize=None)
def layers_of(c, cout):
    return head_layers(c, cout, HEAD_SEED[(c, cout)], GAIN)


def layers64(layers):
    return [(w.astype(np.float64), b.astype(np.float64)) for w, b in layers]


def project64(p, calib):
    """Rows 0-2 of calib applied to [3,N] points in float64 (the op order of the oracle's project_row)."""
    c = np.asarray(calib, np.float64)
    p = np.asarray(p, np.float64)
    return np.stack([c[k, 3] + (c[k, 2] * p[2] + (c[k, 1] * p[1] + c[k, 0] * p[0])) for k in range(3)])


def corner_points(calib, reach=(8, 40, 40), margin=1e-12):
    """[3,4] f32 world points that the kernel's own float32 projection (oracle.orthogonal, the same FMA chain) puts
    EXACTLY on the four image corners (+-1, +-1) while their exact projection lies inside the image by more than
    ``margin``: the float32 kernel takes its border path (last texel, the taps past it weigh 0) and no float64
    reference disagrees about the in-image mask.  Found by a search over neighbouring floats of the float64
    solution; the candidate nearest to it wins."""
    inv = np.linalg.inv(np.asarray(calib, np.float64))
    offs = np.stack(np.meshgrid(*[np.arange(-r, r + 1) for r in reach], indexing="ij"), -1).reshape(-1, 3)
    offs = offs[np.argsort(np.abs(offs).sum(1), kind="stable")]
    out = np.empty((3, 4), np.float32)
    for k, (sx, sy) in enumerate(CORNERS):
        base = (inv @ np.array([sx, sy, 0.0, 1.0]))[:3].astype(np.float32)
        cand = (base.view(np.int32)[None, :] + offs.astype(np.int32)).view(np.float32)  # neighbouring floats
        cand = np.ascontiguousarray(cand.T)
        x32 = orc.orthogonal(cand, calib, "f32")
        x64 = project64(cand, calib)
        ok = ((x32[0] == np.float32(sx)) & (x32[1] == np.float32(sy))
              & (np.abs(x64[0]) <= 1 - margin) & (np.abs(x64[1]) <= 1 - margin))
        if not ok.any():
            raise AssertionError("no float near corner %s projects onto it" % ((sx, sy),))
        out[:, k] = cand[:, int(np.argmax(ok))]
    return out


@functools.lru_cache(maxsize=None)
def scene_views(c):
    """(f [MAX_V,C,H,W], p [3,N], calibs [MAX_V,4,4]) -- view 0 is the single-view scene of this C."""
    f = np.stack([syn.rand_feat(c, H, W, FEAT_SEED[c] + v) for v in range(MAX_V)])
    calibs = np.stack([orc.pifu_calib(*syn.scene_camera(s, yaw))[0] for s, yaw in CAMERA[c]])
    p = syn.rand_points(N, POINT_SEED[c], EXTENT)
    p[:, :4] = corner_points(calibs[0])
    for a in (f, p, calibs):
        a.setflags(write=False)
    return f, p, calibs


def scene(c, view=0):
    """(f [C,H,W], p [3,N], calib [4,4]) of one view."""
    f, p, calibs = scene_views(c)
    return f[view], p, calibs[view]


@functools.lru_cache(maxsize=None)
def in_image(c, view=0, precision="f32"):
    """bool [N]: the kernel's mask (float32 projection) or the float64 one."""
    _, p, calib = scene(c, view)
    xyz = orc.orthogonal(p, calib, "f32") if precision == "f32" else project64(p, calib)
    return (np.abs(xyz[0]) <= 1) & (np.abs(xyz[1]) <= 1)


@functools.lru_cache(maxsize=None)
def ref_query(c, cout, last_op, precision, view=0):
    """oracle.query on the scene: [Cout,N] f32."""
    f, p, calib = scene(c, view)
    out = orc.query(f, p, calib, layers_of(c, cout), last_op, syn.Z_SCALE, precision=precision)
    out.setflags(write=False)
    return out


def y32(c, cout, last_op):
    """The yardstick: what the oracle's own float32 evaluation loses against float64 on this case."""
    return float(np.abs(ref_query(c, cout, last_op, "f32").astype(np.float64) - ref_query(c, cout, last_op, "f64")).max())


def y0(c):
    """The yardstick of the linear heads of this C: the largest y32 over its last_op = none cases."""
    return max(y32(c, cout, 0) for cout in COUTS)


# ---- the direct (explicit-feature) form ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct_features(c, view=0):
    """[C+1,N] f32: what the fused kernel feeds its MLP on the scene -- the float32 samples and z_feat."""
    f, p, calib = scene(c, view)
    xyz = orc.orthogonal(p, calib, "f32")
    x = np.concatenate([orc.sample(f, xyz[:2], "f32"), (xyz[2:3] * np.float32(syn.Z_SCALE)).astype(np.float32)], 0)
    x.setflags(write=False)
    return x


def mlp_numpy(layers, x, last_op, dtype=np.float64):
    """SurfaceClassifier.py:47-69 in numpy at ``dtype`` for any (c, cout, last_op): x [C+1,N] -> [Cout,N]."""
    x = np.asarray(x, dtype)
    y = x
    for i, (w, b) in enumerate(layers):
        inp = y if i == 0 else np.concatenate([y, x], 0)  # SurfaceClassifier.py:55
        y = w.astype(dtype) @ inp + b.astype(dtype)[:, None]
        if i != len(layers) - 1:
            y = np.where(y > 0, y, dtype(0.01) * y)
    if last_op == 1:
        y = 1 / (1 + np.exp(-y))
    elif last_op == 2:
        y = np.tanh(y)
    return y


@functools.lru_cache(maxsize=None)
def ref_direct(c, cout, last_op, precision="f64"):
    out = mlp_numpy(layers_of(c, cout), direct_features(c), last_op, np.float64 if precision == "f64" else np.float32)
    out.setflags(write=False)
    return out


def y0_direct(c):
    return max(float(np.abs(ref_direct(c, cout, 0, "f32") - ref_direct(c, cout, 0, "f64")).max()) for cout in COUTS)


# ---- multi-view references (the torch-CPU restatement of tests/test_query_views_cpu.py) ----------------------------
@functools.lru_cache(maxsize=None)
def ref_views(c, cout, last_op, v_n, precision="f64"):
    """cpu_views on the first v_n views: [V,Cout,N] at float64, or at float32 (the yardstick's evaluation)."""
    import torch
    from test_query_views_cpu import cpu_views
    f, p, calibs = scene_views(c)
    layers = layers_of(c, cout)
    if precision == "f64":
        f, p, calibs, layers = f.astype(np.float64), p.astype(np.float64), calibs.astype(np.float64), layers64(layers)
    with torch.no_grad():
        out = cpu_views(layers, f[:v_n].copy(), p.copy(), calibs[:v_n].copy(), "orthogonal", last_op).numpy()
    out.setflags(write=False)
    return out


def y32_views(c, cout, last_op, v_n):
    return float(np.abs(ref_views(c, cout, last_op, v_n, "f32") - ref_views(c, cout, last_op, v_n, "f64")).max())


def y0_views(c, v_n):
    return max(y32_views(c, cout, 0, v_n) for cout in COUTS)


@functools.lru_cache(maxsize=None)
def ref_direct_views(c, cout, last_op, v_n, precision="f64"):
    """mlp_views on the direct features of the first v_n views: [1,Cout,N]."""
    import torch
    from test_query_views_cpu import mlp_views
    x = np.stack([direct_features(c, v) for v in range(v_n)])
    layers = layers_of(c, cout)
    if precision == "f64":
        x, layers = x.astype(np.float64), layers64(layers)
    with torch.no_grad():
        out = mlp_views(layers, torch.from_numpy(x), last_op).numpy()
    out.setflags(write=False)
    return out


def y0_direct_views(c, v_n):
    return max(float(np.abs(ref_direct_views(c, cout, 0, v_n, "f32") - ref_direct_views(c, cout, 0, v_n, "f64")).max())
               for cout in COUTS)


# ---- the octree scene of the (512, 1, sigmoid) head ------------------------------------------------------------
def body_layers(c, k=40.0, cc=2.0, noise=0.05, seed=0):
    """syn.body_mlp's analytic weights for a (c, 1) head: channel 0 = front depth, channel 1 = back depth, z_feat the
    LAST input (index c); sigmoid(cc - k (z - z_front)+ - k (z_back - z)+) > 0.5 strictly inside the body."""
    d = head_dims(c, 1)
    rs = np.random.RandomState(seed)
    layers = []
    for l in range(len(d) - 1):
        out_c, in_c = d[l + 1], d[l] + (d[0] if l > 0 else 0)
        bound = noise / math.sqrt(in_c)
        w = rs.uniform(-bound, bound, size=(out_c, in_c)).astype(np.float32)
        b = rs.uniform(-bound, bound, size=(out_c,)).astype(np.float32)
        if l == 0:
            w[0:2, :] = 0
            w[0, 0], w[0, c] = -k, k / syn.Z_SCALE
            w[1, 1], w[1, c] = k, -k / syn.Z_SCALE
            b[0:2] = 0
        elif l < len(d) - 2:
            w[0:2, :] = 0
            w[0, 0] = w[1, 1] = 1.0
            b[0:2] = 0
        else:
            w[0, 0] -= 1.0
            w[0, 1] -= 1.0
            b[0] += cc
        layers.append((w, b))
    return layers


def body_scene(c):
    """The scene's map with the body's depth planes in channels 0 / 1 (syn.body_feat), and its calibration."""
    f, _, calib = scene(c)
    f = f.copy()
    f[0:2] = syn.body_feature_planes(H, W)
    return f, calib
