"""Non-square feature maps: the case table and input builders shared by oracle/gen_golden.py (gen_rect), by
tests/test_rect_maps_cpu.py and by tests/test_rect_maps_gpu.py.  Every kernel that samples a map takes its height
and width as two arguments; on a square map an exchanged pair is invisible.  numpy only.

The fixture tests/golden/rect_maps.npz holds what the REFERENCE's geometry.index and PIFuNetG / PIFuNetC.query
return for these inputs (outputs and calibrations only); the inputs are regenerated here from the seeds."""
import numpy as np

from monoport_amd import synthetic as syn

FIXTURE = "rect_maps"
# name -> (H, W).  wide / tall: 3840 texels = 60 skip-table tiles of 64.  thin: 192 texels = 3 tiles, every sample
# blends both rows (columns).  line: 64 texels = 1 tile, (W - 1) = 0 (or H - 1): the second tap is always invalid.
SHAPES = {
    "wide": (48, 80), "tall": (80, 48),
    "thin_w": (2, 96), "thin_h": (96, 2),
    "line_w": (1, 64), "line_h": (64, 1),
}
# the sizes on which oracle.sample(f32) is held to torch's grid_sample
SAMPLER_SIZES = [(40, 24), (24, 40), (16, 12), (12, 16), (32, 64), (64, 32), (1, 64), (64, 1), (2, 96), (96, 2), (7, 5)]

N_POINTS = 4096
N_BORDER = 8     # points 0-7: the four corners and the four edge midpoints of the image
N_CENTRES = 64   # points 8-71: texel centres
EXTENT = 1.1
N_UV = 64
MIN_INSIDE, MIN_OUTSIDE = 2000, 200  # per query case, asserted by the tests

# geometry.index: name -> (shape, feature seed, uv seed); C = 256
INDEX_CASES = {
    "index_" + shape: (shape, 600 + i, 620 + i) for i, shape in enumerate(SHAPES)
}
# PIFuNetG / PIFuNetC.query: name -> kind, shape, head seed, feature seed, point seed, camera
# ("scene": scene_camera(40); "eye": identity, under which the border and centre points land where they are meant
# to; "persp": the K [R | t] camera of tools/gen_golden_query_ext.py)
QUERY_CASES = {
    "G_wide_scene": dict(kind="G", shape="wide", mlp=641, feat=651, pts=661, camera="scene"),
    "G_tall_eye": dict(kind="G", shape="tall", mlp=642, feat=652, pts=662, camera="eye"),
    "G_thin_scene": dict(kind="G", shape="thin_w", mlp=643, feat=653, pts=663, camera="scene"),
    "G_line_eye": dict(kind="G", shape="line_h", mlp=644, feat=654, pts=664, camera="eye"),
    "C_tall_scene": dict(kind="C", shape="tall", mlp=645, feat=655, pts=665, camera="scene"),
    "C_wide_eye": dict(kind="C", shape="wide", mlp=646, feat=656, pts=666, camera="eye"),
    "G_wide_persp": dict(kind="G", shape="wide", mlp=647, feat=657, pts=667, camera="persp"),
}
# the other orientation of the thin and line maps: no fixture, held to the oracle only
ORACLE_ONLY_CASES = {
    "G_thin_h_eye": dict(kind="G", shape="thin_h", mlp=648, feat=658, pts=668, camera="eye"),
    "G_line_w_scene": dict(kind="G", shape="line_w", mlp=649, feat=659, pts=669, camera="scene"),
}
ALL_QUERY_CASES = {**QUERY_CASES, **ORACLE_ONLY_CASES}
SCENE_STEP = 40
# points 72-75 of the perspective case: z_cam == 0 exactly (0.8f * -3.75 + 3), NaN rows in the reference
PERSP_SPECIAL = np.array([[0.0] * 4, [0.0, 0.5, -0.5, 0.25], [-3.75] * 4], np.float32)
PERSP_AT = N_BORDER + N_CENTRES

# the fused reconstruction on non-square maps: body_feat(256, H, W, 2), body_mlp("G", noise=0.05, seed=1),
# scene_camera(30); per-level counts of oracle.seg3d_lossless driven by oracle.query(f32)
RECON_RES = [9, 17, 33, 65]
RECON_STEP = 30
RECON_COUNTS = {"wide": [729, 2515, 6443, 11840], "tall": [729, 2732, 6354, 11544]}


def index_inputs(name):
    """-> ([256,H,W] map, [2,64] uv in +-1.1 with the exact corners first)."""
    shape, feat_seed, uv_seed = INDEX_CASES[name]
    h, w = SHAPES[shape]
    uv = np.random.RandomState(uv_seed).uniform(-EXTENT, EXTENT, size=(2, N_UV)).astype(np.float32)
    uv[:, :4] = np.array([[-1, 1, -1, 1], [-1, -1, 1, 1]], np.float32)
    return syn.rand_feat(256, h, w, feat_seed), uv


def rect_points(h, w, seed):
    """[3,4096] f32: rand_points(4096, seed, 1.1) with points 0-7 on the corners and edge midpoints of the image and
    points 8-71 on texel centres x = -1 + 2j/(W-1), y = -1 + 2i/(H-1) (a degenerate axis keeps its random value)."""
    p = syn.rand_points(N_POINTS, seed, EXTENT)
    p[:2, :N_BORDER] = np.array([[-1, 1, -1, 1, 0, 0, -1, 1], [-1, -1, 1, 1, -1, 1, 0, 0]], np.float32)
    rs = np.random.RandomState(seed + 1000)
    i, j = rs.randint(0, h, N_CENTRES), rs.randint(0, w, N_CENTRES)
    sl = slice(N_BORDER, N_BORDER + N_CENTRES)
    if w > 1:
        p[0, sl] = (-1.0 + 2.0 * j / (w - 1)).astype(np.float32)
    if h > 1:
        p[1, sl] = (-1.0 + 2.0 * i / (h - 1)).astype(np.float32)
    return p


def persp_calib(focal=3.0, depth=3.0):
    """[1,4,4] f32, rows 0-2 = K [R | t]: the camera of tools/gen_golden_query_ext.py (yaw (sin, cos) = (0.6, 0.8)) with
    the focal length 3 instead of 2: at 2 only 63 of the 4096 points in +-1.1 leave the image, at 3 1098 do."""
    r = np.array([[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]], np.float64)
    k = np.diag([focal, focal, 1.0])
    m = np.eye(4)
    m[:3, :3] = k @ r
    m[:3, 3] = k @ np.array([0.0, 0.0, depth])
    return m.astype(np.float32)[None]


def case_camera(name):
    """-> [1,4,4] f32 calibration of a query case, built without the reference (the fixture stores the reference's)."""
    from oracle import pifu_oracle as orc
    camera = ALL_QUERY_CASES[name]["camera"]
    if camera == "scene":
        return orc.pifu_calib(*syn.scene_camera(SCENE_STEP))
    return persp_calib() if camera == "persp" else np.eye(4, dtype=np.float32)[None]


def query_inputs(name):
    """-> (kind, layers, [C,H,W] map, [3,4096] points)."""
    case = ALL_QUERY_CASES[name]
    kind = case["kind"]
    h, w = SHAPES[case["shape"]]
    p = rect_points(h, w, case["pts"])
    if case["camera"] == "persp":
        p[:, PERSP_AT:PERSP_AT + 4] = PERSP_SPECIAL
    return kind, syn.rand_mlp(kind, case["mlp"], 2.0), syn.rand_feat(syn.MLP_DIMS[kind][0] - 1, h, w, case["feat"]), p


def three_output_head(layers, seed=5):
    """A netG head whose last layer has 3 outputs (the C = 256, Cout = 3 instantiations), as
    tests/test_query_gpu.py: test_small_tile_kernel_is_bit_identical builds it.  Run it with tanh (last_op 2)."""
    rs = np.random.RandomState(seed)
    w4 = layers[-1][0]
    return layers[:-1] + [(rs.uniform(-0.1, 0.1, (3, w4.shape[1])).astype(np.float32),
                           rs.uniform(-0.1, 0.1, (3,)).astype(np.float32))]


def project(oracle, p, calib, camera):
    """Image-space [3,N] f32 of the points: the reference's orthogonal, or its perspective (the same affine map, then
    x / z and y / z in f32)."""
    xyz = oracle.orthogonal(p, calib)
    if camera == "persp":
        with np.errstate(divide="ignore", invalid="ignore"):
            xyz = np.stack([xyz[0] / xyz[2], xyz[1] / xyz[2], xyz[2]]).astype(np.float32)
    return xyz


def outside_image(xyz):
    """Points clearly off the image (finite coordinates): the reference's mask makes them exactly 0."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(xyz[:2]).all(0) & (np.minimum(1 - np.abs(xyz[0]), 1 - np.abs(xyz[1])) < -1e-6)


def inside_image(xyz):
    with np.errstate(invalid="ignore"):
        return np.isfinite(xyz[:2]).all(0) & (np.abs(xyz[0]) <= 1) & (np.abs(xyz[1]) <= 1)


def swapped_maps(f):
    """What an exchanged (h, w) makes of a [C,H,W] map: the transposed map, and the same channels-last buffer read
    with the other row length."""
    c, h, w = f.shape
    reread = np.ascontiguousarray(f.transpose(1, 2, 0)).reshape(w, h, c).transpose(2, 0, 1)
    return {"transposed": np.ascontiguousarray(f.transpose(0, 2, 1)), "reread": np.ascontiguousarray(reread)}


def oracle_query(oracle, name, f, p, calib, layers, precision, last_op=None):
    """oracle.query of a case.  The oracle projects orthogonally: a perspective case hands it the image-space
    points (the reference's affine map and divisions, bit for bit) under the identity, which is exact; the rows of
    points on z_cam == 0 mean nothing then (the reference has NaN there)."""
    case = ALL_QUERY_CASES[name]
    if last_op is None:
        last_op = syn.LAST_OP[case["kind"]]
    if case["camera"] != "persp":
        return oracle.query(f, p, calib, layers, last_op, syn.Z_SCALE, precision=precision)
    xyz = project(oracle, p, calib, "persp")
    return oracle.query(f, xyz, np.eye(4, dtype=np.float32), layers, last_op, syn.Z_SCALE, precision=precision)


def recon_inputs(shape):
    """-> (layers, [256,H,W] body map) of the reconstruction cases; the camera is scene_camera(RECON_STEP)."""
    h, w = SHAPES[shape]
    return syn.body_mlp("G", noise=0.05, seed=1), syn.body_feat(256, h, w, 2)
