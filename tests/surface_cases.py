"""Adversarial volumes for marching cubes (csrc/mcubes.hip) and forward_vertices (csrc/vertices.hip), seeded, no GPU.

The smooth blobs, spheres and reconstructed bodies of the other tests reach 116 of the 256 marching-cubes cases, no
hit of forward_vertices within two voxels of a face of the box, no plateau and no value exactly at the threshold.
The volumes here hold every case, hits at every border and in every scan segment, ties and non-finite entries.
oracle/gen_golden.py builds the same volumes from the same seeds (tests/golden/forward_vertices_edges.npz holds
the reference's results only), tests/test_surface_cases_cpu.py asserts what they contain."""
import numpy as np

KINDS = ("smooth", "binary", "quant")
DIRECTIONS = ("front", "back", "left", "right")
DEPTH_SEED = 7          # depth_volume(r, DEPTH_SEED + r, kind)
NONFINITE = (20, 91)    # nonfinite_volume(r, seed)
NOISE = {13: 13, 17: 17}  # noise_volume(r, NOISE[r]): all 256 cases each
QUARTERS = (17, 5)
ONE_CELL_SEED = 1


def depth_volume(r, seed, kind="smooth"):
    """(vol [z,y,x] f32, depth [x,y]): column (x, y) of the front view s[x, y, z'] stays <= 0.5 below depth[x, y],
    is > 0.5 at it (depth == r: no hit) and arbitrary behind it.  Row x = 0 and column y = 1 hit within the first
    four voxels (the three ``max(. - 2, 0)`` clamps run), row x = 5 hits in the last voxel only.
    smooth: [0, 0.5) below, [0, 1) behind, the hit in [0.5, 1]; binary: 0 below, {0, 1} behind, hit 1 (plateaus and
    zero-length normals); quant: {0, .25, .5} below (0.5 itself is no hit), quarters behind, hit 1."""
    rs = np.random.RandomState(seed)
    d = rs.randint(0, r + 1, size=(r, r))
    d[0, :] = rs.randint(0, 4, size=r)
    d[:, 1] = rs.randint(0, 4, size=r)
    d[5, :] = r - 1
    zp = np.arange(r)[None, None, :]
    if kind == "binary":
        below = np.zeros((r, r, r), np.float32)
        above = (rs.rand(r, r, r) > 0.3).astype(np.float32)
    elif kind == "quant":
        below = (rs.randint(0, 3, size=(r, r, r)) / 4.0).astype(np.float32)
        above = (rs.randint(0, 5, size=(r, r, r)) / 4.0).astype(np.float32)
    elif kind == "smooth":
        below = (rs.rand(r, r, r) * 0.5).astype(np.float32)
        above = rs.rand(r, r, r).astype(np.float32)
    else:
        raise ValueError(kind)
    s = np.where(zp < d[:, :, None], below, above).astype(np.float32)
    hit = (0.5 + 0.5 * rs.rand(r, r)).astype(np.float32) if kind == "smooth" else np.ones((r, r), np.float32)
    hit = np.maximum(hit, np.nextafter(np.float32(0.5), np.float32(1)))  # strictly above the threshold
    xs, ys = np.nonzero(d < r)
    s[xs, ys, d[xs, ys]] = hit[xs, ys]
    vol = np.ascontiguousarray(s.transpose(2, 1, 0)[::-1])  # s = vol[::-1].transpose(2, 1, 0)
    return vol, d


def depth_case(r, kind):
    return depth_volume(r, DEPTH_SEED + r, kind)


def noise_volume(r, seed):
    return np.random.RandomState(seed).rand(r, r, r).astype(np.float32)


def quarters_volume(r, seed):
    return (np.random.RandomState(seed).randint(0, 5, size=(r, r, r)) / 4.0).astype(np.float32)


def one_cell_volumes(seed=ONE_CELL_SEED):
    """[256,2,2,2] f32: volume c is the single cell of corner case c (bit i = corner dx + 2 dy + 4 dz, [dz,dy,dx]);
    inside values in (0.5, 1], outside values in [0, 0.5)."""
    rs = np.random.RandomState(seed)
    out = np.empty((256, 2, 2, 2), np.float32)
    for case in range(256):
        ins = np.array([(case >> i) & 1 for i in range(8)], bool).reshape(2, 2, 2)
        hi = (1.0 - 0.49 * rs.rand(2, 2, 2)).astype(np.float32)
        lo = (0.49 * rs.rand(2, 2, 2)).astype(np.float32)
        out[case] = np.where(ins, hi, lo)
    return out


def nonfinite_volume(r, seed):
    """0.8 * rand with 100 NaN, 100 +inf and 100 -inf entries (fewer where positions repeat)."""
    rs = np.random.RandomState(seed)
    vol = (rs.rand(r, r, r) * 0.8).astype(np.float32)
    idx = rs.randint(0, r, size=(300, 3))
    for k, val in enumerate((np.nan, np.inf, -np.inf)):
        i = idx[100 * k:100 * (k + 1)]
        vol[i[:, 0], i[:, 1], i[:, 2]] = val
    return vol


def corner_cases(vol, level=0.5):
    """Marching-cubes case of every cell: [r-1,r-1,r-1] int32, bit i = corner dx + 2 dy + 4 dz above the level."""
    r = vol.shape[0]
    inside = vol > np.float32(level)
    case = np.zeros((r - 1,) * 3, np.int32)
    for i in range(8):
        dx, dy, dz = i & 1, (i >> 1) & 1, (i >> 2) & 1
        case |= inside[dz:r - 1 + dz, dy:r - 1 + dy, dx:r - 1 + dx].astype(np.int32) << i
    return case


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(got, want, what=""):
    """NaN where and only where ``want`` has NaN, the same 32 bits everywhere else (-0.0 is not +0.0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN in %d places, expected %d" % (what, np.isnan(got).sum(), nan.sum())
    diff = bits(got)[~nan] != bits(want)[~nan]
    if diff.any():
        err = np.abs(got[~nan].astype(np.float64) - want[~nan].astype(np.float64))
        with np.errstate(invalid="ignore"):
            worst = np.nanmax(np.where(np.isfinite(err), err, np.nan)) if np.isfinite(err).any() else np.nan
        raise AssertionError("%s: %d of %d values differ in bits, largest difference %.3g"
                             % (what, int(diff.sum()), diff.size, worst))
