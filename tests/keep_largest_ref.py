"""The definition of mp_volume_keep_largest restated in numpy (include/monoport_hip.h), and
the synthetic volumes its tests run on.  tests/test_keep_largest_cpu.py holds the labeller to scipy.ndimage.label;
tests/test_keep_largest_gpu.py holds the kernels to the labeller.  numpy only."""
import functools
import itertools

import numpy as np

LEVEL = 0.5


def forward_offsets(connectivity):
    """(dz, dy, dx) of the neighbours with a larger linear index: 3 for 6, 13 for 26."""
    if connectivity == 6:
        return [(0, 0, 1), (0, 1, 0), (1, 0, 0)]
    assert connectivity == 26
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0)]


def _neighbour_pairs(fg, connectivity):
    """Linear indices (a, b) of every pair of foreground voxels that are forward neighbours."""
    r = fg.shape[0]
    idx = np.arange(fg.size, dtype=np.int64).reshape(fg.shape)
    pa, pb = [], []

    def cut(d):  # the slices of a voxel and of its neighbour at offset d along one axis
        return (slice(max(0, -d), r - max(0, d)), slice(max(0, d), r - max(0, -d)))

    for dz, dy, dx in forward_offsets(connectivity):
        (za, zb), (ya, yb), (xa, xb) = cut(dz), cut(dy), cut(dx)
        both = fg[za, ya, xa] & fg[zb, yb, xb]
        pa.append(idx[za, ya, xa][both])
        pb.append(idx[zb, yb, xb][both])
    return np.concatenate(pa), np.concatenate(pb)


def label_components(fg, connectivity):
    """Component ids of a boolean volume: int64 [R,R,R], the smallest linear index of the voxel's component, -1 for
    background.  Vectorised min-label propagation over the neighbour pairs with pointer jumping."""
    pa, pb = _neighbour_pairs(fg, connectivity)
    lab = np.arange(fg.size, dtype=np.int64)
    while True:
        la, lb = lab[pa], lab[pb]
        if (la == lb).all():
            break
        m = np.minimum(la, lb)
        for target in (la, lb, pa, pb):  # hook the two labels (roots once jumped) and the voxels themselves
            np.minimum.at(lab, target, m)
        while True:  # pointer jumping: a label is the index of a voxel of the same component
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt
    lab = lab.reshape(fg.shape)
    return np.where(fg, lab, -1)


def keep_largest_ref(vol, level=LEVEL, connectivity=6, fill=0.0):
    """(out float32 [R,R,R], stats [foreground, components, kept voxels, kept id]) by the definition."""
    vol = np.asarray(vol, np.float32)
    with np.errstate(invalid="ignore"):
        fg = vol > np.float32(level)  # a NaN compares false: background
    if not fg.any():
        return vol.copy(), [0, 0, 0, -1]
    lab = label_components(fg, connectivity)
    ids, sizes = np.unique(lab[fg], return_counts=True)  # ascending ids: argmax takes the smallest id of a tie
    k = int(np.argmax(sizes))
    out = vol.copy()
    out[fg & (lab != ids[k])] = np.float32(fill)
    return out, [int(fg.sum()), int(ids.size), int(sizes[k]), int(ids[k])]


# ---- the volumes -------------------------------------------------------------------------------------------------

def paint(mask, seed=0):
    """Float32 volume of a boolean mask: foreground uniform in (0.55, 1), background uniform in (0, 0.45) -- every
    voxel its own bits, so a voxel that moved or lost its value shows."""
    rs = np.random.RandomState(seed)
    return np.where(mask, rs.uniform(0.55, 1.0, mask.shape), rs.uniform(0.0, 0.45, mask.shape)).astype(np.float32)


def _grid(r):
    return np.meshgrid(np.arange(r), np.arange(r), np.arange(r), indexing="ij")


def _ball(r, centre, radius):
    z, y, x = _grid(r)
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius ** 2


def _box(r, lo, hi):
    m = np.zeros((r, r, r), bool)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return m


def spheres33():
    return paint(_ball(33, (14, 14, 14), 9) | _ball(33, (27, 27, 27), 3), 1)


def serpentine33():
    """A one-voxel-thick path that snakes through x 0..22 of every second y row of every second z plane (6,935 voxels
    in one chain, whatever the connectivity), and a 5^3 cube three voxels away from it."""
    r, w = 33, 23
    m = np.zeros((r, r, r), bool)
    for z in range(0, r, 2):
        for k, y in enumerate(range(0, r, 2)):
            m[z, y, :w] = True
            if y + 1 < r:
                m[z, y + 1, w - 1 if k % 2 == 0 else 0] = True
        if z + 1 < r:  # every plane has the same pattern: alternate between its end and its start
            m[z + 1, r - 1 if (z // 2) % 2 == 0 else 0, w - 1 if (z // 2) % 2 == 0 else 0] = True
    assert m.sum() == 17 * (17 * w + 16) + 16
    return paint(m | _box(r, (10, 10, 26), (15, 15, 31)), 2)


def equal_cubes17():
    return paint(_box(17, (2, 2, 2), (6, 6, 6)) | _box(17, (10, 10, 10), (14, 14, 14)), 3)


def touching17(direction):
    """A 4^3 cube at [6,10)^3 and a 3^3 cube beside it in `direction` (dz, dy, dx in -1 / 0 / 1): they share a face
    (one non-zero entry), touch along an edge (two) or at a corner (three)."""
    lo = [{-1: 3, 0: 6, 1: 10}[d] for d in direction]
    return paint(_box(17, (6, 6, 6), (10, 10, 10)) | _box(17, lo, [v + 3 for v in lo]), 4)


EDGE_DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if sum(v != 0 for v in d) == 2]
CORNER_DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if sum(v != 0 for v in d) == 3]


def nan_bridge17():
    """Two blobs (64 and 80 voxels) with two columns between them: NaNs of three different bit patterns, and voxels
    exactly at the level.  Neither is foreground, so the blobs stay apart."""
    vol = paint(_box(17, (2, 2, 2), (6, 6, 6)) | _box(17, (2, 2, 8), (6, 6, 13)), 5)
    bits = vol.view(np.uint32)
    bits[2:6, 2:6, 6] = 0x7FC00000
    bits[3, 3, 6] = 0x7FC00001
    bits[4, 4, 6] = 0xFFC00000
    vol[2:6, 2:6, 7] = LEVEL
    bits[0, 0, 0] = 0x7F800001  # a signalling NaN far from everything
    return vol


def empty17():
    vol = paint(np.zeros((17, 17, 17), bool), 6)
    vol[3, 4, 5] = LEVEL
    vol[8, 8, 8] = np.nan
    return vol


def full17():
    return paint(np.ones((17, 17, 17), bool), 7)


def noise65():
    return paint(np.random.RandomState(8).random_sample((65, 65, 65)) < 0.30, 9)


def body129():
    """A sigmoid occupancy field of a figure made of ellipsoids (torso, head, two arms, two legs) and three floaters
    of different size away from it."""
    r = 129
    g = ((np.arange(r) + 0.5) / r) * 2 - 1
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    parts = [((0.0, 0.05, 0.0), (0.16, 0.30, 0.22)), ((0.0, 0.45, 0.0), (0.13, 0.14, 0.12)),
             ((0.0, 0.15, 0.36), (0.08, 0.09, 0.26)), ((0.0, 0.15, -0.36), (0.08, 0.09, 0.26)),
             ((0.0, -0.50, 0.11), (0.10, 0.36, 0.09)), ((0.0, -0.50, -0.11), (0.10, 0.36, 0.09)),
             ((0.6, 0.7, 0.7), (0.06, 0.06, 0.06)), ((-0.7, -0.6, 0.5), (0.04, 0.05, 0.03)),
             ((0.3, 0.8, -0.75), (0.02, 0.02, 0.02))]
    d = np.full((r, r, r), np.inf)
    for (cz, cy, cx), (az, ay, ax) in parts:
        d = np.minimum(d, np.sqrt(((z - cz) / az) ** 2 + ((y - cy) / ay) ** 2 + ((x - cx) / ax) ** 2))
    return (1.0 / (1.0 + np.exp(-10.0 * (1.0 - d)))).astype(np.float32)


def body_floater33():
    """A sphere about the centre and a small one in a corner, as sigmoid fields: a mesh with a loose shell."""
    r = 33
    g = ((np.arange(r) + 0.5) / r) * 2 - 1
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    d = np.minimum(np.sqrt(x * x + y * y + z * z) / 0.5,
                   np.sqrt((x - 0.75) ** 2 + (y - 0.75) ** 2 + (z - 0.75) ** 2) / 0.12)
    return (1.0 / (1.0 + np.exp(-8.0 * (1.0 - d)))).astype(np.float32)


CASES = {"spheres33": spheres33, "serpentine33": serpentine33, "equal_cubes17": equal_cubes17,
         "nan_bridge17": nan_bridge17, "empty17": empty17, "full17": full17, "noise65": noise65, "body129": body129,
         "body_floater33": body_floater33}


@functools.lru_cache(maxsize=None)
def volume(name):
    """The named volume, made once (read-only)."""
    vol = CASES[name]() if isinstance(name, str) else touching17(name)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def reference(name, connectivity, fill=0.0):
    """keep_largest_ref of the named volume, computed once and shared (read-only)."""
    out, stats = keep_largest_ref(volume(name), LEVEL, connectivity, fill)
    out.setflags(write=False)
    return out, stats
