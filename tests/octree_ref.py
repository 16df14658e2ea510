"""Plain numpy restatement of the lossless octree housekeeping (include/monoport_hip.h: mp_octree_select_box,
mp_octree_conflicts) on top of oracle.upsample2x, oracle.dilate_box and oracle.lattice_points, with the bitset / node
code helpers of the C-ABI and the adversarial inputs the kernels of csrc/octree.hip are held to, bit for bit:
random and hand-built volumes with an arbitrary evaluated set, and analytic fields that reach the faces of the box."""
import numpy as np

from oracle import pifu_oracle as oracle
from test_box_threshold_cpu import B_MAX, B_MIN  # noqa: F401  (the off-centre box of the analytic fields)


# ---- bitsets and node codes of the C-ABI ----------------------------------------------------------------------
def pack_bits(mask):
    """bool [r,r,r] -> the u64 bitset [r*r*ceil(r/64)] of the C-ABI (bit x & 63 of word x >> 6 of row (z, y))."""
    r = mask.shape[0]
    w64 = (r + 63) // 64
    padded = np.zeros((r, r, w64 * 64), bool)
    padded[:, :, :r] = mask
    return np.packbits(padded, axis=-1, bitorder="little").view("<u8").reshape(-1).copy()


def unpack_bits(words, r):
    """The inverse of pack_bits: u64 [r*r*ceil(r/64)] -> (bool [r,r,r], bool [r,r,pad]: the pad bits x >= r)."""
    w64 = (r + 63) // 64
    bits = np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8).reshape(r, r, w64 * 8), axis=-1,
                         bitorder="little").astype(bool)
    return bits[:, :, :r], bits[:, :, r:]


def codes(lin, r):
    """Linear indices z r^2 + y r + x -> the sorted node codes x | y << 10 | z << 20 (int64)."""
    z, y, x = np.unravel_index(lin, (r, r, r))
    return np.sort((x | (y << 10) | (z << 20)).astype(np.int64))


def mask_codes(mask):
    """bool [r,r,r] -> the sorted codes of its nodes."""
    return codes(np.flatnonzero(mask), mask.shape[0])


def even_image(ev_prev):
    """The even-coordinate image of the previous level's evaluated set at r = 2 rp - 1."""
    rp = ev_prev.shape[0]
    ev = np.zeros((2 * rp - 1,) * 3, bool)
    ev[::2, ::2, ::2] = ev_prev
    return ev


# ---- the definitions ------------------------------------------------------------------------------------------
def select_level(prev, ev_prev, box, balance=0.5):
    """mp_octree_select_box: (cur f32, flags, selected, ev_after), each [r,r,r] with r = 2 rp - 1.

    cur = upsample2x(prev); mask = upsample2x(prev > balance) (NaN is not inside); flags: box 3 / 7 / 9: 0 < mask < 1,
    box 1: mask == 0.5, box 0: none; selected = the flags dilated by the box (1 and 0: as they are) minus the even
    image of ev_prev; ev_after = that image | selected."""
    if box not in (0, 1, 3, 7, 9):
        raise ValueError("box %r" % (box,))
    prev = np.asarray(prev, np.float32)
    cur = oracle.upsample2x(prev)
    with np.errstate(invalid="ignore"):
        mask = oracle.upsample2x((prev > np.float32(balance)).astype(np.float32))
    if box == 0:
        flags = np.zeros(mask.shape, bool)
    elif box == 1:
        flags = mask == np.float32(0.5)
    else:
        flags = (mask > 0) & (mask < 1)
    ev = even_image(np.asarray(ev_prev, bool))
    selected = (oracle.dilate_box(flags, box) if box >= 3 else flags) & ~ev
    return cur, flags, selected, ev | selected


def conflicts(packed_codes, values, vol, ev, balance=0.5):
    """mp_octree_conflicts: (sorted codes of the newly claimed nodes (int64), the evaluated set after the call).

    Node i (code x | y << 10 | z << 20, exact value values[i], interpolated value vol[z,y,x]) is in conflict iff
    (interp - balance) * (value - balance) < 0 in f32 (false for NaN and for a factor of 0); the 3^3 neighbourhoods of
    the conflicting nodes, clipped to the volume, minus ``ev`` are claimed."""
    c = np.asarray(packed_codes, np.int64)
    x, y, z = c & 1023, (c >> 10) & 1023, c >> 20
    bv = np.float32(balance)
    with np.errstate(invalid="ignore"):
        hit = ((np.asarray(vol, np.float32)[z, y, x] - bv) * (np.asarray(values, np.float32) - bv)) < 0
    grow = np.zeros(vol.shape, bool)
    grow[z[hit], y[hit], x[hit]] = True
    grow = oracle.dilate_box(grow, 3) & ~np.asarray(ev, bool)
    return mask_codes(grow), ev | grow


# ---- volumes [rp,rp,rp] f32 with a random evaluated set of density 0.5 -------------------------------------------
def _outside(rng, rp):
    return (rng.random((rp, rp, rp), dtype=np.float32) * np.float32(0.49)).astype(np.float32)


def _inside(rng, n):
    return (np.float32(0.51) + rng.random(n, dtype=np.float32) * np.float32(0.49)).astype(np.float32)


def _ev(rng, rp):
    return rng.random((rp, rp, rp)) < 0.5


def noise(rp, seed):
    """About 3 % of the nodes in [0.51, 1), the rest in [0, 0.49) (a third of those above 0.3), 0.2 % NaN; at least
    one inside node, and one NaN from 3^3 on."""
    rng = np.random.default_rng(seed)
    n = rp ** 3
    prev = _outside(rng, rp)
    order = rng.permutation(n)
    n_in = max(1, int(round(0.03 * n)))
    n_nan = max(1 if n >= 27 else 0, int(round(0.002 * n)))
    prev.reshape(-1)[order[:n_in]] = _inside(rng, n_in)
    prev.reshape(-1)[order[n_in:n_in + n_nan]] = np.nan
    return prev, _ev(rng, rp)


def faces(rp, seed):
    """Inside values on 40 % of the nodes of the planes z = 0, y = rp - 1, x = 0 and x = rp - 1: flags on the faces
    of the volume and one node off them, so the dilation is clipped in y, z and x (first and last word)."""
    rng = np.random.default_rng(seed)
    prev = _outside(rng, rp)
    on = np.zeros((rp, rp, rp), bool)
    on[0, :, :] = on[:, rp - 1, :] = on[:, :, 0] = on[:, :, rp - 1] = True
    on &= rng.random((rp, rp, rp)) < 0.4
    on[0, rp - 1, 0] = True
    prev[on] = _inside(rng, int(on.sum()))
    return prev, _ev(rng, rp)


def sparse(rp, seed):
    """Twelve inside nodes (fewer where the volume has no room), no two of them neighbours."""
    rng = np.random.default_rng(seed)
    prev = _outside(rng, rp)
    chosen = []
    for lin in rng.permutation(rp ** 3):
        p = np.array(np.unravel_index(lin, (rp, rp, rp)))
        if all(np.abs(p - q).max() >= 2 for q in chosen):
            chosen.append(p)
            if len(chosen) == 12:
                break
    for p in chosen:
        prev[tuple(p)] = _inside(rng, 1)[0]
    return prev, _ev(rng, rp)


SEAM_ROWS = ((30, 31), (33,), (32,), (31,), (30, 31, 32, 33))


def seam(rp, seed):
    """Inside nodes next to the word boundaries of the fine level (r = 2 rp - 1 >= 67): on the four rows y, z in
    {0, rp - 1} and on one interior row, parent x from {30, 31, 32, 33} -- a different subset per row (SEAM_ROWS), so
    that one row has its flags only below x = 64, one only above x = 63, and the others on both sides -- and the
    last node x = rp - 1 of each of the five rows."""
    if rp < 34:
        raise ValueError("seam needs rp >= 34")
    rng = np.random.default_rng(seed)
    prev = _outside(rng, rp)
    m = rp // 2
    for (z, y), xs in zip(((0, 0), (0, rp - 1), (rp - 1, 0), (rp - 1, rp - 1), (m, m)), SEAM_ROWS):
        for x in xs + (rp - 1,):
            prev[z, y, x] = _inside(rng, 1)[0]
    return prev, _ev(rng, rp)


def plateau(rp, seed, balance=0.5):
    """Values exactly on ``balance`` (outside: the test is a strict >) next to values one ulp above it (inside), among
    nodes clearly below and a few clearly above."""
    rng = np.random.default_rng(seed)
    b = np.float32(balance)
    values = np.array([b, np.nextafter(b, np.float32(1)), b * np.float32(0.5), b + np.float32(0.25)], np.float32)
    prev = values[rng.choice(4, size=(rp, rp, rp), p=[0.4, 0.15, 0.4, 0.05])]
    prev.reshape(-1)[rng.permutation(rp ** 3)[:4]] = values  # each of them at least once
    return prev, _ev(rng, rp)


VOLUMES = dict(noise=noise, faces=faces, sparse=sparse, seam=seam, plateau=plateau)


# ---- analytic fields: world points [3,N] (any float type, evaluated in float64) -> [N] f32 ---------------------
FIN_RADIUS, FIN_HALF, FIN_SLOPE = 0.45, 0.04, 40.0
FIN_NORMAL = np.array([0.2, 1.0, -0.3]) / np.linalg.norm([0.2, 1.0, -0.3])
FIN_OFFSET = 0.1
CORNER_RADIUS, CORNER_SLOPE = 0.55, 30.0


def _sigmoid(t):
    return (1.0 / (1.0 + np.exp(-t))).astype(np.float32)


def _unit(points, b_min, b_max):
    """World points -> [0, 1]^3 of the box, float64."""
    lo = np.asarray(b_min, np.float32).astype(np.float64)[:, None]
    hi = np.asarray(b_max, np.float32).astype(np.float64)[:, None]
    return (np.asarray(points, np.float64) - lo) / (hi - lo)


def fin_field(points, b_min=B_MIN, b_max=B_MAX):
    """A ball of radius 0.45 around the centre of the box in union with a tilted sheet of half-thickness 0.04 that
    crosses the whole box (lengths in [-1, 1]^3 of the box), through a sigmoid of slope 40: the body touches four
    faces of the box, and the sheet is thinner than the spacing of the coarse levels."""
    u = _unit(points, b_min, b_max) * 2.0 - 1.0
    ball = FIN_RADIUS - np.sqrt((u * u).sum(0))
    sheet = FIN_HALF - np.abs(FIN_NORMAL @ u - FIN_OFFSET)
    return _sigmoid(FIN_SLOPE * np.maximum(ball, sheet))


def corner_field(points, b_min=B_MIN, b_max=B_MAX):
    """A ball of radius 0.55 (in units of the box) around the min corner of the box, sigmoid slope 30."""
    t = _unit(points, b_min, b_max)
    return _sigmoid(CORNER_SLOPE * (CORNER_RADIUS - np.sqrt((t * t).sum(0))))


FIELDS = dict(fin=fin_field, corner=corner_field)


def faces_reached(inside):
    """How many of the six faces of a bool volume hold an inside voxel."""
    return sum(bool(inside.take(i, axis).any()) for axis in range(3) for i in (0, -1))
