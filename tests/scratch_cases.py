"""What tests/test_scratch_residue_gpu.py runs every scratch-arena stage on: the fill bytes, the arena size, and the few
inputs the other test modules do not already hold (padded meshes, the second render mesh).  numpy only, no GPU.

The fill bytes.  The launchers establish their scratch by three conventions: hipMemsetAsync(0x00) (valences, list
counters, histogram headers, cell flags), hipMemsetAsync(0xff) (last[v][corner] = -1) and hipMemsetAsync(0x7f) (kNoHit
= 0x7f7f7f7f).  0x00, 0xFF and 0x7F are each what one convention leaves, so each convention is contradicted by the
other two and by 0x5A, a byte no launcher writes.  As data the four give: zero / count 0 / index 0; NaN as f32, -1 as
int32, all-ones bitmaps; 3.39e38 as f32 and 2139062143 as int32; 1.53e16 as f32 and 1515870810 as int32."""
import numpy as np

FILLS = (0x00, 0xFF, 0x7F, 0x5A)
FILL_IDS = ["0x%02X" % b for b in FILLS]
ARENA_BYTES = 32 << 20  # far above what any shape of the file asks for; the tests assert that no call outgrows it

RES = [9, 17, 33]
GARBAGE_INDEX = 2 ** 30  # what the face rows beyond counts[1] hold (tests/test_mesh_gpu.py)


def fill_words(byte):
    """(f32, int32) value of a word of the arena after a fill with ``byte``."""
    raw = np.full(4, byte, np.uint8)
    return raw.view(np.float32)[0], raw.view(np.int32)[0]


def padded_mesh(verts, faces, max_v, max_f, counts=None):
    """(verts [max_v,3] f32, faces [max_f,3] int32, counts int32[2]): the mesh in buffers of a larger capacity, the
    vertex rows beyond it NaN, the face rows beyond it GARBAGE_INDEX except one valid face [0, 1, 2] that must not
    contribute (the buffers of test_mesh_gpu.py's test_counts_below_the_capacities).  ``counts``: what the call is told,
    if less than the mesh."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    assert len(v) < max_v and len(f) + 1 < max_f
    vbuf = np.full((max_v, 3), np.nan, np.float32)
    vbuf[:len(v)] = v
    fbuf = np.full((max_f, 3), GARBAGE_INDEX, np.int32)
    fbuf[:len(f)] = f
    fbuf[len(f) + 1] = (0, 1, 2)
    return vbuf, fbuf, np.array([len(v), len(f)] if counts is None else counts, np.int32)


def mirrored(xyz, attr):
    """The second mesh of the render case: the first one with x and y exchanged and z negated (what was in front is
    behind), the attributes in reverse row order.  Same sizes, another picture."""
    xyz = np.asarray(xyz, np.float32)
    out = np.ascontiguousarray(xyz[:, [1, 0, 2]] * np.array([1.0, 1.0, -1.0], np.float32))
    return out.astype(np.float32), np.ascontiguousarray(np.asarray(attr, np.float32)[::-1])
