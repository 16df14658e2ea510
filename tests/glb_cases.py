"""The meshes the binary glTF tests share (tests/test_glb_ref_cpu.py on the restatement alone, tests/test_glb_gpu.py
against the device): small enough to be milliseconds, at every size and value at which the writer takes another path."""
import collections
import functools

import numpy as np

import glb_ref as ref

F = np.float32
Case = collections.namedtuple("Case", ["name", "verts", "faces", "counts", "normals", "colors", "b_min", "b_max"])
Case.__doc__ = """Capacity-sized arrays as the mesh chain leaves them: verts [max_v,3] f32, faces [max_f,3] int32, counts
(vertices, faces) -- possibly beyond the capacities --, normals [max_v,3], colours [max_v,3] in rows, and the box."""
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
SKEW = ((-0.7, 0.2, -3.0), (1.9, 0.45, 5.0))  # off-centre, another width on every axis
ATTRIBUTE_SETS = ((False, False), (True, False), (False, True), (True, True))
inf, nan = F(np.inf), F(np.nan)


def random_mesh(name, nv, nf, seed, box=UNIT, counts=None, spill=0.02):
    """nv vertices a little beyond the box, nf faces over all of them (the last vertex in the last face), unit normals,
    colours a little beyond [0, 1]."""
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(box[0], F), np.asarray(box[1], F)
    verts = (lo + (hi - lo) * rs.uniform(-spill, 1 + spill, (nv, 3))).astype(F)
    faces = rs.randint(0, nv, (nf, 3)).astype(np.int32)
    if nf:
        faces[-1] = (nv - 1, 0, nv // 2)
    normals = rs.normal(size=(nv, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F)
    colors = rs.uniform(-0.1, 1.1, (nv, 3)).astype(F)
    return Case(name, verts, faces, (nv, nf) if counts is None else counts, normals, colors, box[0], box[1])


def one_triangle():
    verts = np.array([[-1, -1, -1], [1, 1, 1], [0.25, -0.5, 0.75]], F)
    return Case("one_triangle", verts, np.array([[0, 1, 2]], np.int32), (3, 1),
                np.array([[0, 0, 1], [0, -1, 0], [0.6, 0, -0.8]], F), np.array([[1, 0, 0], [0, 1, 0], [0.2, 0.4, 0.6]], F),
                *UNIT)


def around_the_box():
    """Vertices on the skew box's corners and faces, half a step and a step outside, and far outside."""
    lo, hi = np.asarray(SKEW[0], F), np.asarray(SKEW[1], F)
    step = (hi - lo) / F(65535)
    rows = [lo, hi, (lo + hi) / 2, lo - step / 2, hi + step / 2, lo - step, hi + step, lo + step * F(0.49),
            lo + step * F(0.51), hi - step * F(0.49), hi - step * F(0.51), lo - 100, hi + 100, lo * 0 + F(1e30),
            lo * 0 - F(1e30), np.array([lo[0], hi[1], 1e38], F), np.array([3e38, lo[1], hi[2]], F)]
    verts = np.stack(rows).astype(F)
    c = random_mesh("", len(verts), 9, 5, SKEW)
    return c._replace(name="around_the_box", verts=verts)


def specials():
    """NaN, +-inf and -0.0 in positions, normals and colours; zero-length and over-long normals."""
    c = random_mesh("specials", 12, 6, 6)
    v, n, col = c.verts.copy(), c.normals.copy(), c.colors.copy()
    v[0], v[1], v[2], v[3] = (nan, 0, 0), (inf, -inf, nan), (-0.0, 0.0, -0.0), (-inf, inf, 0.5)
    n[0], n[1], n[2], n[3] = (nan, nan, nan), (inf, -inf, 0), (-0.0, 0.0, -0.0), (0, 0, 0)
    n[4], n[5], n[6] = (3, -4, 0.5), (1, -1, 0.99999994), (0.0039, -0.0039, 0.0040)
    col[0], col[1], col[2], col[3] = (nan, 0.5, nan), (inf, -inf, 1), (-0.0, 0.0, 1e-8), (0.5 / 255, 1.5 / 255, 254.5 / 255)
    return c._replace(verts=v, normals=n, colors=col)


def wild_indices():
    c = random_mesh("wild_indices", 20, 6, 7)
    f = c.faces.copy()
    f[0], f[1], f[2], f[3] = (-5, 20, 19), (2 ** 31 - 1, -2 ** 31, 0), (21, 65535, 65536), (-1, 1, 1)
    return c._replace(faces=f)


@functools.lru_cache(maxsize=None)
def small_cases():
    return (
        one_triangle(),
        random_mesh("odd_faces", 50, 7, 1),
        random_mesh("even_faces", 50, 8, 2),
        random_mesh("two_blocks", 300, 515, 3, SKEW),  # more than one workgroup of vertices and of face pairs
        random_mesh("more_verts_than_faces", 700, 3, 4),
        around_the_box(),
        specials(),
        wild_indices(),
        random_mesh("counts_above", 40, 30, 8, counts=(45, 33)),
        random_mesh("counts_partial", 40, 30, 9, counts=(17, 11)),
        random_mesh("verts_above_only", 40, 30, 10, counts=(2 ** 31 - 1, 5)),
        random_mesh("no_vertices", 8, 4, 11, counts=(0, 4)),
        random_mesh("no_faces", 8, 4, 12, counts=(8, 0)),
        random_mesh("gated_off", 8, 4, 13, counts=(0, 0)),
        random_mesh("negative_counts", 8, 4, 14, counts=(-3, -1)),
    )


@functools.lru_cache(maxsize=None)
def index_width_cases():
    """65 535 vertices keep 16-bit indices, 65 536 need 32 bits; a handful of faces that reach the last vertex."""
    return tuple(random_mesh("nv_%d" % nv, nv, 5, nv) for nv in (65535, 65536))


_RESTATED = {}


def restated(case, normals=True, colors=True, layout="rows", scale=1.0, bias=0.0):
    """The restatement's file of a case, made once for all tests (the cases' names are unique).  ``layout`` "planes":
    the colours transposed."""
    key = (case.name, normals, colors, layout, scale, bias)
    if key not in _RESTATED:
        col = None
        if colors:
            col = case.colors.T.copy() if layout == "planes" else case.colors
        _RESTATED[key] = ref.encode(case.verts, case.faces, case.counts, case.normals if normals else None, col, layout,
                                    scale, bias, case.b_min, case.b_max)
    return _RESTATED[key]
