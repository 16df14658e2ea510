"""The meshes and atlas sizes the texture-atlas tests share (tests/test_atlas_ref_cpu.py on the restatements alone,
tests/test_atlas_gpu.py and tests/test_glb_textured_gpu.py against the device): capacity-sized arrays as the mesh chain
leaves them, small enough to be milliseconds, at every size at which the layout takes another path."""
import collections
import functools

import numpy as np

import atlas_ref
import glb_cases

F = np.float32
Case = collections.namedtuple("Case", ["name", "verts", "faces", "counts", "normals", "size", "cell", "b_min", "b_max"])
Case.__doc__ = """verts [max_v,3] f32, faces [max_f,3] int32, counts (vertices, faces) -- possibly beyond the capacities
--, normals [max_v,3], the atlas (size, cell) and the box of the file's positions."""
inf, nan = F(np.inf), F(np.nan)


def _from_glb(c, size, cell, name=None):
    return Case(name or "%s_%d_%d" % (c.name, size, cell), c.verts, c.faces, c.counts, c.normals, size, cell, c.b_min,
                c.b_max)


def hand_made(nf, size=64, cell=8):
    """1, 2 or 3 faces over five vertices, written out by hand."""
    verts = np.array([[-0.5, -0.25, 0.125], [0.75, -0.5, 0.25], [0.0, 0.875, -0.375], [0.625, 0.5, 0.75],
                      [-0.875, 0.25, -0.625]], F)
    faces = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 2]], np.int32)[:nf]
    normals = np.array([[0, 0, 1], [0, -1, 0], [0.6, 0, -0.8], [1, 0, 0], [0, 0.8, 0.6]], F)
    return Case("hand_%d_%d_%d" % (nf, size, cell), verts, faces, (5, nf), normals, size, cell, *glb_cases.UNIT)


@functools.lru_cache(maxsize=None)
def sphere(r):
    """The marching-cubes mesh of sphere_volume(r) from the float64 oracle, with unit normals: (verts, faces, normals)."""
    from monoport_amd import synthetic as syn
    from oracle import pifu_oracle
    v, f = pifu_oracle.marching_cubes(syn.sphere_volume(r))
    v, f = np.ascontiguousarray(v, F), np.ascontiguousarray(f, np.int32)
    n = (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9)).astype(F)
    for a in (v, f, n):
        a.setflags(write=False)
    return v, f, n


def sphere_case(r, size, cell):
    v, f, n = sphere(r)
    return Case("sphere%d_%d_%d" % (r, size, cell), v, f, (len(v), len(f)), n, size, cell, *glb_cases.UNIT)


def full(size, cell, extra):
    """A random mesh of exactly 2 G^2 + extra faces."""
    nf = atlas_ref.capacity(size, cell) + extra
    c = glb_cases.random_mesh("full%+d" % extra, 40, nf, 40 + extra, glb_cases.SKEW)
    return _from_glb(c, size, cell)


def specials(size=64, cell=5):
    """NaN, +-inf and -0.0 vertices, out-of-range indices: two of glb_cases' meshes in one atlas each."""
    small = glb_cases.small_cases()
    return [_from_glb(small[6], size, cell), _from_glb(small[7], size, cell)]


@functools.lru_cache(maxsize=None)
def cases():
    small = glb_cases.small_cases()
    out = [hand_made(1), hand_made(2), hand_made(3), hand_made(3, 64, 4), hand_made(2, 128, 64), hand_made(3, 64, 5),
           sphere_case(17, 128, 4), sphere_case(17, 64, 4),  # the second: more faces than the atlas holds
           sphere_case(33, 256, 4), sphere_case(17, 256, 5), sphere_case(17, 256, 8),
           _from_glb(small[1], 64, 8), _from_glb(small[2], 64, 8),  # odd and even face counts
           _from_glb(small[3], 128, 5),  # a cell that does not divide the side: margins
           full(64, 8, 0), full(64, 8, 1), full(128, 64, 0), full(128, 64, 1)]
    out += specials()
    out += [_from_glb(small[k], 64, 8) for k in (8, 9, 10, 11, 12, 13, 14)]  # counts above / partial / empty / negative
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


_ATLAS = {}


def restated(case, background=0.5):
    """The restatement's (face_id, position, info) of a case, made once for all tests."""
    key = (case.name, background)
    if key not in _ATLAS:
        _ATLAS[key] = atlas_ref.atlas(case.verts, case.faces, case.size, case.cell, background, case.counts)
        for a in _ATLAS[key]:
            a.setflags(write=False)
    return _ATLAS[key]


# rows of absolute sum <= 0.4 and offsets <= 0.1: within +-0.5 on the unit box, which leaves the gutter texels -- the
# face's plane extrapolated by up to half a leg -- inside raw [-1, 1] as well, where no clamp bends the field
AFFINE = ([[0.2, -0.125, 0.075], [0.05, 0.175, -0.15], [-0.1, 0.075, 0.2]], [0.1, -0.05, 0.075])


def affine_colour(points):
    """A colour field for the tests that play the viewer: raw predictions that are an affine function of the position,
    [..., 3] -> [..., 3] in float64 (the painted colour is raw * 0.5 + 0.5)."""
    return np.asarray(points, np.float64) @ np.array(AFFINE[0], np.float64).T + np.array(AFFINE[1], np.float64)
