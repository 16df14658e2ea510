"""The definition of mp_mesh_simplify restated in numpy (include/monoport_hip.h), and the
meshes its tests run on.  tests/test_mesh_simplify_ref_cpu.py holds the restatement to a dict-and-loop implementation
and to exact rational arithmetic; tests/test_mesh_simplify_gpu.py holds the kernels to the restatement.  numpy only."""
import functools

import numpy as np

SCALE = 1048576.0  # 2^20: the fixed point of the coordinate sums
LIMIT = np.float32(32768.0)  # a coordinate at or beyond it (or not finite) makes a vertex invalid
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def cell_keys(verts, n, b_min=BMIN, b_max=BMAX):
    """Step 1: (key int64 [V], valid bool [V]); the key of an invalid vertex is -1.  Every operation in f32."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    lo, hi = np.asarray(b_min, np.float32), np.asarray(b_max, np.float32)
    inv = np.float32(n) / (hi - lo)
    assert inv.dtype == np.float32 and np.isfinite(inv).all()
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (np.abs(v) < LIMIT).all(1)  # False for NaN and inf too
        t = (v - lo) * inv
        assert t.dtype == np.float32
        c = np.clip(np.floor(np.where(valid[:, None], t, np.float32(0))), 0, n - 1).astype(np.int64)
    key = (c[:, 2] * n + c[:, 1]) * n + c[:, 0]
    return np.where(valid, key, -1), valid


def simplify_ref(verts, faces, n, b_min=BMIN, b_max=BMAX):
    """-> (verts_out f32 [V',3], faces_out int32 [F',3], vmap int32 [V])."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    key, valid = cell_keys(v, n, b_min, b_max)
    # 2: one new vertex per occupied cell, ascending in key
    cells, member_of = np.unique(key[valid], return_inverse=True)
    vmap = np.full(len(v), -1, np.int32)
    vmap[valid] = member_of
    # 3: the mean in fixed point
    q = np.rint(v[valid].astype(np.float64) * SCALE).astype(np.int64)  # exact product, ties to even
    sums = np.zeros((len(cells), 3), np.int64)
    np.add.at(sums, member_of, q)
    m = np.bincount(member_of, minlength=len(cells)).astype(np.int64)
    out = (sums.astype(np.float64) / (m.astype(np.float64) * SCALE)[:, None]).astype(np.float32)
    # 4: faces
    ok = ((f >= 0) & (f < len(v))).all(1)
    g = np.full(f.shape, -1, np.int64)
    g[ok] = vmap[f[ok]]
    ok &= (g >= 0).all(1)
    ok &= (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    return out, g[ok].astype(np.int32), vmap


def edge_parity_even(faces):
    """True if every undirected edge lies in an even number of the faces."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return True
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return bool((cnt % 2 == 0).all())


@functools.lru_cache(maxsize=None)
def oracle_mesh(name):
    """The oracle's marching-cubes mesh of a synthetic volume: "blob33_5", "blob17_3", "sphere33"."""
    from monoport_amd import synthetic as syn
    from oracle import pifu_oracle
    vol = {"blob33_5": lambda: syn.blob_volume(33, 5), "blob17_3": lambda: syn.blob_volume(17, 3),
           "sphere33": lambda: syn.sphere_volume(33)}[name]()
    v, f = pifu_oracle.marching_cubes(vol)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


SOUP_BMIN, SOUP_BMAX, SOUP_CELLS = (-0.5, -1.0, 0.25), (1.5, 0.0, 0.75), 8  # off-centre, not a cube: cells of 1/4, 1/8, 1/16


@functools.lru_cache(maxsize=None)
def soup():
    """A triangle soup for the box above: vertices inside, outside (border cells), exactly on cell borders (t an
    integer) and on b_max, every kind of invalid vertex, and faces with out-of-range indices, invalid vertices, two
    corners in one cell, and duplicates.  -> (verts f32 [V,3], faces int32 [F,3])."""
    rng = np.random.RandomState(20)
    lo, hi = np.asarray(SOUP_BMIN, np.float32), np.asarray(SOUP_BMAX, np.float32)
    inside = (lo + (hi - lo) * rng.rand(400, 3)).astype(np.float32)
    outside = (lo + (hi - lo) * (rng.rand(60, 3) * 3.0 - 1.0)).astype(np.float32)
    step = (hi - lo) / np.float32(SOUP_CELLS)
    border = (lo + step * rng.randint(0, SOUP_CELLS + 1, (60, 3)).astype(np.float32)).astype(np.float32)  # exact in f32
    corner = np.array([hi, lo, [hi[0], lo[1], hi[2]]], np.float32)
    far = np.array([[32767.998, 0, 0.5], [-32767.998, -0.5, 0.5], [1e-30, -1e-30, 0.5]], np.float32)  # still valid
    bad = np.array([[np.nan, -0.5, 0.5], [0.5, np.inf, 0.5], [0.5, -0.5, -np.inf], [32768.0, -0.5, 0.5],
                    [0.5, -32768.0, 0.5], [0.5, -0.5, 3e38]], np.float32)
    verts = np.concatenate([inside, outside, border, corner, far, bad])
    nv = len(verts)
    first_bad = nv - len(bad)
    faces = rng.randint(0, first_bad, (900, 3)).astype(np.int32)
    faces[::50, 1] = rng.randint(first_bad, nv, len(faces[::50]))  # an invalid vertex
    faces[7::60, 2] = nv + rng.randint(0, 5, len(faces[7::60]))  # beyond the vertices
    faces[11::70, 0] = -1 - rng.randint(0, 5, len(faces[11::70]))  # negative
    faces[13::40, 2] = faces[13::40, 0]  # a vertex twice
    faces[100:110] = faces[90:100]  # duplicates: both stay
    faces[110:120] = faces[90:100][:, ::-1]  # and their mirror images
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


@functools.lru_cache(maxsize=None)
def crowd(members=300000, seed=21):
    """``members`` vertices near (30000, -30000, 30000) in ONE cell of a 2^3 grid over [-32768, 32768]^3: the sums pass
    2^53.  No faces.  -> verts f32 [members,3]."""
    rng = np.random.RandomState(seed)
    v = (np.array([30000.0, -30000.0, 30000.0]) + rng.rand(members, 3) * 64.0 - 32.0).astype(np.float32)
    v.setflags(write=False)
    return v


CROWD_BMIN, CROWD_BMAX, CROWD_CELLS = (-32768.0,) * 3, (32768.0,) * 3, 2
