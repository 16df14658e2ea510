"""The definition of mp_mesh_smooth restated in numpy (include/monoport_hip.h), and the
meshes its tests run on.  tests/test_mesh_smooth_ref_cpu.py holds the restatement to a dict-and-loop implementation and
to the quality facts; tests/test_mesh_smooth_gpu.py holds the kernels to the restatement.  numpy only."""
import functools

import numpy as np


def directed_pairs(faces, nv):
    """Step 1: the directed entries (v, b) of every edge with distinct ends of every valid face, both directions, with
    repetitions, sorted by (v, b) -> int64 [E,2]."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < nv)).all(1)]
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    e = np.concatenate([e, e[:, ::-1]])
    return e[np.lexsort((e[:, 1], e[:, 0]))]


def ring_of(faces, nv):
    """-> (pairs int64 [P,2]: the distinct (v, b) sorted by (v, b); deg int64 [nv]; border bool [nv])."""
    e = directed_pairs(faces, nv)
    if len(e) == 0:
        return np.zeros((0, 2), np.int64), np.zeros(nv, np.int64), np.zeros(nv, bool)
    pairs, mult = np.unique(e, axis=0, return_counts=True)  # sorted by (v, b); mult = m(v, b)
    deg = np.bincount(pairs[:, 0], minlength=nv)
    border = np.zeros(nv, bool)
    border[pairs[mult % 2 == 1, 0]] = True
    return pairs, deg, border


def ring_ref(verts, faces):
    """The optional ``ring`` output: d(v), negated for a border vertex -> int32 [V]."""
    nv = len(np.asarray(verts).reshape(-1, 3))
    _, deg, border = ring_of(faces, nv)
    return np.where(border, -deg, deg).astype(np.int32)


def smooth_ref(verts, faces, iterations, lam=0.5, mu=-0.53, pin=True):
    """-> verts_out f32 [V,3].  np.add.at adds the pairs one after the other in their (v, b) order, in f32."""
    p = np.array(verts, np.float32).reshape(-1, 3)
    nv = len(p)
    pairs, deg, border = ring_of(faces, nv)
    fixed = (deg == 0) | (border & bool(pin))
    free = ~fixed
    fdeg = deg.astype(np.float32)[free, None]
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(iterations):
            for phi in (np.float32(lam), np.float32(mu)):
                s = np.zeros((nv, 3), np.float32)
                np.add.at(s, pairs[:, 0], p[pairs[:, 1]])
                m = s[free] / fdeg
                q = p.copy()
                q[free] = p[free] + phi * (m - p[free])
                assert m.dtype == np.float32 and q.dtype == np.float32
                p = q
    return p


def loop_ref(verts, faces, iterations, lam=0.5, mu=-0.53, pin=True):
    """The definition once more, one face, one vertex and one np.float32 operation at a time -> (verts_out, ring)."""
    f32 = np.float32
    p = [[f32(x) for x in row] for row in np.asarray(verts, np.float32).reshape(-1, 3)]
    nv = len(p)
    m = [dict() for _ in range(nv)]
    for face in np.asarray(faces).reshape(-1, 3).tolist():
        if any(i < 0 or i >= nv for i in face):
            continue
        for a, b in ((face[0], face[1]), (face[1], face[2]), (face[2], face[0])):
            if a == b:
                continue
            m[a][b] = m[a].get(b, 0) + 1
            m[b][a] = m[b].get(a, 0) + 1
    nbrs = [sorted(d) for d in m]
    border = [any(c % 2 for c in d.values()) for d in m]
    fixed = [len(nbrs[v]) == 0 or (bool(pin) and border[v]) for v in range(nv)]
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(iterations):
            for phi in (f32(lam), f32(mu)):
                q = []
                for v in range(nv):
                    if fixed[v]:
                        q.append(p[v])
                        continue
                    row = []
                    for a in range(3):
                        s = f32(0.0)
                        for b in nbrs[v]:
                            s = f32(s + p[b][a])
                        mean = f32(s / f32(len(nbrs[v])))
                        row.append(f32(p[v][a] + f32(phi * f32(mean - p[v][a]))))
                    q.append(row)
                p = q
    ring = np.array([-len(nbrs[v]) if border[v] else len(nbrs[v]) for v in range(nv)], np.int32).reshape(-1)
    return np.array(p, np.float32).reshape(-1, 3), ring


def same_bits(got, want):
    """True if two f32 arrays agree: the same bits wherever ``want`` is not NaN, NaN for NaN elsewhere (the sign and
    payload of a NaN that an operation produces differ between processors)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and np.isnan(got[nan]).all())


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle_mesh(name):
    """The oracle's marching-cubes mesh of a synthetic volume: "blob33_5", "blob17_3", "sphere65" (sphere_volume(65))
    and "steps65" (the same volume binarised at 0.5: the terraced surface of a saturated field)."""
    from monoport_amd import synthetic as syn
    from oracle import pifu_oracle
    vol = {"blob33_5": lambda: syn.blob_volume(33, 5), "blob17_3": lambda: syn.blob_volume(17, 3),
           "sphere65": lambda: syn.sphere_volume(65),
           "steps65": lambda: (syn.sphere_volume(65) > 0.5).astype(np.float32)}[name]()
    return _frozen(*pifu_oracle.marching_cubes(vol))


def open_faces(faces):
    """``faces`` with every 40th removed: the holes' rims are border vertices."""
    f = np.asarray(faces)
    keep = np.ones(len(f), bool)
    keep[::40] = False
    return _frozen(f[keep].copy())[0]


@functools.lru_cache(maxsize=None)
def open_mesh():
    """The blob_volume(33, 5) mesh with every 40th face removed (227 border vertices of 1,562)."""
    v, f = oracle_mesh("blob33_5")
    return v, open_faces(f)


@functools.lru_cache(maxsize=None)
def soup():
    """synthetic.normals_soup_mesh(): a random soup with a vertex twice in a face, huge and tiny coordinates,
    degenerate faces, unreferenced vertices and a fan of 200 faces -> (verts, faces)."""
    from monoport_amd import synthetic as syn
    v, f, _ = syn.normals_soup_mesh()
    return _frozen(v.copy(), f.copy())


@functools.lru_cache(maxsize=None)
def book(pages=2000):
    """``pages`` faces that share the edge (0, 1), each with a third vertex of its own: two vertices of valence
    pages + 1 whose segments every face writes to -> (verts f32 [pages + 2, 3], faces int32 [pages, 3])."""
    rng = np.random.RandomState(31)
    v = np.concatenate([[[0.0, 0.0, -0.5], [0.0, 0.0, 0.5]], rng.standard_normal((pages, 3))]).astype(np.float32)
    f = np.stack([np.zeros(pages), np.ones(pages), 2 + rng.permutation(pages)], 1).astype(np.int32)
    f[1::2] = f[1::2][:, [2, 0, 1]]
    return _frozen(v, f)
