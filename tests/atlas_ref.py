"""The texture atlas of mp_mesh_atlas (include/monoport_hip.h) restated in numpy, bit for bit: the G-buffer of a mesh in
texture space, the closed form of the corner UVs, and -- for the tests that play the viewer -- the bilinear lookup of
glTF's LINEAR filter with CLAMP_TO_EDGE."""
import numpy as np

F = np.float32


def grid(size, cell):
    return size // cell


def capacity(size, cell):
    """The faces an atlas holds: 2 G^2."""
    return 2 * grid(size, cell) ** 2


def counts_of(verts, faces, counts=None):
    """(nv, nf) as the call clamps them; nf = 0 where nv == 0."""
    counts = (len(verts), len(faces)) if counts is None else counts
    nv = min(max(int(counts[0]), 0), len(verts))
    nf = min(max(int(counts[1]), 0), len(faces)) if nv else 0
    return nv, nf


def texel_faces(size, cell):
    """Per texel of the [size,size] picture (row y, column x): (face slot or -1 in the margins, a, b, leg) -- the slot
    is 2 q + h whatever the mesh's face count."""
    g = grid(size, cell)
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    cx, cy = x // cell, y // cell
    i, j = x - cx * cell, y - cy * cell
    h = (i + j >= cell).astype(np.int64)
    slot = np.where((cx < g) & (cy < g), 2 * (cy * g + cx) + h, -1)
    a = np.where(h == 1, cell - 1 - i, i)
    b = np.where(h == 1, cell - 1 - j, j)
    return slot, a, b, cell - 2 - h


def atlas(verts, faces, size, cell, background=0.5, counts=None):
    """-> (face_id int32 [size,size], position f32 [size,size,3], info int32[2])."""
    verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    nv, nf = counts_of(verts, faces, counts)
    laid = min(nf, capacity(size, cell))
    slot, a, b, leg = texel_faces(size, cell)
    own = (slot >= 0) & (slot < laid)
    face_id = np.where(own, slot, -1).astype(np.int32)
    position = np.full((size, size, 3), F(background), F)
    if laid:
        tri = np.clip(faces[face_id[own]].astype(np.int64), 0, nv - 1)
        with np.errstate(all="ignore"):
            s = (a[own].astype(F) / leg[own].astype(F)).astype(F)[:, None]
            t = (b[own].astype(F) / leg[own].astype(F)).astype(F)[:, None]
            v0 = verts[tri[:, 0]]
            e1 = (verts[tri[:, 1]] - v0).astype(F)
            e2 = (verts[tri[:, 2]] - v0).astype(F)
            position[own] = ((v0 + (s * e1).astype(F)).astype(F) + (t * e2).astype(F)).astype(F)
    return face_id, position, np.array([laid, nf], np.int32)


def corner_texels(nf, size, cell):
    """The texel (x, y) of every corner of faces 0..nf-1 (all < 2 G^2): int64 [nf,3,2]."""
    g = grid(size, cell)
    f = np.arange(nf, dtype=np.int64)
    q, h = f >> 1, f & 1
    leg = cell - 2 - h
    ci = np.stack([np.zeros_like(leg), leg, np.zeros_like(leg)], axis=1)  # (0,0), (l,0), (0,l)
    cj = np.stack([np.zeros_like(leg), np.zeros_like(leg), leg], axis=1)
    up = (h == 1)[:, None]
    x = (q % g)[:, None] * cell + np.where(up, cell - 1 - ci, ci)
    y = (q // g)[:, None] * cell + np.where(up, cell - 1 - cj, cj)
    return np.stack([x, y], axis=2)


def corner_uvs(nf, size, cell):
    """TEXCOORD_0 of the 3 nf corner vertices: f32 [nf,3,2] = (texel + 0.5) / size, exact."""
    return ((corner_texels(nf, size, cell).astype(F) + F(0.5)).astype(F) / F(size)).astype(F)


def bilinear_footprint(uv, size):
    """glTF's LINEAR magnification with CLAMP_TO_EDGE at uv [n,2] (float64): the four texels (x, y) int64 [n,4,2] and
    their weights [n,4], as a viewer takes them."""
    p = np.asarray(uv, np.float64) * size - 0.5
    p0 = np.floor(p)
    fr = p - p0
    xs = np.stack([p0[:, 0], p0[:, 0] + 1, p0[:, 0], p0[:, 0] + 1], axis=1)
    ys = np.stack([p0[:, 1], p0[:, 1], p0[:, 1] + 1, p0[:, 1] + 1], axis=1)
    w = np.stack([(1 - fr[:, 0]) * (1 - fr[:, 1]), fr[:, 0] * (1 - fr[:, 1]), (1 - fr[:, 0]) * fr[:, 1],
                  fr[:, 0] * fr[:, 1]], axis=1)
    tex = np.stack([np.clip(xs, 0, size - 1), np.clip(ys, 0, size - 1)], axis=2).astype(np.int64)
    return tex, w


def sample_bilinear(image, uv):
    """``image`` [size,size,C] looked up at uv [n,2] in float64."""
    tex, w = bilinear_footprint(uv, image.shape[0])
    return (np.asarray(image, np.float64)[tex[..., 1], tex[..., 0]] * w[..., None]).sum(axis=1)


def surface_points(nf, size, cell, per_face, seed, edges=True):
    """Random barycentric points of faces 0..nf-1, with their corners and edge points if ``edges``: (face [n] int64,
    bary [n,3] float64 weights of corners 0, 1, 2, uv [n,2] float64)."""
    rng = np.random.default_rng(seed)
    r = rng.random((nf, per_face, 2))
    flip = r.sum(axis=2) > 1
    r[flip] = 1 - r[flip]
    if edges:
        t = rng.random((nf, 3, 1))
        fixed = np.array([[0, 0], [1, 0], [0, 1]], np.float64)[None].repeat(nf, 0)
        on = np.concatenate([np.concatenate([t[:, 0:1], np.zeros_like(t[:, 0:1])], 2),
                             np.concatenate([np.zeros_like(t[:, 1:2]), t[:, 1:2]], 2),
                             np.concatenate([t[:, 2:3], 1 - t[:, 2:3]], 2)], axis=1)
        r = np.concatenate([r, fixed, on], axis=1)
    face = np.repeat(np.arange(nf, dtype=np.int64), r.shape[1])
    st = r.reshape(-1, 2)
    bary = np.stack([1 - st[:, 0] - st[:, 1], st[:, 0], st[:, 1]], axis=1)
    uvs = corner_uvs(nf, size, cell).astype(np.float64)[face]  # [n,3,2]
    return face, bary, (uvs * bary[:, :, None]).sum(axis=1)
