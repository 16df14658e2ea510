"""numpy restatement of the CLIPPED mesh rasteriser's definition (include/monoport_hip.h, mp_mesh_render_clip; DESIGN.md
4.8.3): near-plane clipping of perspective cameras and perspective-correct interpolation, on top of the functions of
tests/mesh_render_ref.py.

It starts from CAMERA-SPACE coordinates (the rows of [R|t] p before the divide: what mp_orthogonal returns for the
camera's calibration) and performs every step with the operations and in the order the header gives.  A Python loop
over the faces, vectorised over each sub-triangle's box of pixel centres."""
import collections

import numpy as np

import mesh_render_ref as ref

F32 = np.float32

Clipped = collections.namedtuple("Clipped", ["image", "depth", "face", "cover", "kind", "both"])
Clipped.__doc__ = """image [H,W,3] f32 or None, depth [H,W] f32, face [H,W] int32, cover [H,W] int64 = the number of
sub-triangles that cover each pixel centre (before any depth test), kind [F] = inside vertices of each face (0..3; -1
for a face skipped for an index out of range or a non-finite camera coordinate), both [H,W] int64 = the number of
faces BOTH of whose sub-triangles cover the centre."""

# a vertex of a sub-triangle: (X, Y, z, inside vertex, outside vertex or -1, t)
Vert = collections.namedtuple("Vert", ["x", "y", "z", "i", "o", "t"])
Tri = collections.namedtuple("Tri", ["v", "area2", "box"])


def project(cam):
    """Camera-space [N,3] f32 -> the perspective projection (xc / zc, yc / zc, zc), two IEEE divisions."""
    cam = np.asarray(cam, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([cam[:, 0] / cam[:, 2], cam[:, 1] / cam[:, 2], cam[:, 2]], 1)


def _cut(cam, i, o, near, h, w):
    """cut(I, O) from the inside vertex i to the outside vertex o, or None if it fails the snap guard."""
    with np.errstate(all="ignore"):
        t = (near - cam[i, 2]) / (cam[o, 2] - cam[i, 2])
        xc = cam[i, 0] + t * (cam[o, 0] - cam[i, 0])
        yc = cam[i, 1] + t * (cam[o, 1] - cam[i, 1])
        X, Y, _, valid = ref.snap(np.array([[xc / near, yc / near, near]], np.float32), h, w)
    if not valid[0]:
        return None
    return Vert(int(X[0]), int(Y[0]), near, i, o, F32(t))


def _tri(a, b, c, h, w):
    """Step 3's area2, orientation exchange and clamped box of one sub-triangle; None for zero area."""
    area2 = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x)
    if area2 == 0:
        return None
    if area2 < 0:
        b, c, area2 = c, b, -area2
    xs, ys = (a.x, b.x, c.x), (a.y, b.y, c.y)
    i0, i1 = max((min(xs) - 128 + 255) >> 8, 0), min((max(xs) - 128) >> 8, h - 1)
    j0, j1 = max((min(ys) - 128 + 255) >> 8, 0), min((max(ys) - 128) >> 8, w - 1)
    return Tri((a, b, c), area2, (i0, i1, j0, j1))


def clip_verts(face, cam, X, Y, z, valid, near, h, w):
    """(kind, vertices) of one face: [A, B, C] (kind 3), [A, P, Q] (kind 1), [A, B, P, Q] (kind 2), or None where the
    definition skips the face whole."""
    idx = [int(k) for k in face]
    if any(k < 0 or k >= len(cam) for k in idx) or not np.isfinite(cam[idx]).all():
        return -1, None
    inside = [bool(cam[k, 2] >= near) for k in idx]
    kind = sum(inside)
    if kind == 0:
        return kind, None

    def own(k):
        return Vert(int(X[k]), int(Y[k]), z[k], k, -1, F32(0)) if valid[k] else None

    if kind == 3:
        v = [own(k) for k in idx]
    else:  # one inside: it comes first; two inside: the outside one comes last
        r = inside.index(True) if kind == 1 else (inside.index(False) + 1) % 3
        A, B, C = idx[r], idx[(r + 1) % 3], idx[(r + 2) % 3]
        if kind == 1:
            v = [own(A), _cut(cam, A, B, near, h, w), _cut(cam, A, C, near, h, w)]
        else:
            v = [own(A), own(B), _cut(cam, B, C, near, h, w), _cut(cam, A, C, near, h, w)]
    return kind, (None if any(k is None for k in v) else v)


def clip_face(face, cam, X, Y, z, valid, near, h, w):
    """(kind, [sub-triangle 0 or None, sub-triangle 1 or None]) of one face."""
    kind, v = clip_verts(face, cam, X, Y, z, valid, near, h, w)
    if v is None:
        return kind, [None, None]
    if len(v) == 3:
        return kind, [_tri(v[0], v[1], v[2], h, w), None]
    return kind, [_tri(v[0], v[1], v[2], h, w), _tri(v[0], v[2], v[3], h, w)]


def cut_segments(cam, faces, h, w, near):
    """The snapped cut segments (P, Q) of every face the plane cuts and the definition does not skip: the border of
    what is drawn of a closed mesh."""
    cam = np.asarray(cam, np.float32).reshape(-1, 3)
    X, Y, z, valid = ref.snap(project(cam), h, w)
    out = []
    for face in np.asarray(faces).reshape(-1, 3):
        kind, v = clip_verts(face, cam, X, Y, z, valid, F32(near), h, w)
        if v is not None and kind in (1, 2):
            out.append((v[-2], v[-1]))
    return out


def covered(tri, h, w):
    """[H,W] bool: the pixel centres a sub-triangle (``_tri``) covers."""
    out = np.zeros((h, w), bool)
    if tri is not None:
        px = (256 * np.arange(h, dtype=np.int64) + 128)[:, None]
        py = (256 * np.arange(w, dtype=np.int64) + 128)[None, :]
        out |= _fragments(tri, px, py, False)[0]
    return out


def _fragments(tri, px, py, pc):
    """Coverage, the factors q_k, the divisor s (None without ``pc``) and the depth at the centres (px, py)."""
    a, b, c = tri.v
    e0, c0 = ref._edge(b.x, b.y, c.x, c.y, px, py)
    e1, c1 = ref._edge(c.x, c.y, a.x, a.y, px, py)
    e2, c2 = ref._edge(a.x, a.y, b.x, b.y, px, py)
    area = F32(tri.area2)
    with np.errstate(all="ignore"):
        q = [e.astype(np.float32) / area for e in (e0, e1, e2)]
        if not pc:
            return c0 & c1 & c2, q, None, (q[0] * a.z + q[1] * b.z) + q[2] * c.z
        q = [q[0] / a.z, q[1] / b.z, q[2] / c.z]
        s = (q[0] + q[1]) + q[2]
        return c0 & c1 & c2, q, s, F32(1.0) / s


def _value(attr, v, c):
    with np.errstate(all="ignore"):
        return attr[v.i, c] if v.o < 0 else attr[v.i, c] + v.t * (attr[v.o, c] - attr[v.i, c])


def render(cam, faces, h, w, near, perspective_correct=False, attr=None, channel_major=False, nearest="min",
           scale=1.0, bias=0.0, lo=-np.inf, hi=np.inf, background=1.0):
    """The clipped definition on camera-space ``cam`` [N,3] and ``faces`` [F,3]; ``attr`` [N,3] ([3,N] with
    ``channel_major``) or None; ``nearest`` "max" or "min".  Returns a ``Clipped``."""
    cam = np.asarray(cam, np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    near = F32(near)
    X, Y, z, valid = ref.snap(project(cam), h, w)
    keys = np.zeros((h, w), np.uint64)
    cover = np.zeros((h, w), np.int64)
    both = np.zeros((h, w), np.int64)
    kinds = np.zeros(len(faces), np.int64)
    for f, face in enumerate(faces):
        kinds[f], subs = clip_face(face, cam, X, Y, z, valid, near, h, w)
        seen = np.zeros((h, w), np.int64) if subs[1] is not None else None
        for tri in subs:
            if tri is None:
                continue
            i0, i1, j0, j1 = tri.box
            if i0 > i1 or j0 > j1:
                continue
            px = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[:, None]
            py = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[None, :]
            cov, _, _, depth = _fragments(tri, px, py, perspective_correct)
            cover[i0:i1 + 1, j0:j1 + 1] += cov
            if seen is not None:
                seen[i0:i1 + 1, j0:j1 + 1] += cov
            d = -depth if nearest == "min" else depth
            key = (ref.orderable(d.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - f)
            key = np.where(cov & np.isfinite(depth), key, np.uint64(0))
            keys[i0:i1 + 1, j0:j1 + 1] = np.maximum(keys[i0:i1 + 1, j0:j1 + 1], key)
        if seen is not None:
            both += seen > 1
    hit = keys != 0
    face_id = np.where(hit, 0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth_out = np.zeros((h, w), np.float32)
    image = None
    if attr is not None:
        attr = np.asarray(attr, np.float32)
        attr = attr.T if channel_major else attr
        image = np.full((h, w, 3), F32(background), np.float32)
    for f in np.unique(face_id[hit]):
        _, subs = clip_face(faces[f], cam, X, Y, z, valid, near, h, w)
        todo = face_id == f
        for tri in subs:  # the lowest-numbered sub-triangle that covers the centre
            if tri is None or not todo.any():
                continue
            ii, jj = np.nonzero(todo)
            cov, q, s, depth = _fragments(tri, 256 * ii.astype(np.int64) + 128, 256 * jj.astype(np.int64) + 128,
                                          perspective_correct)
            ii, jj, depth, q = ii[cov], jj[cov], depth[cov], [k[cov] for k in q]
            todo[ii, jj] = False
            depth_out[ii, jj] = depth
            if image is None:
                continue
            with np.errstate(all="ignore"):
                for c in range(3):
                    a = [_value(attr, v, c) for v in tri.v]
                    o = (q[0] * a[0] + q[1] * a[1]) + q[2] * a[2]
                    if perspective_correct:
                        o = o / s[cov]
                    o = o * F32(scale) + F32(bias)
                    image[ii, jj, c] = np.where(o < F32(lo), F32(lo), np.where(o > F32(hi), F32(hi), o))
        # a centre no sub-triangle covers cannot hold the face's key; the device writes background there
        ii, jj = np.nonzero(todo)
        face_id[ii, jj] = -1
    return Clipped(image, depth_out, face_id, cover, kinds, both)
