"""numpy restatement of the mesh rasteriser's definition (include/monoport_hip.h, mp_mesh_render).

It starts from PROJECTED coordinates (step 1 of the definition is mp_orthogonal / mp_perspective, which have their own
parity tests) and performs steps 2-5 with the operations and in the order the header gives: f32 snapping to 1/256
pixel, int64 coverage with a top-left rule, f32 screen-space barycentrics without FMA, one 64-bit key maximum per
fragment.  A Python loop over the faces, vectorised over each face's box of pixel centres."""
import collections

import numpy as np

GUARD = np.float32(2.0 ** 22)
F32 = np.float32

Rendered = collections.namedtuple("Rendered", ["image", "depth", "face", "cover"])
Rendered.__doc__ = """image [H,W,3] f32 or None, depth [H,W] f32, face [H,W] int32, cover [H,W] int64 = the number of
faces that cover each pixel centre (before any depth test)."""


def orderable(bits):
    """uint32 bits of a float -> a uint32 that orders as the float does (-0 below +0)."""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def snap(xyz, h, w):
    """Projected xyz [N,3] f32 -> (X int64 [N], Y int64 [N], z f32 [N], valid bool [N])."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = ((xyz[:, 0] + F32(1.0)) * (F32(0.5) * F32(h))) * F32(256.0)
        v = ((xyz[:, 1] + F32(1.0)) * (F32(0.5) * F32(w))) * F32(256.0)
        z = xyz[:, 2]
        valid = np.isfinite(u) & np.isfinite(v) & np.isfinite(z)
        valid &= ~(np.abs(u) > GUARD) & ~(np.abs(v) > GUARD)
        X = np.rint(np.where(valid, u, F32(0))).astype(np.int64)
        Y = np.rint(np.where(valid, v, F32(0))).astype(np.int64)
    return X, Y, z, valid


def _prepare(face, X, Y, valid, h, w):
    """A face's (idx[3], area2, box) after the orientation fix, or None where the definition skips it."""
    idx = [int(k) for k in face]
    if any(k < 0 or k >= len(X) for k in idx) or not all(valid[k] for k in idx):
        return None
    x = [int(X[k]) for k in idx]
    y = [int(Y[k]) for k in idx]
    area2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if area2 == 0:
        return None
    if area2 < 0:
        idx[1], idx[2] = idx[2], idx[1]
        area2 = -area2
    # pixel i has its centre at 256 i + 128 (Python's >> floors)
    i0, i1 = max((min(x) - 128 + 255) >> 8, 0), min((max(x) - 128) >> 8, h - 1)
    j0, j1 = max((min(y) - 128 + 255) >> 8, 0), min((max(y) - 128) >> 8, w - 1)
    return idx, area2, (i0, i1, j0, j1)


def _edge(ax, ay, bx, by, px, py):
    dx, dy = bx - ax, by - ay
    e = dx * (py - ay) - dy * (px - ax)
    return e, (e > 0) | ((e == 0) & (dy < 0 or (dy == 0 and dx > 0)))


def _fragments(idx, area2, px, py, X, Y, z):
    """Coverage and, per pixel centre (px, py int64 arrays), the weights and depth of face ``idx``."""
    x = [int(X[k]) for k in idx]
    y = [int(Y[k]) for k in idx]
    e0, c0 = _edge(x[1], y[1], x[2], y[2], px, py)
    e1, c1 = _edge(x[2], y[2], x[0], y[0], px, py)
    e2, c2 = _edge(x[0], y[0], x[1], y[1], px, py)
    a = F32(area2)
    with np.errstate(all="ignore"):
        w = [e.astype(np.float32) / a for e in (e0, e1, e2)]
        depth = (w[0] * z[idx[0]] + w[1] * z[idx[1]]) + w[2] * z[idx[2]]
    return c0 & c1 & c2, w, depth


def render(xyz, faces, h, w, attr=None, channel_major=False, nearest="max", scale=1.0, bias=0.0, lo=-np.inf,
           hi=np.inf, background=1.0):
    """Steps 2-5 of the definition on projected ``xyz`` [N,3] and ``faces`` [F,3]; ``attr`` [N,3] ([3,N] with
    ``channel_major``) or None; ``nearest`` "max" or "min".  Returns a ``Rendered``."""
    faces = np.asarray(faces).reshape(-1, 3)
    X, Y, z, valid = snap(xyz, h, w)
    keys = np.zeros((h, w), np.uint64)
    cover = np.zeros((h, w), np.int64)
    for f, face in enumerate(faces):
        prep = _prepare(face, X, Y, valid, h, w)
        if prep is None:
            continue
        idx, area2, (i0, i1, j0, j1) = prep
        if i0 > i1 or j0 > j1:
            continue
        px = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[:, None]
        py = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[None, :]
        cov, _, depth = _fragments(idx, area2, px, py, X, Y, z)
        cover[i0:i1 + 1, j0:j1 + 1] += cov
        d = -depth if nearest == "min" else depth
        key = (orderable(d.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - f)
        key = np.where(cov & np.isfinite(depth), key, np.uint64(0))
        keys[i0:i1 + 1, j0:j1 + 1] = np.maximum(keys[i0:i1 + 1, j0:j1 + 1], key)
    hit = keys != 0
    face_id = np.where(hit, 0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth_out = np.zeros((h, w), np.float32)
    image = None
    if attr is not None:
        attr = np.asarray(attr, np.float32)
        attr = attr.T if channel_major else attr
        image = np.full((h, w, 3), F32(background), np.float32)
    for f in np.unique(face_id[hit]):
        idx, area2, _ = _prepare(faces[f], X, Y, valid, h, w)
        ii, jj = np.nonzero(face_id == f)
        _, wt, depth = _fragments(idx, area2, 256 * ii.astype(np.int64) + 128, 256 * jj.astype(np.int64) + 128, X, Y, z)
        depth_out[ii, jj] = depth
        if image is not None:
            with np.errstate(all="ignore"):
                for c in range(3):
                    a = (wt[0] * attr[idx[0], c] + wt[1] * attr[idx[1], c]) + wt[2] * attr[idx[2], c]
                    o = a * F32(scale) + F32(bias)
                    image[ii, jj, c] = np.where(o < F32(lo), F32(lo), np.where(o > F32(hi), F32(hi), o))
    return Rendered(image, depth_out, face_id, cover)


def to_ndc(pix, h, w):
    """Pixel-grid coordinates (1.0 = one pixel, pixel i's centre at i + 0.5) of a hand-made test shape -> the projected
    coordinates that snap to them exactly: pix [N,2] or [N,3] (z passes through) -> [N,3] f32.  Exact for coordinates
    that are multiples of 1/256 on images whose sizes are powers of two or small."""
    pix = np.asarray(pix, np.float64)
    out = np.zeros((len(pix), 3), np.float64)
    out[:, 0] = pix[:, 0] * 2.0 / h - 1.0
    out[:, 1] = pix[:, 1] * 2.0 / w - 1.0
    if pix.shape[1] > 2:
        out[:, 2] = pix[:, 2]
    return out.astype(np.float32)
