"""The numpy restatement of mp_picture_shadow (include/monoport_hip.h): the shadow a shadow map casts on a picture.
Step 2, the projection under the light, is the oracle's ``orthogonal`` (the op sequence of mp_orthogonal, pinned by
tests/test_oracle_golden.py) followed, for a perspective light, by the two IEEE divisions the render restatement uses
(mesh_render_clip_ref.project).  Every float operation of steps 3-6 is a single float32 +, - or * on float32 arrays, in
the header's order, as on the device; there is no sqrt, log or division.  Everything else is integer work, comparisons
and copies of 32-bit patterns."""
import numpy as np

import mesh_render_clip_ref as clip
from oracle import pifu_oracle as oracle

F = np.float32
MOST = F(2.0 ** 22)
MAX_Z, MIN_Z = 0, 1  # MP_NEAREST_*
ORTHOGONAL, PERSPECTIVE = 0, 1  # MP_PROJ_*
K = [F(1.0), F(1.0) / F(9.0), F(1.0) / F(25.0), F(1.0) / F(49.0)]  # the f32 nearest to 1 / (2r+1)^2


def project(points, calib, projection):
    """World-space points [N,3] f32 -> (x, y, z) [N,3] under the light: the bits of mp_orthogonal / mp_perspective; z
    is the camera-space row in both."""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    if points.shape[0] == 0:
        return np.zeros((0, 3), F)
    with np.errstate(all="ignore"):
        cam = oracle.orthogonal(np.ascontiguousarray(points.T), np.asarray(calib, F)).T
        return clip.project(cam) if projection == PERSPECTIVE else np.ascontiguousarray(cam)


def map_coordinates(xyz, hs, ws, projection):
    """Steps 2-3 on projected xyz [N,3]: (live bool [N], i0, j0 int64 [N], fa, fb f32 [N]); dead points hold zeros."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        live = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        if projection == PERSPECTIVE:
            live &= z > 0
        a = (x + F(1.0)) * (F(0.5) * F(hs)) - F(0.5)
        b = (y + F(1.0)) * (F(0.5) * F(ws)) - F(0.5)
        live &= ~(np.abs(a) > MOST) & ~(np.abs(b) > MOST)
        a, b = np.where(live, a, F(0)), np.where(live, b, F(0))
        af, bf = np.floor(a), np.floor(b)
        fa, fb = a - af, b - bf
    return live, af.astype(np.int64), bf.astype(np.int64), fa.astype(F), fb.astype(F)


def occluded(i, j, z, map_depth, map_face, nearest, bias):
    """Step 4: occ(i, j) as float32 1.0 / 0.0 for taps (i, j int64 [N]) against receivers of depth z f32 [N]."""
    hs, ws = map_depth.shape
    inside = (i >= 0) & (i < hs) & (j >= 0) & (j < ws)
    ic, jc = np.clip(i, 0, hs - 1), np.clip(j, 0, ws - 1)
    d = map_depth[ic, jc]
    with np.errstate(all="ignore"):
        nearer = (d + F(bias) < z) if nearest == MIN_Z else (d - F(bias) > z)
    return np.where(inside & (map_face[ic, jc] >= 0) & nearer, F(1.0), F(0.0)).astype(F)


def weights(f, radius):
    """Step 5's weights along one axis for fractions f f32 [N]: a list of 2 radius + 2 arrays, offsets -r..r+1."""
    one = np.ones_like(f)
    return [F(1.0) - f] + [one] * (2 * radius) + [f]


def shade(position, face, map_depth, map_face, calib, projection=ORTHOGONAL, nearest=MIN_Z, bias=0.0, radius=1):
    """position f32 [...,3], face int32 [...] -> shade f32 [...]."""
    position = np.asarray(position, F)
    face = np.asarray(face, np.int32)
    assert position.shape[:-1] == face.shape and position.shape[-1] == 3 and 0 <= radius <= 3
    map_depth, map_face = np.asarray(map_depth, F), np.asarray(map_face, np.int32)
    hs, ws = map_depth.shape
    out = np.zeros(face.size, F)
    covered = np.nonzero(face.reshape(-1) >= 0)[0]
    xyz = project(position.reshape(-1, 3)[covered], calib, projection)
    live, i0, j0, fa, fb = map_coordinates(xyz, hs, ws, projection)
    z = xyz[:, 2]
    wi, wj = weights(fa, radius), weights(fb, radius)
    total = np.zeros(len(covered), F)
    for a, di in enumerate(range(-radius, radius + 2)):
        row = np.zeros(len(covered), F)
        for b, dj in enumerate(range(-radius, radius + 2)):
            row = row + wj[b] * occluded(i0 + di, j0 + dj, z, map_depth, map_face, nearest, bias)
        total = total + wi[a] * row
    s = total * K[radius]
    s = np.where(s < F(1.0), s, F(1.0)).astype(F)
    out[covered] = np.where(live, s, F(0.0))
    return out.reshape(face.shape)


def paint(image, shade_, strength):
    """Step 6: image f32 [...,3], shade f32 [...] -> image_out; the input's bits wherever the shade is 0."""
    image = np.ascontiguousarray(image, F)
    factor = (F(1.0) - F(strength) * shade_)[..., None]
    with np.errstate(all="ignore"):
        dark = (image * factor).astype(F)
    return np.where((shade_ == 0)[..., None], image.view(np.uint32), dark.view(np.uint32)).view(F)


def shadow(image, position, face, map_depth, map_face, calib, projection=ORTHOGONAL, nearest=MIN_Z, bias=0.0, radius=1,
           strength=0.6):
    """(image_out or None for ``image`` None, shade)."""
    s = shade(position, face, map_depth, map_face, calib, projection, nearest, bias, radius)
    return (None if image is None else paint(image, s, strength)), s
