"""The numpy restatement of mp_picture_points / mp_picture_paint (include/monoport_hip.h): the covered pixels of a flat
picture as a counted point list in ascending pixel order, and the scatter of per-entry values back into the picture.
Everything is a copy of 32-bit patterns except paint's ``v * scale + bias`` and its clamp, which are single float32
operations here as they are on the device."""
import numpy as np


def points(face_id, position, capacity=None, points_out=None, pixels_out=None):
    """face_id: int32 with L elements (-1 = uncovered); position: float32 with 3 L elements ([L,3] flattened).
    -> (points [3,capacity] float32, pixels [capacity] int32, count int32[2] = (min(K, capacity), K)).  Columns at or
    beyond count[0] keep what ``points_out`` / ``pixels_out`` held (zeros in fresh ones)."""
    face = np.asarray(face_id, np.int32).reshape(-1)
    pos = np.ascontiguousarray(position, np.float32).reshape(-1, 3).view(np.uint32)
    assert pos.shape[0] == face.shape[0]
    capacity = face.shape[0] if capacity is None else int(capacity)
    covered = np.flatnonzero(face >= 0)  # ascending
    k_all = covered.shape[0]
    n = min(k_all, capacity)
    pts = np.zeros((3, capacity), np.float32) if points_out is None else points_out
    pix = np.zeros(capacity, np.int32) if pixels_out is None else pixels_out
    assert pts.shape == (3, capacity) and pts.dtype == np.float32 and pix.shape == (capacity,) and pix.dtype == np.int32
    pix[:n] = covered[:n]
    pts.view(np.uint32)[:, :n] = pos[covered[:n]].T
    return pts, pix, np.array([n, k_all], np.int32)


def paint(values, pixels, count, image, scale=0.5, bias=0.5, lo=-np.inf, hi=np.inf):
    """values [3,capacity] float32, pixels [capacity] int32, count: count[0] entries are painted (clamped to
    [0, capacity]); image: float32 with 3 L elements, modified IN PLACE (it may be the array the positions came from)
    and returned.  An entry whose pixel lies outside [0, L) is skipped."""
    values = np.asarray(values, np.float32)
    capacity = values.shape[1]
    assert image.dtype == np.float32 and image.flags.c_contiguous  # reshape is then a view of the caller's image
    flat = image.reshape(-1, 3)
    n = min(max(int(np.asarray(count).reshape(-1)[0]), 0), capacity)
    scale, bias, lo, hi = (np.float32(v) for v in (scale, bias, lo, hi))
    p = np.asarray(pixels, np.int32)[:n].astype(np.int64)
    ok = (p >= 0) & (p < flat.shape[0])
    o = values[:, :n][:, ok] * scale + bias  # float32 arrays: one rounding per operation
    o = np.where(o < lo, lo, np.where(o > hi, hi, o)).astype(np.float32)
    flat[p[ok]] = o.T  # a list of points() names no pixel twice
    return image
