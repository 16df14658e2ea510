"""numpy restatement of mp_picture_resolve (include/monoport_hip.h): the final picture of one rendered at s times its
size.  Every step is written as the header writes it: explicit f32 additions in row-major sample order starting from the
first sample, one f32 division, the rasteriser's orderable key compared on bits, ties to the first sample."""
import numpy as np


def orderable(bits):
    """The rasteriser's key of a depth's bits (uint32): unsigned order = float order, -0 below +0."""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _planes(a, s, channels=False):
    """[..., s h, s w(, 3)] -> the s*s sample planes [..., h, w(, 3)] in row-major (a, b) order."""
    if channels:
        return [a[..., i::s, j::s, :] for i in range(s) for j in range(s)]
    return [a[..., i::s, j::s] for i in range(s) for j in range(s)]


def resolve(image, depth, face, mask, samples, nearest="max"):
    """(image_out, depth_out, face_out, mask_out, coverage) of pictures [..., s h, s w(, 3)]; an output whose input is
    None is None (image: image; depth and face: both depth and face; mask: mask; coverage: mask or face)."""
    s = int(samples)
    assert 2 <= s <= 4 and nearest in ("max", "min")
    image_out = depth_out = face_out = mask_out = coverage = None
    if image is not None:
        planes = _planes(np.asarray(image, np.float32), s, True)
        acc = planes[0].copy()
        with np.errstate(over="ignore", invalid="ignore"):
            for p in planes[1:]:
                acc = (acc + p).astype(np.float32)  # one f32 addition per sample
            image_out = (acc / np.float32(s * s)).astype(np.float32)
    masks = None if mask is None else _planes(np.asarray(mask, np.uint8), s)
    faces = None if face is None else _planes(np.asarray(face, np.int32), s)
    if masks is not None:
        subject, shows = [m == 2 for m in masks], [m != 0 for m in masks]
        mask_out = masks[0].copy()
        for m in masks[1:]:
            mask_out = np.maximum(mask_out, m)
    elif faces is not None:
        subject = shows = [f >= 0 for f in faces]
    if masks is not None or faces is not None:
        count = np.zeros(subject[0].shape, np.int32)
        for sub in subject:
            count += sub
        coverage = (count.astype(np.float32) / np.float32(s * s)).astype(np.float32)
    if depth is not None and face is not None:
        bits = _planes(np.ascontiguousarray(depth, np.float32).view(np.uint32), s)
        flip = np.uint32(0x80000000 if nearest == "min" else 0)
        found = np.zeros(bits[0].shape, bool)
        best_key = np.zeros(bits[0].shape, np.uint32)
        best_bits = np.zeros(bits[0].shape, np.uint32)  # +0.0
        face_out = np.full(bits[0].shape, -1, np.int32)
        for b, f, show in zip(bits, faces, shows):
            key = orderable(b ^ flip)
            take = show & (~found | (key > best_key))  # strictly nearer: a tie keeps the first
            best_key = np.where(take, key, best_key)
            best_bits = np.where(take, b, best_bits)
            face_out = np.where(take, f, face_out)
            found |= show
        depth_out = best_bits.view(np.float32)
    return image_out, depth_out, face_out, mask_out, coverage


def same_bits(a, b):
    """Equal as bit patterns (floats: -0 != +0, equal NaNs equal), shapes and dtypes included."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))
