"""The numpy restatement of mp_picture_light (include/monoport_hip.h): second-order spherical harmonics and one
directional light at the normal of every covered pixel, a gamma, and clamp(albedo * shading, 0, 1).  Every operation is
one float32 operation on float32 arrays, in the header's order; ``dtype=np.float64`` evaluates the same formulae in
float64 from the same float32 inputs (what the gamma test compares powf against)."""
import numpy as np

C1, C2, C3, C4, C5 = 0.429043, 0.511664, 0.743125, 0.886227, 0.247708


def max0(a):
    """a where a > 0, else +0.0 (a NaN, a -0.0: +0.0)."""
    return np.where(a > 0, a, a.dtype.type(0))


def normalise(v):
    """[N,3] -> v / |v| per row, (0, 0, 0) where |v|^2 is not finite or not > 0."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        s = (x * x + y * y) + z * z
        ok = np.isfinite(s) & (s > 0)
        length = np.sqrt(np.where(ok, s, s.dtype.type(1)))
        out = np.stack([x / length, y / length, z / length], 1)
    out[~ok] = 0
    return out.astype(v.dtype)


def basis(m):
    """The nine basis values H[0..8] at the unit normals m [N,3], as a list of [N] arrays."""
    t = m.dtype.type
    c1, c2, c3, c4, c5 = (t(np.float32(c)) for c in (C1, C2, C3, C4, C5))
    d1, d2 = t(2) * c1, t(2) * c2
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    return [np.full(mx.shape, c4, m.dtype), d2 * my, d2 * mz, d2 * mx, (d1 * mx) * my, (d1 * my) * mz,
            ((c3 * mz) * mz) - c5, (d1 * mz) * mx, c1 * ((mx * mx) - (my * my))]


def shade_normals(u, m, sh, direct_dir=None, direct_rgb=None, visibility=None, gamma=1.0):
    """Steps 4-6 on unit world normals u and SH normals m [N,3]: the shading [N,3]."""
    t = u.dtype.type
    sh = np.asarray(sh, np.float32).reshape(9, 3).astype(u.dtype)
    h = basis(m)
    res = np.zeros((u.shape[0], 3), u.dtype)
    for i in range(9):
        for c in range(3):
            res[:, c] = res[:, c] + h[i] * sh[i, c]
    rgb = np.zeros(3, np.float32) if direct_rgb is None else np.asarray(direct_rgb, np.float32)
    if (rgb != 0).any():
        d = np.asarray(direct_dir, np.float32).astype(u.dtype)
        k = max0(-((d[0] * u[:, 0] + d[1] * u[:, 1]) + d[2] * u[:, 2]))
        vis = t(1) if visibility is None else t(1) - np.asarray(visibility, np.float32).astype(u.dtype)
        kv = k * vis
        for c in range(3):
            res[:, c] = res[:, c] + kv * rgb[c].astype(u.dtype)
    gamma = np.float32(gamma)
    if gamma != np.float32(1):
        inv = (np.float32(1) / gamma).astype(u.dtype)  # one f32 division, as on the host side of the call
        res = np.power(max0(res), inv)
    return res


def light(normal, face_id, albedo, sh, direct_dir=None, direct_rgb=None, gamma=1.0, normal_mats=None, n_views=1,
          visibility=None, albedo_rgb=None, background=1.0, dtype=np.float32):
    """normal float32 [L,3] (any leading shape), face_id int32 [L], albedo float32 [L,3] or None with ``albedo_rgb``;
    normal_mats None or [n_views,3,3]; visibility None or [L].  -> (image [L,3], shading [L,3]) of ``dtype``; uncovered
    pixels of the image are the albedo's 32-bit patterns (``background`` without albedo), of the shading 0."""
    nrm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    face = np.asarray(face_id, np.int32).reshape(-1)
    npix = face.shape[0]
    assert nrm.shape[0] == npix and npix % n_views == 0
    cov = np.flatnonzero(face >= 0)
    shading = np.zeros((npix, 3), dtype)
    if albedo is None:
        image = np.full((npix, 3), np.float32(background), dtype)
        alb = np.broadcast_to(np.asarray(albedo_rgb, np.float32), (cov.shape[0], 3))
    else:
        image = np.ascontiguousarray(albedo, np.float32).reshape(-1, 3).astype(dtype)  # a copy: the bits, widened
        alb = np.ascontiguousarray(albedo, np.float32).reshape(-1, 3)[cov]
    with np.errstate(all="ignore"):
        u = normalise(nrm[cov].astype(dtype))
        m = u
        if normal_mats is not None:
            mats = np.asarray(normal_mats, np.float32).reshape(n_views, 3, 3).astype(dtype)[cov // (npix // n_views)]
            ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
            m = normalise(np.stack([(mats[:, r, 0] * ux + mats[:, r, 1] * uy) + mats[:, r, 2] * uz
                                    for r in range(3)], 1))
        res = shade_normals(u, m, sh, direct_dir, direct_rgb,
                            None if visibility is None else np.asarray(visibility, np.float32).reshape(-1)[cov], gamma)
        v = alb.astype(dtype) * res
        one, zero = dtype(1), dtype(0)
        image[cov] = np.where(v < zero, zero, np.where(v > one, one, v))
    shading[cov] = res
    return image, shading
