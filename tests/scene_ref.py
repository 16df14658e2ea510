"""The numpy restatement of mp_texture_mips / mp_picture_texture / mp_picture_composite (include/monoport_hip.h): the
mip pyramid of a texture, its lookup per pixel of a UV picture, and the composite of two pictures by coverage or by
depth.  Every float operation is a single float32 +, - or * on float32 arrays, in the header's order, as on the device;
there is no sqrt, log or division.  Everything else is integer work and copies of 32-bit patterns."""
import numpy as np

F = np.float32
UV_MOST = F(65536.0)
WRAP_REPEAT, WRAP_CLAMP = 0, 1
OVER, DEPTH = 0, 1
MAX_Z, MIN_Z = 0, 1  # MP_NEAREST_*


def max_levels(ht, wt):
    n, m = 1, max(ht, wt)
    while m > 1:
        n, m = n + 1, m >> 1
    return n


def level_sizes(ht, wt, levels):
    """[(h_l, w_l)] of levels 0..levels-1."""
    assert 1 <= ht <= 8192 and 1 <= wt <= 8192 and 1 <= levels <= min(14, max_levels(ht, wt))
    out = [(ht, wt)]
    for _ in range(levels - 1):
        h, w = out[-1]
        out.append((max(1, h >> 1), max(1, w >> 1)))
    return out


def level_offsets(ht, wt, levels):
    """The float offset of every level, and the float count of the pyramid as the last entry."""
    off = [0]
    for h, w in level_sizes(ht, wt, levels):
        off.append(off[-1] + 3 * h * w)
    return off


def pyramid_floats(ht, wt, levels):
    return level_offsets(ht, wt, levels)[-1]


def mips(tex, levels=None):
    """tex float32 [ht,wt,3] -> the levels as a list of [h_l,w_l,3] arrays (level 0: a copy)."""
    tex = np.ascontiguousarray(tex, F)
    ht, wt = tex.shape[:2]
    levels = max_levels(ht, wt) if levels is None else levels
    out = [tex.copy()]
    for h, w in level_sizes(ht, wt, levels)[1:]:
        src = out[-1]
        hs, ws = src.shape[:2]
        i0, i1 = np.minimum(2 * np.arange(h), hs - 1), np.minimum(2 * np.arange(h) + 1, hs - 1)
        j0, j1 = np.minimum(2 * np.arange(w), ws - 1), np.minimum(2 * np.arange(w) + 1, ws - 1)
        a, b = src[i0][:, j0], src[i0][:, j1]
        c, d = src[i1][:, j0], src[i1][:, j1]
        out.append(((a + b) + (c + d)) * F(0.25))
    return out


def pyramid(tex, levels=None):
    """The levels back to back, as mp_texture_mips writes them."""
    return np.concatenate([m.reshape(-1) for m in mips(tex, levels)])


def covered(uv, face):
    """uv [..., 3] float32, face [...] int32 -> bool [...]."""
    with np.errstate(invalid="ignore"):
        return (face >= 0) & (np.abs(uv[..., 0]) <= UV_MOST) & (np.abs(uv[..., 1]) <= UV_MOST)


def _axis_rho2(s, t, cov, axis):
    """The smaller d2 to the covered neighbours at +1 and -1 along ``axis`` of [V,H,W] arrays; 0 with none."""
    best = np.full(s.shape, -1.0, F)
    n = s.shape[axis]
    for step in (1, -1):
        here = [slice(None)] * 3
        there = [slice(None)] * 3
        here[axis] = slice(0, n - 1) if step == 1 else slice(1, n)
        there[axis] = slice(1, n) if step == 1 else slice(0, n - 1)
        here, there = tuple(here), tuple(there)
        with np.errstate(invalid="ignore", over="ignore"):
            ds, dt = s[there] - s[here], t[there] - t[here]
            d2 = (ds * ds) + (dt * dt)
        cur = best[here]
        take = cov[there] & ((cur < 0) | (d2 < cur))
        best[here] = np.where(take, d2, cur)
    return np.where(best < 0, F(0), best)


def select_level(uv, face, ht, wt, levels):
    """uv [V,H,W,3], face [V,H,W] -> (covered bool [V,H,W], level int [V,H,W] (0 where uncovered))."""
    uv = np.asarray(uv, F)
    cov = covered(uv, face)
    with np.errstate(invalid="ignore", over="ignore"):
        s, t = uv[..., 0] * F(wt), uv[..., 1] * F(ht)
    rho2 = np.maximum(_axis_rho2(s, t, cov, 1), _axis_rho2(s, t, cov, 2))
    level = np.zeros(rho2.shape, np.int64)
    for l in range(levels - 1):
        level += rho2 > F(2.0 ** (2 * l + 1))
    return cov, np.where(cov, level, 0)


def _wrap(k, n, wrap):
    return ((k % n) + n) % n if wrap == WRAP_REPEAT else np.clip(k, 0, n - 1)


def texture(uv, face, pyr, ht, wt, levels, wrap=WRAP_REPEAT, scale=1.0, bias=0.0, lo=-np.inf, hi=np.inf,
            background=1.0, return_level=False):
    """uv float32 [V,H,W,3], face int32 [V,H,W], pyr: the flat pyramid -> image float32 [V,H,W,3]."""
    uv = np.asarray(uv, F)
    face = np.asarray(face, np.int32)
    assert uv.ndim == 4 and uv.shape[:3] == face.shape
    cov, level = select_level(uv, face, ht, wt, levels)
    off, sizes = level_offsets(ht, wt, levels), level_sizes(ht, wt, levels)
    scale, bias, lo, hi = (F(v) for v in (scale, bias, lo, hi))
    image = np.full(uv.shape, F(background), F)
    for l, (h, w) in enumerate(sizes):
        pick = cov & (level == l)
        if not pick.any():
            continue
        tex = pyr[off[l]:off[l + 1]].reshape(h, w, 3)
        u, v = uv[pick][:, 0], uv[pick][:, 1]
        s, t = u * F(w) - F(0.5), v * F(h) - F(0.5)
        s0, t0 = np.floor(s), np.floor(t)
        fs, ft = (s - s0)[:, None], (t - t0)[:, None]
        x0, y0 = s0.astype(np.int64), t0.astype(np.int64)
        xa, xb = _wrap(x0, w, wrap), _wrap(x0 + 1, w, wrap)
        ya, yb = _wrap(y0, h, wrap), _wrap(y0 + 1, h, wrap)
        c00, c10, c01, c11 = tex[ya, xa], tex[ya, xb], tex[yb, xa], tex[yb, xb]
        gs, gt = F(1) - fs, F(1) - ft
        value = (c00 * gs + c10 * fs) * gt + (c01 * gs + c11 * fs) * ft
        o = value * scale + bias
        image[pick] = np.where(o < lo, lo, np.where(o > hi, hi, o)).astype(F)
    return (image, level) if return_level else image


def composite(front, back, mode=DEPTH, nearest=MAX_Z, background=1.0):
    """front, back: (image float32 [...,3], depth float32 [...], face int32 [...]) -> (image, depth, mask uint8)."""
    fi, fd, ff = (np.asarray(a) for a in front)
    bi, bd, bf = (np.asarray(a) for a in back)
    fc, bc = ff >= 0, bf >= 0
    with np.errstate(invalid="ignore"):
        back_nearer = (bd < fd) if nearest == MIN_Z else (bd > fd)
    shows_front = fc & (~bc | (mode == OVER) | ~back_nearer)
    shows_back = ~shows_front & bc
    image = np.full(fi.shape, F(background), F).view(np.uint32)
    depth = np.zeros(fd.shape, np.uint32)
    image[shows_front] = fi.astype(F, copy=False).view(np.uint32)[shows_front]
    image[shows_back] = bi.astype(F, copy=False).view(np.uint32)[shows_back]
    depth[shows_front] = fd.astype(F, copy=False).view(np.uint32)[shows_front]
    depth[shows_back] = bd.astype(F, copy=False).view(np.uint32)[shows_back]
    mask = np.where(shows_front, 2, np.where(shows_back, 1, 0)).astype(np.uint8)
    return image.view(F), depth.view(F), mask
