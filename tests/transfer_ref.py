"""The numpy restatement of mp_volume_bits, mp_mesh_transfer, mp_mesh_transfer_shade and mp_picture_light_transfer
(include/monoport_hip.h).  Every operation is one float32 operation on float32 arrays, in the header's order.  The
tracer visits EVERY sample j = 0..J-1 of every ray and knows nothing of blocks or skipping."""
import math

import numpy as np

import light_ref

F = np.float32


def bits_words(r):
    """(words of occupancy bits, words of the whole buffer) at resolution r."""
    nb = (r + 7) // 8
    fine = r * r * ((r + 31) // 32)
    return fine, fine + (nb ** 3 + 31) // 32


def volume_bits(vol, level):
    """uint32 [R * R * ceil(R/32)]: bit x & 31 of word (z*R + y)*WX + (x >> 5) set iff v > level (a NaN: not)."""
    vol = np.asarray(vol, F)
    r = vol.shape[0]
    wx = (r + 31) // 32
    with np.errstate(invalid="ignore"):
        occ = vol > F(level)
    out = np.zeros((r, r, wx), np.uint32)
    for x in range(r):
        out[:, :, x >> 5] |= occ[:, :, x].astype(np.uint32) << np.uint32(x & 31)
    return out.reshape(-1)


def occupancy(vol, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(vol, F) > F(level)


def tables(n_dirs):
    """(dirs f32 [D,3], basis f32 [D,9], weight) of recon.Transfer, from the issue's formulae in float64."""
    d = np.arange(n_dirs, dtype=np.float64)
    z = 1.0 - (2.0 * d + 1.0) / n_dirs
    phi = d * math.pi * (3.0 - math.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    x, y = s * np.cos(phi), s * np.sin(phi)
    pi = math.pi
    basis = np.stack([np.full(n_dirs, math.sqrt(1 / (4 * pi))),
                      math.sqrt(3 / (4 * pi)) * y, math.sqrt(3 / (4 * pi)) * z, math.sqrt(3 / (4 * pi)) * x,
                      math.sqrt(15 / (4 * pi)) * x * y, math.sqrt(15 / (4 * pi)) * y * z,
                      math.sqrt(5 / (16 * pi)) * (3 * z * z - 1), math.sqrt(15 / (4 * pi)) * z * x,
                      math.sqrt(15 / (16 * pi)) * (x * x - y * y)], 1)
    return np.stack([x, y, z], 1).astype(F), basis.astype(F), F(4 * pi / n_dirs)


def rays(r, b_min, b_max, bias=1.5, step=1.0, reach=None):
    """(bias_w, step_w, J) of recon.Transfer.rays: voxels times the smallest voxel edge, rounded to f32."""
    edge = float(np.min(np.asarray(b_max, np.float64) - np.asarray(b_min, np.float64))) / r
    j = math.ceil(math.sqrt(3.0) * r / step) + 2 if reach is None else math.ceil(reach / step)
    return F(bias * edge), F(step * edge), max(1, int(j))


def transfer(verts, normals, occ, b_min, b_max, dirs, basis, weight, bias_w, step_w, max_steps):
    """verts, normals f32 [V,3]; occ bool [R,R,R] (z, y, x) -> (mask uint64 [V, D/64], prt f32 [V,9], samples): the
    last is the number of samples the definition visits (what a tracer without skipping costs)."""
    verts = np.ascontiguousarray(verts, F).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, F).reshape(-1, 3)
    dirs, basis = np.asarray(dirs, F), np.asarray(basis, F)
    nv, nd, r = verts.shape[0], dirs.shape[0], occ.shape[0]
    rf = F(r)
    lo, hi = np.asarray(b_min, F), np.asarray(b_max, F)
    weight, bias_w, step_w = F(weight), F(bias_w), F(step_w)
    samples = 0
    with np.errstate(all="ignore"):
        u = light_ref.normalise(normals)
        length = hi - lo
        vox = rf / length
        g = ((verts - lo) / length) * rf
        o = g + (bias_w * u) * vox  # [V,3]
        kd = (dirs[None, :, 0] * u[:, None, 0] + dirs[None, :, 1] * u[:, None, 1]) + dirs[None, :, 2] * u[:, None, 2]
        traced = kd > 0  # [V,D]
        delta = (step_w * dirs) * vox  # [D,3]
        seen = np.zeros((nv, nd), bool)
        vi, di = np.nonzero(traced)  # the rays still under way
        for j in range(max_steps):
            if vi.size == 0:
                break
            samples += vi.size
            s = o[vi] + (F(j) * delta[di])  # [n,3] (x, y, z)
            inside = ((s >= 0) & (s < rf)).all(1)
            seen[vi[~inside], di[~inside]] = True
            vi, di, s = vi[inside], di[inside], s[inside]
            c = np.floor(s).astype(np.int64)
            hit = occ[c[:, 2], c[:, 1], c[:, 0]]
            vi, di = vi[~hit], di[~hit]
        seen[vi, di] = True  # used up J samples: unoccluded
        mask = np.zeros((nv, nd // 64), np.uint64)
        for d in range(nd):
            mask[:, d >> 6] |= seen[:, d].astype(np.uint64) << np.uint64(d & 63)
        acc = np.zeros((nv, 9), F)
        for d in range(nd):
            term = kd[:, d, None] * basis[d][None, :]
            acc = acc + np.where(seen[:, d, None], term, F(0))  # acc is never -0.0: adding +0.0 changes no bit
        prt = acc * weight
    return mask, prt, samples


def shade(prt, sh):
    """t [V,3]: t_c = 0, then + prt_k * sh[k][c] for k ascending."""
    prt = np.asarray(prt, F)
    sh = np.asarray(sh, F).reshape(9, 3)
    t = np.zeros((prt.shape[0], 3), F)
    with np.errstate(all="ignore"):
        for k in range(9):
            for c in range(3):
                t[:, c] = t[:, c] + prt[:, k] * sh[k, c]
    return t


def light_transfer(ambient, normal, face_id, albedo, direct_dir=None, direct_rgb=None, gamma=1.0, visibility=None,
                   albedo_rgb=None, background=1.0, dtype=np.float32):
    """mp_picture_light_transfer: light_ref.light with step 4 replaced by res = ambient.  normal may be None without
    a direct term.  -> (image [L,3], shading [L,3])."""
    amb = np.ascontiguousarray(ambient, F).reshape(-1, 3)
    face = np.asarray(face_id, np.int32).reshape(-1)
    npix = face.shape[0]
    cov = np.flatnonzero(face >= 0)
    shading = np.zeros((npix, 3), dtype)
    if albedo is None:
        image = np.full((npix, 3), F(background), dtype)
        alb = np.broadcast_to(np.asarray(albedo_rgb, F), (cov.shape[0], 3))
    else:
        image = np.ascontiguousarray(albedo, F).reshape(-1, 3).astype(dtype)
        alb = np.ascontiguousarray(albedo, F).reshape(-1, 3)[cov]
    t = dtype
    with np.errstate(all="ignore"):
        res = amb[cov].astype(dtype)
        rgb = np.zeros(3, F) if direct_rgb is None else np.asarray(direct_rgb, F)
        if (rgb != 0).any():
            u = light_ref.normalise(np.ascontiguousarray(normal, F).reshape(-1, 3)[cov].astype(dtype))
            d = np.asarray(direct_dir, F).astype(dtype)
            k = light_ref.max0(-((d[0] * u[:, 0] + d[1] * u[:, 1]) + d[2] * u[:, 2]))
            vis = t(1) if visibility is None else t(1) - np.asarray(visibility, F).reshape(-1)[cov].astype(dtype)
            kv = k * vis
            res = res.copy()
            for c in range(3):
                res[:, c] = res[:, c] + kv * rgb[c].astype(dtype)
        gamma = F(gamma)
        if gamma != F(1):
            res = np.power(light_ref.max0(res), (F(1) / gamma).astype(dtype))
        v = alb.astype(dtype) * res
        image[cov] = np.where(v < t(0), t(0), np.where(v > t(1), t(1), v))
    shading[cov] = res
    return image, shading


# ---- the volumes of the tests -----------------------------------------------------------------------------------------
def sphere_with_blob(r):
    """A ball in the lower middle with a smaller blob hovering over it (z up = the first index)."""
    z, y, x = np.meshgrid(*[(np.arange(r) + 0.5) / r * 2 - 1] * 3, indexing="ij")
    ball = 0.55 - np.sqrt(x * x + y * y + (z + 0.2) ** 2)
    blob = 0.22 - np.sqrt((x - 0.1) ** 2 + (y + 0.05) ** 2 + (z - 0.68) ** 2)
    return (0.5 + 2.0 * np.maximum(ball, blob)).astype(F)


def corner(r, thick=4):
    """A floor slab (low z) meeting a wall slab (low x): occupancy 1 inside, 0 outside."""
    vol = np.zeros((r, r, r), F)
    vol[:thick, :, :] = 1
    vol[:, :, :thick] = 1
    return vol
