"""OBJ export of the marching-cubes mesh in the reference's on-disk format
(monoport/lib/mesh_util.py:223-242: ``v x y z [r g b]`` with %.4f, 1-based ``f i j k``), the per-vertex
normals of its ``compute_normal`` (:201-220), plus the per-vertex colour query of BASELINE configs[2]."""
import numpy as np
import torch

from . import ops


def _as_numpy(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def save_obj_mesh(mesh_path, verts, faces):
    """mesh_util.py:223-230."""
    v, f = _as_numpy(verts), _as_numpy(faces).astype(np.int64) + 1
    with open(mesh_path, "w") as fh:
        fh.write("".join("v %.4f %.4f %.4f\n" % tuple(row) for row in v))
        fh.write("".join("f %d %d %d\n" % tuple(row) for row in f))


def save_obj_mesh_with_color(mesh_path, verts, faces, colors):
    """mesh_util.py:233-242."""
    v, c = _as_numpy(verts), _as_numpy(colors)
    f = _as_numpy(faces).astype(np.int64) + 1
    with open(mesh_path, "w") as fh:
        fh.write("".join("v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (tuple(a) + tuple(b))
                         for a, b in zip(v, c)))
        fh.write("".join("f %d %d %d\n" % tuple(row) for row in f))


def save_obj_mesh_with_normals(mesh_path, verts, faces, normals, colors=None):
    """``v x y z [r g b]`` lines as the two writers above, one ``vn %.4f %.4f %.4f`` per vertex, then
    1-based ``f i//i j//j k//k``.  The reference has no such writer; it has the reader: the file loads with
    its ``load_obj_mesh(path, with_normal=True)`` (mesh_util.py:89-187), which renormalises the ``vn`` rows."""
    v, n = _as_numpy(verts), _as_numpy(normals)
    f = _as_numpy(faces).astype(np.int64) + 1
    with open(mesh_path, "w") as fh:
        if colors is None:
            fh.write("".join("v %.4f %.4f %.4f\n" % tuple(row) for row in v))
        else:
            fh.write("".join("v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (tuple(a) + tuple(b))
                             for a, b in zip(v, _as_numpy(colors))))
        fh.write("".join("vn %.4f %.4f %.4f\n" % tuple(row) for row in n))
        fh.write("".join("f %d//%d %d//%d %d//%d\n" % (i, i, j, j, k, k) for i, j, k in f))


def _normalize_v3(arr):
    """normalize_v3 (mesh_util.py:190-198), out of place: sqrt(x**2 + y**2 + z**2) left to right, lengths
    below 1e-8 replaced by 1e-8, three divisions -- in ``arr``'s dtype."""
    lens = np.sqrt(arr[:, 0] * arr[:, 0] + arr[:, 1] * arr[:, 1] + arr[:, 2] * arr[:, 2])
    eps = arr.dtype.type(1e-8)
    lens[lens < eps] = eps
    return arr / lens[:, None]


def _compute_normal_numpy(v, f, mode):
    """The two definitions of include/monoport_hip.h (MP_NORMALS_*) op by op in ``v``'s dtype."""
    t = v[f]
    a, b = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    n = np.empty_like(a)  # np.cross: multiply, multiply, subtract per component
    n[:, 0] = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    n[:, 1] = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    n[:, 2] = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    n = _normalize_v3(n)
    out = np.zeros_like(v)
    if mode == "reference":
        # norm[faces[:, c]] += n assigns, it does not accumulate: per corner the last face wins
        for c in range(3):
            last = np.full(len(v), -1, np.int64)
            np.maximum.at(last, f[:, c], np.arange(len(f)))
            m = last >= 0
            out[m] = out[m] + n[last[m]]
    else:
        # unbuffered, in ascending (face, corner) order
        np.add.at(out, f.reshape(-1), np.repeat(n, 3, axis=0))
    return _normalize_v3(out)


def compute_normal(vertices, faces, mode="reference"):
    """Per-vertex normals [V,3] of a triangle mesh: the drop-in for mesh_util.py:201-220.

    ``mode="reference"`` is what the reference computes, bit for bit: its fancy-index ``+=`` keeps, for each
    of the three corners, only the LAST face that has the vertex at that corner.  ``mode="accumulate"`` is what
    its comments describe: every incident face's unit normal, added in ascending (face, corner) order.
    float32 vertices on a HIP device run mp_mesh_normals (a face that names a vertex outside [0, V) is skipped
    there); numpy arrays, CPU tensors and other dtypes run the same two definitions in numpy, in the input's
    dtype.  Returns the kind it was given; the inputs are not modified."""
    if mode not in ops.NORMALS_MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(ops.NORMALS_MODES), mode))
    if torch.is_tensor(vertices) and vertices.is_cuda and vertices.dtype == torch.float32:
        v = vertices.detach().contiguous()
        f = torch.as_tensor(faces, device=v.device).to(torch.int32).contiguous() if not torch.is_tensor(faces) \
            else faces.detach().to(device=v.device, dtype=torch.int32).contiguous()
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError("vertices must be [V,3] and faces [F,3]")
        counts = torch.tensor([v.shape[0], f.shape[0]], dtype=torch.int32, device=v.device)
        return ops.mesh_normals_raw(v, f, counts, mode)
    v = _as_numpy(vertices)
    if not np.issubdtype(v.dtype, np.floating):
        v = v.astype(np.float64)
    f = _as_numpy(faces).astype(np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("vertices must be [V,3] and faces [F,3]")
    out = _compute_normal_numpy(v, f, mode)
    if torch.is_tensor(vertices):
        return torch.from_numpy(out).to(vertices.device)
    return out


@torch.no_grad()
def vertex_colors(netC, feat_tensor_C, verts, calib_tensor):
    """RGB in [0,1] for world-space vertices [V,3]: netC.query(...)*0.5+0.5 as RTL/main.py:239-244
    does for the visible-surface vertices."""
    pts = verts.t().contiguous()[None]  # [1,3,V]
    preds = netC.query(feat_tensor_C, points=pts, calibs=calib_tensor)[0]
    return (preds[0] * 0.5 + 0.5).t().contiguous()
