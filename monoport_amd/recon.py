"""Drop-ins for RTL/recon.py (``pifu_calib``, ``forward_vertices``) and for the colorization
closure of RTL/main.py:201-249, on top of the HIP kernels in csrc/vertices.hip."""
import collections
import math

import numpy as np
import torch

from . import ops
from .modeling.MonoPortNet import ViewsBinding, capture_query

_FLIP_Y = np.diag([1.0, -1.0, 1.0, 1.0])  # RTL/recon.py:6-11


@torch.no_grad()
def pifu_calib(extrinsic, intrinsic, device="cuda:0"):
    """Calibration tensor [1,4,4] f32 = inv(K' E' diag(1,-1,1,1)) with the orthographic tweaks
    K'[2,2]=K[0,0], K'[2,3]=0, E'[2,3]=0 (RTL/recon.py:4-25).  Host-side float64 numpy; inputs are
    not modified."""
    k = np.array(intrinsic, copy=True)
    k[2, 2] = k[0, 0]
    k[2, 3] = 0
    e = np.array(extrinsic, copy=True)
    e[2, 3] = 0
    calib = np.linalg.inv(k @ e @ _FLIP_Y)
    return torch.from_numpy(calib).unsqueeze(0).float().to(device)


@torch.no_grad()
def forward_vertices(sdf, direction="front"):
    """Visible-surface vertices of an occupancy volume [1,1,D,H,W] (RTL/recon.py:27-89):
    X, Y int64 [N], Z f32 [N] (sub-voxel depth), norm f32 [N,3]; four Nones for ``sdf is None``.
    One host sync (N), like the reference's ``nonzero``."""
    if sdf is None:
        return None, None, None, None
    x, y, z, n, count = ops.forward_vertices_raw(sdf, direction)
    c = int(count.item())
    return x[:c], y[:c], z[:c], n[:c]


@torch.no_grad()
def forward_vertices_many(sdfs, direction="front"):
    """``[forward_vertices(s, direction) for s in sdfs]`` with ONE host sync for all the vertex
    counts (monoport_amd extension; the hook of a coalescing stage, stage_pipeline.Coalesced)."""
    idx = [i for i, s in enumerate(sdfs) if s is not None]
    raws = [None] * len(sdfs)
    if idx and len({tuple(sdfs[i].shape[-3:]) for i in idx}) == 1:  # one size: one set of launches for all of them
        for i, r in zip(idx, ops.forward_vertices_raw_batch([sdfs[i] for i in idx], direction)):
            raws[i] = r
    else:
        for i in idx:
            raws[i] = ops.forward_vertices_raw(sdfs[i], direction)
    live = [r for r in raws if r is not None]
    counts = torch.cat([r[4] for r in live]).cpu().tolist() if live else []
    out, k = [], 0
    for r in raws:
        if r is None:
            out.append((None, None, None, None))
        else:
            c = int(counts[k])
            k += 1
            out.append((r[0][:c], r[1][:c], r[2][:c], r[3][:c]))
    return out


def color_matrix(b_min, b_max, resolution):
    """voxel -> world matrix of RTL/main.py:204-210."""
    mat = np.eye(4, dtype=np.float32)
    length = np.asarray(b_max, np.float32).reshape(3) - np.asarray(b_min, np.float32).reshape(3)
    for i in range(3):
        mat[i, i] = length[i] / np.float32(resolution)
    mat[0:3, 3] = np.asarray(b_min, np.float32).reshape(3)
    return mat


def _counted_colours(bindings, pts, counts, outs=None, view=0):
    """netC's predictions [3,cap] per frame at the first counts[f] of the points pts[f] [3,cap]: lists with one entry per
    frame, ``bindings`` of one head.  One orthogonal frame without buffers of the caller's (``outs``) is the per-frame
    counted launch; anything else the batched one per ops.MAX_FRAMES frames, with the projection modes if a frame is
    perspective.  ``ViewsBinding``s (a multi-view head; one ``batch_key``): row ``view`` of the head's [V,3,N] result,
    ops.query_views_counted_batch per ``ops.max_view_frames(V)`` frames."""
    n, preds = len(bindings), []
    if isinstance(bindings[0], ViewsBinding):
        b0 = bindings[0]
        key = b0.batch_key(view)
        if any(not isinstance(b, ViewsBinding) or b.batch_key(view) != key for b in bindings):
            raise ValueError("_counted_colours: the bindings differ in head, views, projection or map size")
        step = ops.max_view_frames(b0.num_views)
        for f0 in range(0, n, step):
            chunk = bindings[f0:f0 + step]
            preds += ops.query_views_counted_batch(b0.mlp, [b.maps for b in chunk], pts[f0:f0 + step],
                                                   counts[f0:f0 + step], [b.calibs for b in chunk], b0.projection,
                                                   b0.z_scale, view=view,
                                                   outs=None if outs is None else outs[f0:f0 + step])
        return preds
    for f0, f1 in ops._frame_chunks(n):
        chunk = bindings[f0:f1]
        b0 = chunk[0]
        ortho = all(b.projection == ops.PROJECTIONS["orthogonal"] for b in chunk)
        if n == 1 and ortho and outs is None:
            return [ops.query_counted(b0.mlp, b0.feat_hwc, pts[0], counts[0], b0.calib, b0.z_scale)]
        preds += ops.query_counted_batch(b0.mlp, [b.feat_hwc for b in chunk], pts[f0:f1], counts[f0:f1],
                                         [b.calib for b in chunk], b0.z_scale,
                                         outs=None if outs is None else outs[f0:f1],
                                         projections=None if ortho else [b.projection for b in chunk])
    return preds


def _check_colour_view(who, netC, view):
    """``view`` of the mesh calls against ``netC`` (None: no colours), before anything is bound or enqueued: None keeps
    the single-view path, an int asks for row ``view`` of a multi-view head."""
    if view is None or netC is None:
        if view is not None:
            raise ValueError("%s: view=%r picks a row of a multi-view netC, and there is no netC" % (who, view))
        return
    v_n = netC.surface_classifier.num_views
    if v_n <= 1:
        raise ValueError("%s: view=%r needs a multi-view netC; this one has num_views = %d" % (who, view, v_n))
    if isinstance(view, bool) or not isinstance(view, int) or not 0 <= view < v_n:
        raise ValueError("%s: view must be an int in 0..%d (netC has %d views), got %r" % (who, v_n - 1, v_n, view))


def _bind_netC(who, netC, frames, view=None):
    """The query bindings of ``netC``, one per frame of ``frames`` = (feature maps, calibration, device to query on);
    the maps are moved there first (main.py:229-230).  ``view`` None: a single-view head (a multi-view one is refused);
    an int (checked by ``_check_colour_view``): the ``ViewsBinding``s of a multi-view head, maps of batch V and
    calibrations [V,4,4] per frame."""
    if view is not None:
        return [netC.bind_views([[f.to(device) for f in fs] for fs in feats], calib) for feats, calib, device in frames]
    if netC.surface_classifier.num_views > 1:
        raise NotImplementedError("%s: netC has num_views = %d; colour the vertices of a multi-view head with "
                                  "mesh_util.vertex_colors, or pass view= to the mesh calls"
                                  % (who, netC.surface_classifier.num_views))
    return [netC.bind([[f.to(device) for f in fs] for fs in feats], calib) for feats, calib, device in frames]


@torch.no_grad()
def colorization(netC, feat_tensor_C, X, Y, Z, calib_tensor, norm=None, resolution=257,
                 mat_color=None):
    """[res,res,3] f32 render (RTL/main.py:212-249): normals as colour when ``norm`` is given,
    else netC.query on the vertices mapped to world space; ``None`` passes through (:214-215)."""
    if X is None:
        return None
    count = torch.tensor([X.shape[0]], dtype=torch.int32, device=X.device)
    if norm is not None:
        return ops.paint(X, Y, norm, 0, count, resolution, 0.5, 0.5, 0.0, 1.0)
    if mat_color is None:
        mat_color = color_matrix([-1, -1, -1], [1, 1, 1], resolution)
    if torch.is_tensor(mat_color):
        mat_color = mat_color.detach().cpu().numpy()
    device = calib_tensor.device
    feat_tensor_C = [[f.to(device) for f in feats] for feats in feat_tensor_C]  # main.py:229-230
    X, Y, Z = X.to(device), Y.to(device), Z.to(device)
    pts = ops.vertex_points(X, Y, Z.float(), count.to(device), resolution, mat_color)
    preds = _counted_colours([netC.bind(feat_tensor_C, calib_tensor)], [pts], [count.to(device)])[0]
    return ops.paint(X, Y, preds, 1, count.to(device), resolution, 0.5, 0.5, -np.inf, np.inf)


@torch.no_grad()
def marching_cubes(sdf, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1)):
    """Triangle mesh of an occupancy volume [1,1,D,H,W] (or [D,H,W]): (verts [V,3] f32 world
    coordinates, faces [F,3] int32), or (None, None) for ``sdf is None``.  Not part of the
    reference (it renders from the volume directly); the mesh output the north star asks for.
    One host sync (the two counts); retried once with exact capacities if the guess was short."""
    if sdf is None:
        return None, None
    verts, faces, counts = ops.marching_cubes_raw(sdf, level, b_min, b_max)
    nv, nf = (int(c) for c in counts.cpu())
    if nv > verts.shape[0] or nf > faces.shape[0]:
        verts, faces, counts = ops.marching_cubes_raw(sdf, level, b_min, b_max, max_verts=nv,
                                                      max_faces=nf)
    return verts[:nv], faces[:nf]


CLEAN_FILL = 0.0  # what ``clean`` puts into dropped voxels: below every level a sigmoid field is cut at


@torch.no_grad()
def keep_largest(sdf, level=0.5, connectivity=6, fill=0.0):
    """The occupancy volume [1,1,D,H,W] (or [D,H,W]) without its floating blobs: of the voxels > ``level`` only the
    largest connected body stays (``connectivity`` 6: face neighbours, 26: edges and corners too; of equally large
    bodies the one with the smallest linear index), every other such voxel becomes ``fill`` (<= level); all other
    voxels keep their bits.  Returns a new volume of the input's shape, None for ``sdf is None``.  On the device,
    nothing synchronised (``ops.keep_largest_raw`` also hands out the statistics).  Not part of the reference."""
    if sdf is None:
        return None
    return ops.keep_largest_raw(sdf, level, connectivity, fill)[0].reshape(sdf.shape)


@torch.no_grad()
def keep_largest_many(sdfs, level=0.5, connectivity=6, fill=0.0):
    """``[keep_largest(s, level, connectivity, fill) for s in sdfs]`` -- the same bits -- in one set of launches per
    ops.MAX_FRAMES volumes.  ``None`` entries give ``None``; the other volumes must be of one size (ValueError)."""
    sdfs = list(sdfs)
    idx = [i for i, s in enumerate(sdfs) if s is not None]
    out = [None] * len(sdfs)
    if idx:
        raws = ops.keep_largest_raw_batch([sdfs[i] for i in idx], level, connectivity, fill)
        for i, (vol, _) in zip(idx, raws):
            out[i] = vol.reshape(sdfs[i].shape)
    return out


Mesh = collections.namedtuple("Mesh", ["verts", "faces", "normals", "colors"])
Mesh.__doc__ = """Triangle mesh of ``reconstruct_mesh``: verts [V,3] f32 world coordinates, faces [F,3] int32,
normals [V,3] f32 or None, colors [V,3] f32 in [0,1] or None."""


SMOOTH_KEYS = ("iterations", "lam", "mu", "pin_border")
SMOOTH_DEFAULTS = {"iterations": 10, "lam": 0.5, "mu": -0.53, "pin_border": True}

MeshOptions = collections.namedtuple("MeshOptions", ["normals", "level", "colors", "clean", "simplify", "smooth"])
MeshOptions.__doc__ = """What a mesh chain is asked for, validated by ``mesh_options``: the normals mode or None, the
iso-level, whether netC colours the vertices, and per optional stage None (nothing allocated or enqueued for it) or its
setting: ``clean`` the connectivity of ``keep_largest``, ``simplify`` the cells per axis of the vertex clustering,
``smooth`` the keyword arguments of ``ops.mesh_smooth_raw``."""


def mesh_options(normals="accumulate", level=0.5, colors=False, clean=None, simplify=None, smooth=None):
    """The ``MeshOptions`` of the mesh calls' arguments, or ValueError.  ``normals``: None or a mode of
    ``ops.NORMALS_MODES``.  ``clean``: None, or 6 / 26; dropped voxels become 0.0, which must lie below the level.
    ``simplify``: None, or an int in 1..512.  ``smooth``: None, the iterations (an int in 1..64) of
    ``ops.mesh_smooth_raw`` at its default factors, or a dict with ``iterations`` and any of ``lam``, ``mu``,
    ``pin_border``; the record holds the full keyword dict."""
    if normals is not None and normals not in ops.NORMALS_MODES:
        raise ValueError("normals must be None or one of %s, got %r" % (sorted(ops.NORMALS_MODES), normals))
    if clean is not None:
        if clean not in ops.CONNECTIVITIES:
            raise ValueError("clean must be None or one of %s, got %r" % (list(ops.CONNECTIVITIES), clean))
        if not float(level) > 0.0:
            raise ValueError("clean fills the dropped voxels with 0.0: it needs level > 0, got %r" % (level,))
    if simplify is not None:
        ops._simplify_cells("simplify", simplify)
    if smooth is not None:
        if isinstance(smooth, dict):
            unknown = sorted(set(smooth) - set(SMOOTH_KEYS))
            if unknown or "iterations" not in smooth:
                raise ValueError("smooth: a dict has 'iterations' and any of %s, got %r"
                                 % (list(SMOOTH_KEYS[1:]), smooth))
            smooth = dict(SMOOTH_DEFAULTS, **smooth)
        else:
            smooth = dict(SMOOTH_DEFAULTS, iterations=smooth)
        ops._smooth_params("smooth", smooth["iterations"], smooth["lam"], smooth["mu"], smooth["pin_border"])
    return MeshOptions(normals, level, bool(colors), clean, simplify, smooth)


MeshChain = collections.namedtuple("MeshChain", ["verts", "faces", "counts", "normals", "preds", "mc_counts"])
MeshChain.__doc__ = """What ``_mesh_chains`` leaves on the device for one volume, capacity-sized: verts [max_v,3], faces
[max_f,3], counts int32[2] of the mesh handed out (the simplified, smoothed one if asked for), its normals [max_v,3] or
None, netC's raw predictions [3,max_v] or None, and with ``simplify`` marching cubes' own counts (what the capacities
are compared with), else None."""


def _mesh_chains(sdfs, b_min, b_max, opts, bindings=None, gates=None, out=None, max_verts=None, max_faces=None,
                 view=0, bits_out=None):
    """volume [-> its largest body] -> verts, faces [-> their vertex clustering] [-> Taubin passes] -> normals ->
    netC predictions for volumes of one size, every stage one set of launches for all of them and no host value in
    between: one ``MeshChain`` per volume (the chain of one volume is this on a list of one).  ``opts``: a
    ``MeshOptions``.  ``bindings``: None or one QueryBinding per volume (one head), or one ViewsBinding per volume (a
    multi-view head: the colours are row ``view`` of its result); the colour query takes the positions before
    smoothing, which lie on the iso-surface.  ``gates``: as ``ops.marching_cubes_raw_batch``'s, for ``clean``
    too; a gated-off frame's counts of (0, 0) switch the later stages off.  ``out``: None or a dict of the caller's
    buffers (verts, faces, counts, normals, points, point_counts: [n, ...] tensors, preds: a list; with ``clean`` also
    cleaned [n,R,R,R] and clean_stats [n,4], with ``simplify`` simple_verts, simple_faces, simple_counts, simple_vmap,
    with ``smooth`` smooth_verts).  ``max_verts`` / ``max_faces``: marching cubes' capacities, if not its defaults.
    ``bits_out``: None, or int32 [n, ops.volume_bits_words(R)]: the occupancy bits (``ops.volume_bits_raw_batch``) of
    the volumes marching cubes reads -- with ``clean`` the cleaned ones: a dropped blob casts no occlusion -- under
    the same gates."""
    out = out or {}
    n = len(sdfs)
    if opts.clean is not None:  # into a scratch volume: the caller's is never modified
        cc_out = (out["cleaned"], out["clean_stats"]) if "cleaned" in out else None
        sdfs = [c[0] for c in ops.keep_largest_raw_batch(sdfs, opts.level, opts.clean, CLEAN_FILL, gates=gates,
                                                         out=cc_out)]
    if bits_out is not None:
        ops.volume_bits_raw_batch(sdfs, opts.level, gates=gates, out=bits_out)
    mc_out = (out["verts"], out["faces"], out["counts"]) if "verts" in out else None
    raws = ops.marching_cubes_raw_batch(sdfs, opts.level, b_min, b_max, max_verts=max_verts, max_faces=max_faces,
                                        gates=gates, out=mc_out)
    verts, faces, counts = ([r[k] for r in raws] for k in range(3))
    mc_counts = [None] * n
    if opts.simplify is not None:
        mc_counts = counts
        sm_out = (tuple(out["simple_" + k] for k in ("verts", "faces", "counts", "vmap"))
                  if "simple_verts" in out else None)
        raws = ops.mesh_simplify_raw_batch(verts, faces, counts, opts.simplify, b_min, b_max, out=sm_out)
        verts, faces, counts = ([r[k] for r in raws] for k in range(3))
    on_surface = verts
    if opts.smooth is not None:
        verts = ops.mesh_smooth_raw_batch(verts, faces, counts, out=out.get("smooth_verts"), **opts.smooth)
    nrm = [None] * n
    if opts.normals is not None:
        nrm = ops.mesh_normals_raw_batch(verts, faces, counts, opts.normals, out=out.get("normals"))
    preds = [None] * n
    if bindings is not None:
        pt_out = (out["points"], out["point_counts"]) if "points" in out else None
        pts = ops.mesh_points_raw_batch(on_surface, counts, out=pt_out)
        preds = _counted_colours(list(bindings), [p[0] for p in pts], [p[1] for p in pts], outs=out.get("preds"),
                                 view=view)
    return [MeshChain(*frame) for frame in zip(verts, faces, counts, nrm, preds, mc_counts)]


def _finish_mesh(chain, nv, nf):
    """The ``Mesh`` of a chain's capacity-sized tensors once the counts are on the host."""
    col = chain.preds
    if col is not None:  # elementwise: the same bits as over the whole capacity
        col = (col[:, :nv] * 0.5 + 0.5).t().contiguous()
    return Mesh(chain.verts[:nv], chain.faces[:nf], None if chain.normals is None else chain.normals[:nv], col)


def _device_sizes(chain):
    """The counts a chain leaves on the device, as one tensor: (vertices, faces) of the mesh, followed with
    ``simplify`` by the (vertices, faces) marching cubes needed."""
    return chain.counts if chain.mc_counts is None else torch.cat([chain.counts[:2], chain.mc_counts[:2]])


def _collect_meshes(chains, sizes, rerun):
    """The ``Mesh`` of every chain (None for a None) once ``sizes``, per chain the host list of ``_device_sizes``, is
    there: a chain whose marching cubes needed more than its capacities is made again alone with exact ones by
    ``rerun(k, max_verts, max_faces)`` (with ``simplify`` that costs one more host copy, for the new counts)."""
    meshes = []
    for k, (chain, size) in enumerate(zip(chains, sizes)):
        if chain is None:
            meshes.append(None)
            continue
        nv, nf = size[0], size[1]
        need_v, need_f = size[-2], size[-1]
        if need_v > chain.verts.shape[0] or need_f > chain.faces.shape[0]:
            chain = rerun(k, need_v, need_f)
            if chain.mc_counts is not None:
                nv, nf = chain.counts.cpu().tolist()[:2]
        meshes.append(_finish_mesh(chain, nv, nf))
    return meshes


@torch.no_grad()
def reconstruct_mesh(sdf, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1), normals="accumulate", netC=None,
                     feat_tensor_C=None, calib_tensor=None, clean=None, simplify=None, smooth=None, view=None):
    """The finished mesh of an occupancy volume [1,1,D,H,W] (or [D,H,W]) as one device chain: marching cubes,
    per-vertex normals (``normals``: "accumulate", "reference" -- mesh_util.compute_normal's two modes -- or
    None to skip them) and, with ``netC``, per-vertex colours netC.query(vertices) * 0.5 + 0.5 as
    ``mesh_util.vertex_colors`` gives them.  Returns a ``Mesh``; None for ``sdf is None``.  One host sync
    per mesh (the two counts, read after everything is enqueued); if a capacity guess was short the chain
    runs once more with exact capacities.  ``view``: None for a single-view ``netC`` (a multi-view one then raises
    NotImplementedError); k in 0..V-1 for a multi-view ``netC`` (num_views = V; ValueError for a single-view one or a k
    outside): ``feat_tensor_C`` then holds the V views' maps (batch V), ``calib_tensor`` is [V,4,4], and the colours are
    row k of the head's result on the vertices -- ``netC.query(feats, vertices for every view, calibs)[0][k]``, the
    view-averaged prediction under view k's in-image mask -- from one counted launch
    (``ops.query_views_counted_batch``), still without a host value in between.  ``clean``: None, or 6 / 26 =
    ``keep_largest(sdf, level, clean)`` in front of marching cubes inside the same chain (into a scratch volume;
    ``sdf`` is not modified; needs level > 0).  ``simplify``: None, or the cells per axis (1..512) of
    ``ops.mesh_simplify_raw`` over the box between marching cubes and the normals / colours: the mesh, its normals and
    its colours are those of the simplified mesh (nothing is averaged; the colour query shrinks with it).  Still one
    host sync: marching cubes' counts (for the capacity check) and the simplified ones come in one copy.
    ``smooth``: None, the iterations (1..64), or dict(iterations=, lam=, mu=, pin_border=) of ``smooth_mesh`` behind
    marching cubes / the clustering: the vertices and normals are the smoothed mesh's, while the colours are queried
    at the positions before smoothing (on the iso-surface) and so are the bits that ``smooth=None`` gives.  The counts
    do not change: the one host sync and the re-run are as before."""
    if sdf is None:
        return None
    opts = mesh_options(normals, level, netC is not None, clean, simplify, smooth)
    _check_colour_view("reconstruct_mesh", netC, view)
    bindings = None
    if netC is not None:
        bindings = _bind_netC("reconstruct_mesh", netC, [(feat_tensor_C, calib_tensor, sdf.device)], view)

    def run(k=0, max_verts=None, max_faces=None):
        return _mesh_chains([sdf], b_min, b_max, opts, bindings, max_verts=max_verts, max_faces=max_faces,
                            view=view or 0)[0]

    chain = run()
    return _collect_meshes([chain], [_device_sizes(chain).cpu().tolist()], run)[0]  # the one host sync


@torch.no_grad()
def reconstruct_mesh_many(sdfs, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1), normals="accumulate", netC=None,
                          feat_tensors_C=None, calib_tensors=None, clean=None, simplify=None, smooth=None, view=None):
    """``[reconstruct_mesh(s, level, b_min, b_max, normals, netC, feat_tensors_C[i], calib_tensors[i], clean, simplify,
    smooth, view) for i, s in enumerate(sdfs)]`` -- every field of every ``Mesh`` the same bits -- with the chain enqueued ONCE for all volumes
    (batched marching cubes, normals, points and one counted colour query per ops.MAX_FRAMES volumes) and ONE host
    sync for all the counts (monoport_amd extension; the hook of a coalescing stage).  ``None`` entries of ``sdfs``
    give ``None``; the other volumes must be of one size (ValueError).  ``feat_tensors_C`` / ``calib_tensors``: one
    entry per volume (those of ``None`` volumes are not looked at).  A volume whose capacity guess was short is
    re-run alone with exact capacities, as ``reconstruct_mesh`` does.  ``view``: as in ``reconstruct_mesh``; with a
    multi-view ``netC`` the colour query of all volumes is one ``ops.query_views_counted_batch`` launch per
    ``ops.max_view_frames(V)`` volumes."""
    sdfs = list(sdfs)
    opts = mesh_options(normals, level, netC is not None, clean, simplify, smooth)
    _check_colour_view("reconstruct_mesh_many", netC, view)
    if netC is not None:
        if feat_tensors_C is None or calib_tensors is None:
            raise ValueError("reconstruct_mesh_many: netC needs feat_tensors_C and calib_tensors")
        if len(feat_tensors_C) != len(sdfs) or len(calib_tensors) != len(sdfs):
            raise ValueError("reconstruct_mesh_many: %d volumes, %d feature sets, %d calibrations"
                             % (len(sdfs), len(feat_tensors_C), len(calib_tensors)))
    idx = [i for i, s in enumerate(sdfs) if s is not None]
    if len({tuple(sdfs[i].shape[-3:]) for i in idx}) > 1:
        raise ValueError("reconstruct_mesh_many wants volumes of one size, got %s"
                         % sorted({tuple(sdfs[i].shape[-3:]) for i in idx}))
    bindings = None
    if netC is not None:
        bindings = _bind_netC("reconstruct_mesh_many", netC,
                              [(feat_tensors_C[i], calib_tensors[i], sdfs[i].device) for i in idx], view)
    meshes = [None] * len(sdfs)
    if not idx:
        return meshes
    live = [sdfs[i] for i in idx]

    def rerun(k, max_verts, max_faces):
        return _mesh_chains([live[k]], b_min, b_max, opts, None if bindings is None else [bindings[k]],
                            max_verts=max_verts, max_faces=max_faces, view=view or 0)[0]

    chains = _mesh_chains(live, b_min, b_max, opts, bindings, view=view or 0)
    sizes = torch.stack([_device_sizes(c) for c in chains]).cpu().tolist()  # the one host sync
    for i, mesh in zip(idx, _collect_meshes(chains, sizes, rerun)):
        meshes[i] = mesh
    return meshes


def _shape_counts(pairs):
    """int32 [n,2] = the (vertices, faces) that the shapes of n (verts, faces) pairs give, on the pairs' device (through
    pinned memory, nothing waited for)."""
    counts = torch.tensor([[v.shape[0], f.shape[0]] for v, f in pairs], dtype=torch.int32)
    dev = pairs[0][0].device
    if dev.type == "cuda":
        counts = counts.pin_memory().to(dev, non_blocking=True)
    return counts


@torch.no_grad()
def simplify_mesh(mesh, cells, b_min=(-1, -1, -1), b_max=(1, 1, 1), normals="accumulate"):
    """A smaller mesh by vertex clustering on the device (monoport_amd extension; ``ops.mesh_simplify_raw``): every
    vertex of ``mesh`` (a ``Mesh``, or a (verts [V,3] f32, faces [F,3] int32) pair) falls into one of ``cells``^3 cells
    (an int in 1..512) over the box, each occupied cell becomes one vertex at its members' mean, and the faces that do
    not collapse are kept in order.  Returns (``Mesh``, vmap): normals recomputed on the simplified mesh (``normals``:
    "accumulate", "reference" or None), ``colors`` None, and vmap int32 [V] = the new index of every old vertex (-1 for
    one with a non-finite or huge coordinate) to carry attributes over.  One host sync (the two counts).
    ``(None, None)`` for ``mesh is None``."""
    if mesh is None:
        return None, None
    mesh_options(normals, simplify=cells)
    verts, faces = ops._f32c(mesh[0]), mesh[1].contiguous()
    counts = _shape_counts([(verts, faces)])[0]
    v, f, c, vmap = ops.mesh_simplify_raw(verts, faces, counts, cells, b_min, b_max)
    nrm = ops.mesh_normals_raw(v, f, c, normals) if normals is not None else None
    nv, nf = c.cpu().tolist()
    return Mesh(v[:nv], f[:nf], None if nrm is None else nrm[:nv], None), vmap


@torch.no_grad()
def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, pin_border=True, normals="accumulate"):
    """A faired mesh by Taubin smoothing on the device (monoport_amd extension; ``ops.mesh_smooth_raw``, defined in
    include/monoport_hip.h): ``iterations`` (1..64) times, every vertex of ``mesh`` (a ``Mesh``, or a (verts [V,3] f32,
    faces [F,3] int32) pair) moves by ``lam`` towards the mean of its one-ring and then by ``mu`` (negative: away from
    it), which takes the lattice terraces out of a marching-cubes mesh of a sharp field without the shrinkage of plain
    Laplacian passes (mu = 0).  ``pin_border``: the vertices of open edges stay where they are.  Returns a ``Mesh``
    with the faces of the input, normals recomputed on the smoothed vertices (``normals``: "accumulate", "reference"
    or None) and the input's ``colors`` carried over unchanged.  It gains little on a field that is already smooth
    (DESIGN.md section 4.8.5).  No host sync.  None for ``mesh is None``."""
    if mesh is None:
        return None
    kw = mesh_options(normals, smooth=dict(iterations=iterations, lam=lam, mu=mu, pin_border=pin_border)).smooth
    verts, faces = ops._f32c(mesh[0]), mesh[1].contiguous()
    counts = _shape_counts([(verts, faces)])[0]
    out = ops.mesh_smooth_raw(verts, faces, counts, **kw)
    nrm = ops.mesh_normals_raw(out, faces, counts, normals) if normals is not None else None
    return Mesh(out, faces, nrm, mesh[3] if len(mesh) > 3 else None)


MeshRender = collections.namedtuple("MeshRender", ["image", "depth", "face"])
MeshRender.__doc__ = """Picture of ``render_mesh``: image [H,W,3] f32 (None without shading), depth [H,W] f32 (+0.0 where
nothing is seen), face [H,W] int32 (-1 where nothing is seen); with a set of cameras each has a leading [n_views]."""

SHADES = ("colors", "normals", "netC", None)


_Subjects = collections.namedtuple("_Subjects", ["verts", "faces", "counts", "capacity", "attrs", "channel_major",
                                                 "paint", "normals", "transfers"],
                                   defaults=(None, None, False, (1.0, 0.0, -np.inf, np.inf), None, None))
_Subjects.__doc__ = """What a set of pictures is of, one list entry per subject: verts, faces and the device counts;
``capacity`` (max_v, max_f) where the subjects' tensors are cut to their own sizes, None where all share one capacity;
the per-vertex values ``attrs`` that the shade paints (None: ``shade`` None or "netC") with their layout and their
(scale, bias, lo, hi); the normals (None where no lighting reads them) and, for a ``Lighting.transfer``, the radiance
transfers."""
NORMALS_PAINT = (0.5, 0.5, 0.0, 1.0)  # as main.py:220-225 paints them


def _mesh_subjects(who, meshes, shade=None, lighting=None):
    """The ``_Subjects`` of live ``Mesh``es (no None): counts from the tensors' shapes, the capacity of the call the
    largest of them, finished colours painted as they are."""
    if shade not in SHADES:
        raise ValueError("%s: shade must be one of %s, got %r" % (who, list(SHADES), shade))
    s = _Subjects([m.verts.contiguous() for m in meshes], [m.faces.contiguous() for m in meshes], None)
    s = s._replace(counts=list(_shape_counts(list(zip(s.verts, s.faces))).unbind(0)),
                   capacity=(max(v.shape[0] for v in s.verts), max(f.shape[0] for f in s.faces)))
    if shade in ("colors", "normals"):
        attrs = [m.colors if shade == "colors" else m.normals for m in meshes]
        if any(a is None for a in attrs):
            raise ValueError("%s: shade=%r, but the mesh has no %s" % (who, shade, shade))
        s = s._replace(attrs=[ops._f32c(a) for a in attrs], paint=NORMALS_PAINT if shade == "normals" else s.paint)
    if lighting is not None:
        s = s._replace(normals=[ops._f32c(m.normals) for m in meshes],
                       transfers=None if lighting.transfer is None else [m.transfer for m in meshes])
    return s


def _chain_subjects(chains, shade, transfers=None):
    """The ``_Subjects`` of ``MeshChain``s (a slot's): the chains' own device counts, one capacity; ``shade="colors"``
    paints netC's raw predictions [3,cap] channel-major, * 0.5 + 0.5 behind the interpolation (``_finish_mesh``'s
    factors), which costs no transposing launch -- and is why the capacity may not be cut."""
    s = _Subjects([c.verts for c in chains], [c.faces for c in chains], [c.counts for c in chains],
                  normals=[c.normals for c in chains], transfers=transfers)
    if shade == "normals":
        return s._replace(attrs=s.normals, paint=NORMALS_PAINT)
    if shade == "colors":
        return s._replace(attrs=[c.preds for c in chains], channel_major=True, paint=(0.5, 0.5, -np.inf, np.inf))
    return s


def _check_shade_netC(who, shade, netC, view):
    """``shade`` against ``netC`` / ``view`` of the render calls, before anything is bound or enqueued."""
    if shade == "netC" and netC is None:
        raise ValueError("%s: shade='netC' colours the picture per pixel with netC= (and its feature maps and "
                         "calibration)" % who)
    if shade != "netC" and netC is not None:
        raise ValueError("%s: netC= is what shade='netC' queries; shade=%r does not use it" % (who, shade))
    _check_colour_view(who, netC, view)


def _single_camera(calibs):
    return (calibs.dim() if torch.is_tensor(calibs) else np.asarray(calibs).ndim) == 2


@torch.no_grad()
def render_mesh(mesh, calibs, res=257, shade="colors", projection="orthogonal", nearest="max", background=1.0,
                near=None, perspective_correct=False, netC=None, feat_tensor_C=None, calib_tensor=None, view=None,
                samples=1, lighting=None):
    """The z-buffered picture of a ``Mesh`` on the device (monoport_amd extension; ``ops.mesh_render_raw``): any camera
    ``calibs`` ([4,4] / [3,4], the convention of the queries; or [n_views, ...] for several pictures in one set of
    launches), any size ``res`` (int or (H, W)).  ``shade``: "colors" (the mesh's colours), "normals" (its normals * 0.5
    + 0.5 clamped to [0,1], as the reference paints them), "netC" (below) or None (depth and face ids only).  x runs
    along the first image index as in the painted canvas, so a square image feeds ``visulization`` unchanged.  ``near``
    (> 0, with ``projection="perspective"``): faces are clipped at the plane zc = near, so the camera may stand
    anywhere, also inside the body; ``perspective_correct`` then interpolates depth and shading perspective-correctly
    (both as ``ops.mesh_render_raw``; None, the default, is the unclipped call).  Returns a ``MeshRender``; None for
    ``mesh is None``.  No host sync.

    ``shade="netC"`` colours the picture per pixel (deferred shading): the rasteriser interpolates the world-space
    surface position of every covered pixel, ``netC`` (with ``feat_tensor_C`` and ``calib_tensor``, the frame's own
    input maps and calibration, as ``reconstruct_mesh`` takes them) is queried at those points only, and ``image``
    holds ``netC.query(point) * 0.5 + 0.5`` there and ``background`` elsewhere; ``depth`` and ``face`` are those of
    ``shade=None``.  The mesh needs neither colours nor normals, the query costs the covered pixels instead of the
    vertices, and the texture keeps netC's detail whatever the mesh density.  ``view``: None for a single-view
    ``netC``, k for row k of a multi-view one, as in ``reconstruct_mesh``.  ``shade="netC"`` without ``netC``, and
    ``netC`` with any other shade, are ValueErrors raised before anything is enqueued.

    ``lighting`` (a ``Lighting``; None, the default: nothing more is enqueued): the image is lit per pixel -- a second
    pass of the rasteriser with the mesh's normals as the attribute, under the same camera, ``near`` and flags, then
    ``ops.picture_light_batch`` in place: clamp(albedo * shading, 0, 1) at the covered pixels, where the albedo is the
    picture's own colours (``shade="colors"`` / ``"netC"``) or the lighting's constant ``albedo`` (``shade="normals"``).
    ``shade=None``, ``shade="normals"`` without a constant albedo, a mesh without normals and a ``self_shadow`` (which
    needs a scene's light: ``render_mesh_many_in_scene``) are ValueErrors raised before anything is enqueued.

    ``samples`` (1, the default: exactly the calls and tensors above): s in 2..4 anti-aliases the picture.  Every pass
    -- the shade, the positions of ``shade="netC"``, the normals and transfer of ``lighting`` -- runs under the same
    camera at s times ``res`` (s * res may not exceed 4096; the near-plane clip and the 2^22 snap guard act at that
    size), which samples every pixel on a regular s x s grid, and ``ops.picture_resolve_batch`` averages once at the
    end: one launch more.  Returns a ``ResolvedPicture`` (image, depth, face, mask None, coverage = the subject's
    alpha): bit for bit the resolve, as include/monoport_hip.h defines it, of this call at ``res * s``.  The working
    pictures cost s * s times the memory, and ``shade="netC"`` queries every covered fine sample: s * s times the
    points.  A ``samples`` outside 1..4 and an s * res beyond 4096 are ValueErrors raised before anything is
    enqueued."""
    if type(samples) is not int or samples != 1:  # refused here also for ``mesh is None``
        ops.raster("render_mesh", res, projection, nearest, background, near, perspective_correct, samples)
    _check_shade_netC("render_mesh", shade, netC, view)
    if lighting is not None:
        _check_lighting("render_mesh", lighting, shade, [mesh], None)
    if mesh is None:
        return None
    return render_mesh_many([mesh], calibs, res, shade, projection, nearest, background, near, perspective_correct,
                            netC=netC, feat_tensors_C=[feat_tensor_C], calib_tensors=[calib_tensor], view=view,
                            lighting=lighting, samples=samples)[0]


@torch.no_grad()
def render_mesh_many(meshes, calibs, res=257, shade="colors", projection="orthogonal", nearest="max", background=1.0,
                     near=None, perspective_correct=False, netC=None, feat_tensors_C=None, calib_tensors=None,
                     view=None, samples=1, lighting=None):
    """``[render_mesh(m, calibs, ...) for m in meshes]`` in one set of launches per ops.MAX_FRAMES pictures (meshes x
    views), the same bits.  ``calibs``: one camera set for all meshes (a tensor / array), or a list with one camera set
    per mesh (those of ``None`` meshes are not looked at; all of one n_views).  ``None`` meshes give ``None``.  The
    meshes may differ in size: the per-mesh counts are made on the device from the tensors' shapes and the capacity of
    the call is the largest of them (no row at or beyond a mesh's counts is touched).  ``near`` / ``perspective_correct``
    as in ``render_mesh``: one plane for all.  With ``shade="netC"``: ``feat_tensors_C`` / ``calib_tensors`` hold one
    entry per mesh (those of ``None`` meshes are not looked at), and the colour query of all meshes is one counted
    launch per ops.MAX_FRAMES meshes (``ops.max_view_frames(V)`` with ``view``).  ``lighting``: as in ``render_mesh``,
    one for all meshes; the normal pass and the lighting are one set of launches per ops.MAX_FRAMES pictures more.
    ``samples``: as in ``render_mesh`` -- 1 changes nothing; 2..4 give ``ResolvedPicture``s, every pass at ``samples``
    times ``res`` and one resolve per ops.MAX_FRAMES pictures at the end (``_resolved_pictures``).  No host sync."""
    ras = ops.raster("render_mesh_many", res, projection, nearest, background, near, perspective_correct, samples)
    raws, cams, _, resolved = _render_mesh_many("render_mesh_many", meshes, calibs, ras, shade, netC, feat_tensors_C,
                                                calib_tensors, view, lighting)
    if resolved is not None:
        return [None if pic is None else ResolvedPicture(*_squeezed(pic, cam)) for pic, cam in zip(resolved, cams)]
    return [None if raw is None else MeshRender(*_squeezed(raw, cam)) for raw, cam in zip(raws, cams)]


def _squeezed(tensors, cam):
    """A picture's tensors [n_views, ...] as the caller of one [4,4] / [3,4] camera gets them: without the leading 1."""
    return tuple(None if t is None else t[0] for t in tensors) if _single_camera(cam) else tensors


def _render_mesh_many(who, meshes, calibs, ras, shade, netC, feat_tensors_C, calib_tensors, view, lighting, scene=None,
                      composite="depth", who_scene=None):
    """``render_mesh_many`` under the ``ops.Raster`` ``ras``, through ``_resolved_pictures`` -> what that returns, with
    the camera sets: (per mesh the raw picture (image, depth, face; each [n_views, ...]) or None, per mesh its camera
    set, the composites or None, the resolved pictures or None).  ``scene``: None, or the ``Scene`` behind the meshes
    (``render_mesh_many_in_scene``, which names itself in ``who_scene``): a None mesh then gives an uncovered picture
    over the bare scene, and under the scene's ``Light`` the live meshes' shadow maps are rendered first
    (``_shadow_maps``), for the lighting's ``self_shadow`` and for the scene, an uncovered map for a None mesh."""
    _check_shade_netC(who, shade, netC, view)
    meshes = list(meshes)
    light = None if scene is None else scene.light
    if lighting is not None:
        _check_lighting(who, lighting, shade, meshes, light)
    if netC is not None:
        if feat_tensors_C is None or calib_tensors is None:
            raise ValueError("%s: netC needs feat_tensors_C and calib_tensors" % who)
        if len(feat_tensors_C) != len(meshes) or len(calib_tensors) != len(meshes):
            raise ValueError("%s: %d meshes, %d feature sets, %d calibrations"
                             % (who, len(meshes), len(feat_tensors_C), len(calib_tensors)))
    idx = [i for i, m in enumerate(meshes) if m is not None]
    if not idx and scene is None:
        return [None] * len(meshes), [None] * len(meshes), None, None
    cams = _camera_sets(who, calibs, len(meshes), "meshes")
    colours = subjects = maps = shadow = None
    if idx:
        if netC is not None:
            bindings = _bind_netC(who, netC,
                                  [(feat_tensors_C[i], calib_tensors[i], meshes[i].verts.device) for i in idx], view)

            def colours(pts, counts):
                return _counted_colours(bindings, pts, counts, view=view or 0)
        subjects = _mesh_subjects(who, [meshes[i] for i in idx], shade, lighting)
        if light is not None:  # a None mesh casts no shadow
            shadow = (light,) + _shadow_maps(who, subjects, light)
            maps = tuple([hole] * len(meshes) for hole in _uncovered_map(light, subjects.verts[0].device))
            for k, i in enumerate(idx):
                maps[0][i], maps[1][i] = shadow[1][k], shadow[2][k]
    fronts, done, resolved = _resolved_pictures(who, subjects, cams, ras, shade, colours, lighting, shadow, scene, maps,
                                                composite, live=idx, who_scene=who_scene)
    return fronts, cams, done, resolved


ResolvedPicture = collections.namedtuple("ResolvedPicture", ["image", "depth", "face", "mask", "coverage"])
ResolvedPicture.__doc__ = """An anti-aliased picture (``samples`` > 1; ``resolve_picture``): every pixel is the box of the
s x s samples that the passes took inside it.  image [H,W,3] f32 = their mean (None with ``shade=None``), depth [H,W] f32
and face [H,W] int32 = those of the nearest sample that shows (+0.0 and -1 where none does; with a scene the face is the
subject's, -1 where the scene is nearest), mask [H,W] uint8 = the largest of the composite's 0 / 1 / 2 (None without a
scene), coverage [H,W] f32 = the fraction of the samples that is the subject's: its alpha, and ``image - (1 - coverage) *
background`` the premultiplied subject (without a scene).  With a set of cameras each has a leading [n_views]."""


def _resolved_pictures(who, subjects, cams, ras, shade, colours=None, lighting=None, shadow=None, scene=None, maps=None,
                       composite="depth", live=None, out=None, back=None, who_scene=None):
    """THE pictures under the ``ops.Raster`` ``ras`` with its ``samples``, for the render calls, a slot and a slot's
    re-run alike; the one place that knows about supersampling.  Every pass runs under ``ops.fine_raster(ras)`` -- at
    ``samples`` times ``ras.res``, under the same cameras -- through the two bodies below, and the resolve runs once at
    the end: (1) ``_subject_pictures`` of ``subjects`` (None: no subject at all) under the camera sets ``cams[i]`` for
    i in ``live`` (None: every one); (2) with a ``scene``: ``_scene_pictures`` under all of ``cams`` -- the bare scene
    without subjects, else the composite, a picture outside ``live`` being an uncovered one of the scene's size;
    (3) ``ras.samples`` > 1: ``ops.picture_resolve_batch`` of the composites (image, depth and mask theirs, the face
    ids the subject's), else of the scene's, else of the live subjects' pictures.  -> (per camera set the subject's
    raw picture or None, per camera set the composite (image, depth, mask) or the bare scene's raw picture or None
    without a scene, per camera set the resolved (image, depth, face, mask, coverage) or None with ``samples`` = 1 --
    then nothing is enqueued or allocated beyond (1) and (2)).  ``shade="netC"`` queries every covered FINE sample:
    ``samples``^2 times the points.  ``out``: None, or the caller's buffers: the keys of ``_subject_pictures`` and
    ``_scene_pictures`` at the fine size, and ``resolved`` = (image, depth, face, mask, coverage) at ``ras.res``, each
    [n, ...] or None.  ``back``: as in ``_scene_pictures``, at the fine size."""
    fine, out, n, who_scene = ops.fine_raster(ras), out or {}, len(cams), who_scene or who
    bare = subjects is None and live is None  # the scene alone: nothing is composited
    live = list(range(n)) if live is None else list(live)
    fronts, done = [None] * n, None
    if subjects is not None:
        for i, raw in zip(live, _subject_pictures(who, subjects, [cams[i] for i in live], fine, shade, colours,
                                                  lighting, shadow, out)):
            fronts[i] = raw
    if scene is not None and bare:
        done = _scene_pictures(who_scene, scene, cams, fine, maps, out=out, back=back)[0]
    elif scene is not None:
        nv = ops._view_calibs(who_scene, cams[0]).shape[0]
        for i in range(n):
            if fronts[i] is None:  # no subject: an uncovered picture of the scene's size
                shape, dev = (nv,) + fine.res, scene.verts.device
                fronts[i] = (torch.full(shape + (3,), fine.background, dtype=torch.float32, device=dev),
                             torch.zeros(shape, dtype=torch.float32, device=dev),
                             torch.full(shape, -1, dtype=torch.int32, device=dev))
        done = _scene_pictures(who_scene, scene, cams, fine, maps, fronts, composite, out, back)[1]
    if ras.samples == 1:
        return fronts, done, None
    masks, where = None, range(n)
    if scene is None:
        pics, where = [fronts[i] for i in live], live
    elif bare:
        pics = done
    else:
        pics, masks = [(d[0], d[1], f[2]) for d, f in zip(done, fronts)], [d[2] for d in done]
    resolved = [None] * n
    if pics:
        got = ops.picture_resolve_batch(None if pics[0][0] is None else [p[0] for p in pics], [p[1] for p in pics],
                                        [p[2] for p in pics], masks, ras.samples, ras.nearest, out.get("resolved"),
                                        who=who_scene)
        for i, pic in zip(where, got):
            resolved[i] = pic
    return fronts, done, resolved


def _subject_pictures(who, subjects, cams, ras, shade, colours=None, lighting=None, shadow=None, out=None):
    """THE picture of a set of subjects, for the render calls, a slot and a slot's re-run alike: per subject the raw
    (image, depth, face; each [n_views, ...]) of ``subjects`` (a ``_Subjects``) under one camera set each and the
    ``ops.Raster`` ``ras``.  (1) ``shade="netC"``: ``ops.render_netc_batch`` -- positions, covered pixels, ``colours``
    (the counted query ``(points, counts) -> predictions``: ``_counted_colours`` over bindings, or a slot's
    ``_picture_colours``), paint -- with the self-shadow's shade made from the position picture before the paint
    covers it; any other shade: one pass with the subjects' attributes and paint.  (2) ``lighting`` (checked by the
    caller): ``ops.light_pictures_batch`` in place on the images.  ``shadow``: (the scene's ``Light``, map depths, map
    faces) as ``_shadow_maps`` gives them, read only by a ``lighting.self_shadow``.  ``out``: None (fresh tensors), or
    a dict of the caller's buffers, each [n, ...]: ``image`` (None with ``shade=None``), ``depth``, ``face``; for
    ``shade="netC"`` ``lists`` = (points, pixels, count) as ``ops.render_netc_batch`` takes them; for the lighting
    ``light``, the ``buffers`` dict of ``ops.light_pictures_batch``.  A new picture stage is one block here."""
    s, out = subjects, out or {}
    pics = (out["image"], out["depth"], out["face"]) if "depth" in out else None
    buffers = out.get("light")
    if lighting is None or lighting.self_shadow is None:
        shadow = None
    shades = None
    if shade == "netC":
        hook = None
        if shadow is not None:  # the positions are there before the paint
            def hook(positions, face_ids):
                nonlocal shades
                shades = ops.self_shades(who, positions, face_ids, lighting, shadow,
                                         None if buffers is None else buffers["shade"])
        raws = ops.render_netc_batch(who, s.verts, s.faces, s.counts, cams, ras, colours, out=pics,
                                     lists=out.get("lists"), capacity=s.capacity, positions_hook=hook)
    else:
        raws = ops._attr_pass(who, s.verts, s.faces, s.counts, s.attrs, cams, ras, pics, s.capacity, s.channel_major,
                              s.paint)
    if lighting is not None:
        ops.light_pictures_batch(who, s.verts, s.faces, s.counts, s.normals, cams, ras, lighting, [r[0] for r in raws],
                                 capacity=s.capacity, shadow=shadow, buffers=buffers, shades=shades,
                                 transfers=s.transfers)
    return raws


ScenePicture = collections.namedtuple("ScenePicture", ["image", "depth", "face", "mask"])
ScenePicture.__doc__ = """A picture of ``composite``: image [H,W,3] f32 and depth [H,W] f32 of whichever of the two
pictures shows at a pixel (``background`` and +0.0 where neither does), face [H,W] int32 = the FRONT picture's face ids
(-1 wherever the front is not covered, also where it is hidden), mask [H,W] uint8 = 0 neither, 1 back (the scene), 2
front (the subject); with a set of cameras each has a leading [n_views]."""


class Light:
    """The one light of a ``Scene``: a camera from which the subject's shadow map is rendered (monoport_amd extension;
    mp_picture_shadow in include/monoport_hip.h).  ``calib``: [4,4] / [3,4], the rows of [R|t] as every camera here;
    ``projection``: "orthogonal" (a directional light) or "perspective" (a spot); ``res``: the map's size, an int or
    (Hs, Ws), each in 1..4096; ``near`` (perspective lights only): the map is then rendered with the clipped rasteriser
    and ``perspective_correct=True``, so the light may stand close to the subject; ``bias`` (finite, >= 0): how much
    nearer than a point the map must be to shadow it; ``radius`` (0..3): the (2 radius + 1)^2 box of bilinear lookups
    that softens the edge; ``strength`` in [0, 1]: a fully shadowed pixel is multiplied by 1 - strength; ``nearest``:
    "min" (the default: depth is the distance along the light) or "max", what the map is rendered and compared with.
    Everything is validated here, before any allocation; a Light holds host values only."""

    def __init__(self, calib, projection="orthogonal", res=512, near=None, bias=0.0, radius=1, strength=0.6,
                 nearest="min"):
        who = "Light"
        cal = ops._view_calibs(who, calib)
        if cal.shape[0] != 1:
            raise ValueError("%s: calib must be one [4,4] or [3,4] camera, got %d" % (who, cal.shape[0]))
        if not np.isfinite(cal).all():
            raise ValueError("%s: calib must be finite" % who)
        if not isinstance(projection, str) or projection not in ops.PROJECTIONS:
            raise ValueError("%s: projection must be one of %s, got %r" % (who, sorted(ops.PROJECTIONS), projection))
        if not isinstance(nearest, str) or nearest not in ops.NEAREST_MODES:
            raise ValueError("%s: nearest must be one of %s, got %r" % (who, sorted(ops.NEAREST_MODES), nearest))
        try:
            hs, ws = (res, res) if isinstance(res, (int, np.integer)) and not isinstance(res, bool) else tuple(res)
            ok = all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) for s in (hs, ws))
        except (TypeError, ValueError):
            ok = False
        if not ok or not (1 <= hs <= ops.SHADOW_MAX_SIZE and 1 <= ws <= ops.SHADOW_MAX_SIZE):
            raise ValueError("%s: res must be an int or (Hs, Ws) in 1..%d, got %r" % (who, ops.SHADOW_MAX_SIZE, res))
        if near is not None:
            near = ops._render_clip(who, projection, near, True)[0]
        self.bias, self.radius, self.strength = ops.shadow_params(who, bias, radius, strength)
        self.calib = cal.reshape(3, 4).copy()
        self.projection, self.nearest, self.res, self.near = projection, nearest, (int(hs), int(ws)), near

    @classmethod
    def directional(cls, direction, b_min=(-1, -1, -1), b_max=(1, 1, 1), **kw):
        """A directional light whose rays travel along ``direction`` (any length), fitted to the box [b_min, b_max].
        In float64, then rounded to f32: d = direction / |direction|; e = the coordinate axis with the smallest |d . e|
        (the first of equals); x = (e x d) / |e x d|, y = d x x, so (x, y, d) is a right-handed orthonormal frame; c =
        (b_min + b_max) / 2 and rho = |b_max - b_min| / 2 * (1 + 2^-20), the box's bounding sphere with a margin for
        the rounding.  The rows of the calib are [x / rho | -x . c / rho], [y / rho | -y . c / rho] and [d | rho -
        d . c]: the sphere fills [-1, 1]^2 of the map and the depth, the distance along the light from the plane that
        touches the sphere on the light's side, runs from 0 to 2 rho -- hence ``nearest="min"``.  ``kw``: ``res``,
        ``bias``, ``radius``, ``strength``."""
        who = "Light.directional"
        d = np.asarray(direction, np.float64).reshape(-1)
        lo, hi = np.asarray(b_min, np.float64).reshape(-1), np.asarray(b_max, np.float64).reshape(-1)
        if d.shape != (3,) or not np.isfinite(d).all() or not np.linalg.norm(d) > 0:
            raise ValueError("%s: direction must be three finite values, not all zero, got %r" % (who, direction))
        box = lo.shape == (3,) and hi.shape == (3,) and np.isfinite(lo).all() and np.isfinite(hi).all()
        if not box or not (hi > lo).all():
            raise ValueError("%s: b_min < b_max must be the finite corners of a box, got %r and %r"
                             % (who, b_min, b_max))
        for k in ("projection", "near", "nearest"):
            if k in kw:
                raise ValueError("%s: a directional light is orthogonal with nearest='min'; %s= is not taken"
                                 % (who, k))
        d = d / np.linalg.norm(d)
        e = np.zeros(3)
        e[int(np.argmin(np.abs(d)))] = 1.0
        x = np.cross(e, d)
        x /= np.linalg.norm(x)
        y = np.cross(d, x)
        c, rho = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2 * (1 + 2.0 ** -20)
        calib = np.zeros((3, 4))
        calib[0, :3], calib[0, 3] = x / rho, -x.dot(c) / rho
        calib[1, :3], calib[1, 3] = y / rho, -y.dot(c) / rho
        calib[2, :3], calib[2, 3] = d, rho - d.dot(c)
        return cls(calib.astype(np.float32), "orthogonal", nearest="min", **kw)


def _check_light(who, light):
    if not isinstance(light, Light):
        raise ValueError("%s: light must be a recon.Light, got %r" % (who, type(light).__name__))


class Transfer:
    """How the radiance transfer of a mesh is traced through its occupancy volume (monoport_amd extension;
    mp_mesh_transfer in include/monoport_hip.h).  ``directions``: D rays per vertex, a multiple of 64 in 64..512;
    ``bias``: how far along the normal a ray starts, ``step``: the distance between its samples, ``reach``: None (a ray
    runs until it leaves the box: J = ceil(sqrt(3) R / step) + 2 samples) or how far it runs (J = ceil(reach / step))
    -- all three in voxels, turned into world units with the box's smallest voxel edge (``rays``).  Built here in
    float64 and rounded to f32 once: the spherical Fibonacci directions z_d = 1 - (2 d + 1) / D, phi_d = d pi (3 -
    sqrt 5), (x, y) = sqrt(1 - z^2) (cos phi, sin phi); the real SH basis at each, in the order of the lighting's H: 1;
    y, z, x; xy, yz, 3 z^2 - 1, zx, x^2 - y^2 with the exact constants sqrt(1/4pi), sqrt(3/4pi), sqrt(15/4pi),
    sqrt(5/16pi), sqrt(15/16pi); ``weight`` = f32(4 pi / D).  prt_k is then the quadrature of (cosine lobe * visibility *
    Y_k) over the sphere: for an unoccluded vertex A_l Y_lm(n) with A = (pi, 2 pi / 3, pi / 4), which times the
    radiance coefficients is what ``Lighting``'s H(n) . sh gives.  Everything is validated here; a Transfer holds host
    values only (``tables(device)`` caches the device copies)."""

    def __init__(self, directions=128, bias=1.5, step=1.0, reach=None):
        who = "Transfer"
        d = directions
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d % 64 or not 64 <= d <= ops.TRANSFER_MAX_DIRS:
            raise ValueError("%s: directions must be a multiple of 64 in 64..%d, got %r"
                             % (who, ops.TRANSFER_MAX_DIRS, directions))
        for what, v, ok in (("bias", bias, lambda v: v >= 0), ("step", step, lambda v: v > 0),
                            ("reach", reach, lambda v: v > 0)):
            if v is None and what == "reach":
                continue
            if (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating))
                    or not math.isfinite(float(v)) or not ok(float(v))):
                raise ValueError("%s: %s must be a finite number %s, got %r"
                                 % (who, what, ">= 0" if what == "bias" else "> 0", v))
        self.directions, self.bias, self.step = int(d), float(bias), float(step)
        self.reach = None if reach is None else float(reach)
        i = np.arange(self.directions, dtype=np.float64)
        z = 1.0 - (2.0 * i + 1.0) / self.directions
        phi = i * math.pi * (3.0 - math.sqrt(5.0))
        rho = np.sqrt(1.0 - z * z)
        x, y = rho * np.cos(phi), rho * np.sin(phi)
        c0, c1 = math.sqrt(1 / (4 * math.pi)), math.sqrt(3 / (4 * math.pi))
        c2, c20, c22 = math.sqrt(15 / (4 * math.pi)), math.sqrt(5 / (16 * math.pi)), math.sqrt(15 / (16 * math.pi))
        basis = np.stack([np.full_like(z, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c20 * (3 * z * z - 1),
                          c2 * z * x, c22 * (x * x - y * y)], axis=1)
        self.dirs = np.ascontiguousarray(np.stack([x, y, z], axis=1).astype(np.float32))
        self.basis = np.ascontiguousarray(basis.astype(np.float32))
        self.weight = float(np.float32(4.0 * math.pi / self.directions))
        self._tables = {}

    def rays(self, r, b_min, b_max):
        """(bias_w, step_w, max_steps) at resolution ``r`` in the box: voxels times the smallest voxel edge, as f32."""
        edge = float(np.min((np.asarray(b_max, np.float64) - np.asarray(b_min, np.float64)).reshape(3))) / r
        steps = (math.ceil(math.sqrt(3.0) * r / self.step) + 2 if self.reach is None
                 else math.ceil(self.reach / self.step))
        return float(np.float32(self.bias * edge)), float(np.float32(self.step * edge)), max(1, int(steps))

    def tables(self, device):
        """The (dirs [D,3], basis [D,9]) f32 tensors on ``device``, made once per device."""
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = (torch.from_numpy(self.dirs).to(device), torch.from_numpy(self.basis).to(device))
        return self._tables[key]


class TransferMesh(Mesh):
    """A ``Mesh`` (the same four fields, so it unpacks, compares and clones as one) that also carries ``.transfer``,
    the [V,9] radiance transfer of its vertices (``with_transfer``)."""
    transfer = None


def with_transfer(mesh, prt):
    """``mesh`` with ``prt`` ([V,9] f32, ``mesh_transfer``'s first result) as its ``.transfer``: what a render call with
    ``Lighting(transfer=...)`` wants of every mesh.  None for ``mesh is None``."""
    if mesh is None:
        return None
    if not torch.is_tensor(prt) or prt.dim() != 2 or tuple(prt.shape) != (mesh.verts.shape[0], 9):
        raise ValueError("with_transfer: prt must be a [V,9] tensor for the mesh's %d vertices, got %r"
                         % (mesh.verts.shape[0], None if not torch.is_tensor(prt) else tuple(prt.shape)))
    out = TransferMesh(*mesh)
    out.transfer = prt
    return out


@torch.no_grad()
def volume_bits(sdf, level=0.5):
    """The occupancy bits of a cubic volume (``ops.volume_bits_raw``): int32 [ops.volume_bits_words(R)] on the device,
    one bit per voxel set iff v > level, then the tracer's block bits.  No host sync."""
    return ops.volume_bits_raw(sdf, level)


@torch.no_grad()
def mesh_transfer(mesh, sdf, transfer, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1)):
    """The radiance transfer of ``mesh``'s vertices, traced through the volume ``sdf`` the mesh was cut from (with
    ``clean``: the cleaned one) at ``level`` in the box [b_min, b_max], as ``transfer`` (a ``Transfer``) says: (prt
    [V,9] f32, mask int64 [V, D/64]: bit d & 63 of word d >> 6 is set where direction d faces away from the surface and
    reaches the box's edge (or the end of its reach) unoccluded).  The mesh needs normals.  No host sync."""
    who = "mesh_transfer"
    if not isinstance(transfer, Transfer):
        raise ValueError("%s: transfer must be a recon.Transfer, got %r" % (who, type(transfer).__name__))
    if mesh.normals is None:
        raise ValueError("%s: the rays start along the mesh's normals, and the mesh has none" % who)
    vol = ops._cubic_volume(sdf, who)
    r = int(vol.shape[0])
    bias_w, step_w, steps = transfer.rays(r, b_min, b_max)
    verts, normals = ops._f32c(mesh.verts), ops._f32c(mesh.normals)
    counts = _shape_counts([(verts, mesh.faces)])[0]
    dirs, basis = transfer.tables(verts.device)
    if verts.shape[0] == 0:  # nothing to trace: nothing is enqueued
        return (torch.empty((0, 9), dtype=torch.float32, device=verts.device),
                torch.empty((0, transfer.directions // 64), dtype=torch.int64, device=verts.device))
    bits = ops.volume_bits_raw(vol, level)
    mask, prt = ops.mesh_transfer_raw(verts, normals, counts, bits, r, b_min, b_max, dirs, basis, transfer.weight,
                                      bias_w, step_w, steps)
    return prt, mask


LIGHTING_FRAMES = ("world", "camera")


class Lighting:
    """How the subject is lit per pixel (the reference's spherical-harmonic lighting model, its SH shader and
    ShRender; mp_picture_light in include/monoport_hip.h): shading = the nine second-order SH basis values at the
    pixel's normal times ``sh`` [9,3] (coefficient, rgb), plus -- ``direct``: None, or a (direction the light travels,
    rgb) pair; the direction is normalised here in float64 -- max(-direction . normal, 0) * rgb, raised to 1 / ``gamma``
    (1.0, the default: nothing, and the bit-exact form; the reference uses 2.2); the picture is clamp(albedo * shading,
    0, 1).  ``frame``: "world" (SH at the world normal) or "camera" (SH at the normal turned by the 3x3 of each view's
    calib and normalised again, the reference's ModelMat * a_Normal); the direct term is always on the world normal.
    ``albedo``: None (the albedo is the picture's own colours: ``shade="colors"`` / ``"netC"``) or a constant (r, g, b)
    "clay" for ``shade="normals"``.  ``self_shadow``: None, or a bias >= 0: the scene's ``Light`` then also shadows the
    subject itself -- its own shadow map looked up at its own surface, nearer by more than the bias -- and the shade
    takes the direct term away (1 = fully occluded), the SH term stays.  ``transfer``: None, or a ``Transfer``: the SH
    term is then self-occluded -- the nine basis values at the normal give way to the radiance transfer of each vertex
    (``mesh_transfer`` + ``with_transfer``: the cosine lobe masked by what the body itself hides, the reference's PRT
    shaders), interpolated over the picture; every mesh rendered must carry ``.transfer`` and ``frame`` must be
    "world".  Everything is validated here; a Lighting holds host values only."""

    def __init__(self, sh, direct=None, gamma=1.0, frame="world", albedo=None, self_shadow=None, transfer=None):
        who = "Lighting"
        if transfer is not None and not isinstance(transfer, Transfer):
            raise ValueError("%s: transfer must be None or a recon.Transfer, got %r" % (who, type(transfer).__name__))
        if transfer is not None and frame == "camera":
            raise ValueError("%s: transfer is traced in the world frame; frame='camera' would need the band rotation "
                             "of the coefficients, which is not built" % who)
        self.transfer = transfer
        if direct is not None:
            try:
                direction, rgb = direct
                d = np.asarray(direction, np.float64).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError("%s: direct must be None or a (direction, rgb) pair, got %r" % (who, direct)) from None
            if d.shape != (3,) or not np.isfinite(d).all() or not np.linalg.norm(d) > 0:
                raise ValueError("%s: direct's direction must be three finite values, not all zero, got %r"
                                 % (who, direction))
            direct = ((d / np.linalg.norm(d)).astype(np.float32), rgb)
        self.sh, self.direct_dir, self.direct_rgb, self.gamma, self.albedo = ops.light_params(who, sh, direct, gamma,
                                                                                             albedo)
        self.direct = None if direct is None else (self.direct_dir, self.direct_rgb)
        if not isinstance(frame, str) or frame not in LIGHTING_FRAMES:
            raise ValueError("%s: frame must be one of %s, got %r" % (who, list(LIGHTING_FRAMES), frame))
        self.frame = frame
        if self_shadow is not None:
            if isinstance(self_shadow, bool) or not isinstance(self_shadow, (int, float, np.integer, np.floating)):
                raise ValueError("%s: self_shadow must be None or a bias >= 0, got %r" % (who, self_shadow))
            self_shadow = float(self_shadow)
            if not (np.isfinite(self_shadow) and self_shadow >= 0):
                raise ValueError("%s: self_shadow must be None or a finite bias >= 0, got %r" % (who, self_shadow))
        self.self_shadow = self_shadow

    @classmethod
    def ambient(cls, rgb, **kw):
        """Light of the same colour from everywhere: only coefficient 0 is set, so that the shading is ``rgb`` exactly
        wherever rgb / c4 * c4 rounds back to rgb -- the coefficient is the f32 nearest to rgb / c4, moved by an ulp
        where that product misses."""
        rgb = ops._finite_floats("Lighting.ambient", "rgb", rgb, (3,))
        c4 = np.float32(0.886227)
        coeff = (rgb / c4).astype(np.float32)
        for c in range(3):  # H0 * coeff == rgb on the bits, if a neighbour of the quotient gives it
            for cand in (coeff[c], np.nextafter(coeff[c], np.float32(np.inf)), np.nextafter(coeff[c], np.float32(-np.inf))):
                if np.float32(c4 * cand) == rgb[c]:
                    coeff[c] = cand
                    break
        sh = np.zeros((9, 3), np.float32)
        sh[0] = coeff
        return cls(sh, **kw)


def _check_lighting(who, lighting, shade, meshes, scene_light):
    """``lighting`` against the shade, the meshes (None entries skipped) and the scene's light, before anything is
    enqueued."""
    _check_lighting_options(who, lighting, shade, not any(m is not None and m.normals is None for m in meshes),
                            scene_light)
    if lighting.transfer is not None:
        for m in meshes:
            if m is None:
                continue
            t = getattr(m, "transfer", None)
            if not torch.is_tensor(t) or t.dim() != 2 or tuple(t.shape) != (m.verts.shape[0], 9):
                raise ValueError("%s: lighting.transfer needs every mesh's radiance transfer [V,9]: "
                                 "with_transfer(mesh, mesh_transfer(...)[0])" % who)


def _check_lighting_options(who, lighting, shade, has_normals, scene_light):
    """``_check_lighting`` for a caller that knows whether its meshes have normals (a slot's mesh options)."""
    if not isinstance(lighting, Lighting):
        raise ValueError("%s: lighting must be a recon.Lighting, got %r" % (who, type(lighting).__name__))
    if shade is None:
        raise ValueError("%s: lighting shades an image; shade=None renders none" % who)
    if shade == "normals" and lighting.albedo is None:
        raise ValueError("%s: shade='normals' is lit as clay: lighting needs a constant albedo=(r, g, b)" % who)
    if shade != "normals" and lighting.albedo is not None:
        raise ValueError("%s: lighting.albedo is the clay of shade='normals'; shade=%r has its own colours"
                         % (who, shade))
    if not has_normals:
        raise ValueError("%s: lighting needs the mesh's normals, and the mesh has none" % who)
    if lighting.transfer is not None and lighting.frame == "camera":
        raise ValueError("%s: lighting.transfer is traced in the world frame; frame='camera' is not built" % who)
    if lighting.self_shadow is not None and scene_light is None:
        raise ValueError("%s: lighting.self_shadow looks the subject up in the shadow map of the scene's light; there "
                         "is no scene light" % who)


class Scene:
    """A textured triangle mesh behind the subject, on the device (RTL/scene.py's floor): ``verts`` [V,3] f32, ``faces``
    [F,3] int, ``uv`` [V,2] f32 per vertex, ``texture`` [Ht,Wt,3] -- uint8 (divided by 255 into f32) or f32; tensors or
    arrays.  ``wrap``: "repeat" or "clamp".  ``flip_v`` (the default): the texture's rows are flipped once at upload,
    as the reference's ``Render.set_texture`` does, so OBJ / GL uv (v = 0 at the bottom of the picture file) need no
    change; without it v = 0 is row 0.  The mip pyramid is built once here (``ops.texture_mips``; ``levels`` None = the
    full chain).  Holds ``verts``, ``faces``, ``counts`` (int32 [2] on the device), ``attr`` [V,3] = (u, v, 0),
    ``pyramid``, ``tex_size`` (Ht, Wt), ``levels``, ``wrap``, ``light``.  ``light``: None, or the ``Light`` under which
    the subject casts its shadow on this scene (``render_mesh_many_in_scene``, ``render_scene(casters=)``, a slot's
    pictures).  The light belongs to the scene: the picture options of a slot do not change."""

    def __init__(self, verts, faces, uv, texture, wrap="repeat", flip_v=True, levels=None, device="cuda", light=None):
        if light is not None:
            _check_light("Scene", light)
        self.light = light
        dev = torch.device(device)
        ops._named_mode("Scene", "wrap", ops.WRAP_MODES, wrap)
        verts = torch.as_tensor(np.asarray(verts.detach().cpu()) if torch.is_tensor(verts) else np.asarray(verts))
        faces = torch.as_tensor(np.asarray(faces.detach().cpu()) if torch.is_tensor(faces) else np.asarray(faces))
        uv = torch.as_tensor(np.asarray(uv.detach().cpu()) if torch.is_tensor(uv) else np.asarray(uv))
        tex = texture.detach().cpu() if torch.is_tensor(texture) else torch.as_tensor(np.ascontiguousarray(texture))
        if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError("Scene: verts [V,3] and faces [F,3], got %s and %s" % (tuple(verts.shape), tuple(faces.shape)))
        if tuple(uv.shape) != (verts.shape[0], 2):
            raise ValueError("Scene: uv must be [%d,2], one per vertex, got %s" % (verts.shape[0], tuple(uv.shape)))
        if tex.dim() != 3 or tex.shape[2] != 3 or tex.dtype not in (torch.uint8, torch.float32):
            raise ValueError("Scene: texture must be uint8 or float32 [Ht,Wt,3], got %s %s" % (tex.dtype, tuple(tex.shape)))
        ht, wt = int(tex.shape[0]), int(tex.shape[1])
        self.levels = ops.texture_levels(ht, wt) if levels is None else int(levels)
        ops.texture_pyramid_floats(ht, wt, self.levels)  # refuses a size or a level count out of range
        if tex.dtype == torch.uint8:
            tex = tex.to(torch.float32) / 255.0
        if flip_v:
            tex = tex.flip(0)
        attr = torch.zeros((verts.shape[0], 3), dtype=torch.float32)
        attr[:, :2] = uv.to(torch.float32)
        self.wrap, self.tex_size = wrap, (ht, wt)
        self.verts = verts.to(torch.float32).contiguous().to(dev)
        self.faces = faces.to(torch.int32).contiguous().to(dev)
        self.attr = attr.to(dev)
        self.counts = torch.tensor([verts.shape[0], faces.shape[0]], dtype=torch.int32).to(dev)
        self.texture = tex.contiguous().to(dev)  # level 0 as uploaded (after the flip)
        self.pyramid, _ = ops.texture_mips(self.texture, self.levels)

    @classmethod
    def from_packed(cls, vert_data, uv_data, texture, **kw):
        """The reference's layout (RTL/scene.py ``_load_floor``): ``vert_data`` [3F,3] and ``uv_data`` [3F,2], three
        rows per face; the faces are ``arange(3F).reshape(F, 3)``."""
        n = int(np.shape(vert_data)[0])
        if n % 3 or n == 0:
            raise ValueError("Scene.from_packed: vert_data holds three rows per face, got %d rows" % n)
        return cls(vert_data, np.arange(n, dtype=np.int32).reshape(-1, 3), uv_data, texture, **kw)


def _check_scene(who, scene):
    if not isinstance(scene, Scene):
        raise ValueError("%s: scene must be a recon.Scene, got %r" % (who, type(scene).__name__))


def _camera_sets(who, calibs, n, what="pictures"):
    if isinstance(calibs, (list, tuple)):
        if len(calibs) != n:
            raise ValueError("%s: %d %s, %d camera sets" % (who, n, what, len(calibs)))
        return list(calibs)
    return [calibs] * n


@torch.no_grad()
def shadow_map(meshes, light, device=None):
    """Per mesh the shadow map (depth [Hs,Ws] f32, face [Hs,Ws] int32) of ``light``: the rasteriser's depth and face
    ids of the mesh under the light's camera, without an image -- through the clipped, perspective-correct call where
    the light has a ``near``.  A ``None`` mesh gives an all-uncovered map (depth +0.0, face -1), which shadows nothing.
    One set of launches per ops.MAX_FRAMES meshes; no host sync.  ``device``: where the maps of ``None`` meshes live
    (None: the first mesh's, "cuda" without any)."""
    who = "shadow_map"
    _check_light(who, light)
    meshes = list(meshes)
    idx = [i for i, m in enumerate(meshes) if m is not None]
    if device is None:
        device = meshes[idx[0]].verts.device if idx else "cuda"
    out = [None] * len(meshes)
    if idx:
        for i, depth, face in zip(idx, *_shadow_maps(who, _mesh_subjects(who, [meshes[i] for i in idx]), light)):
            out[i] = (depth, face)
    return [_uncovered_map(light, device) if m is None else m for m in out]


def _uncovered_map(light, device):
    """The (depth, face) shadow map of no caster at all: it shadows nothing."""
    return (torch.zeros(light.res, dtype=torch.float32, device=device),
            torch.full(light.res, -1, dtype=torch.int32, device=device))


def _shadow_maps(who, subjects, light, out=None):
    """The shadow maps of ``subjects`` (a ``_Subjects``) under ``light`` -> (depths, faces), per subject a [Hs,Ws]: one
    pass of the rasteriser under the light's camera without an image, clipped and perspective-correct where the light
    has a ``near``.  ``out``: None, or the caller's (depth [n,Hs,Ws], face [n,Hs,Ws])."""
    s, n = subjects, len(subjects.verts)
    ras = ops.raster(who, light.res, light.projection, light.nearest, 1.0, light.near, light.near is not None)
    raws = ops._attr_pass(who, s.verts, s.faces, s.counts, None, [light.calib] * n, ras,
                          None if out is None else (None, out[0].unsqueeze(1), out[1].unsqueeze(1)), s.capacity)
    return [r[1][0] for r in raws], [r[2][0] for r in raws]


@torch.no_grad()
def shade_shadow(picture, positions, maps, light):
    """The shadow of ``maps`` = (depth, face) (``shadow_map`` of the caster under ``light``) on ``picture`` (image
    [...,3] f32, depth, face [...] int32; a ``MeshRender`` or a tuple), whose ``positions`` [...,3] f32 hold the
    world-space point of every pixel (a render with the vertices as the attribute).  The generic call: the caller may
    shade the subject's own picture with its own map and a ``bias`` (self-shadowing).  Returns (image, shade): fresh
    tensors, the image's bits unchanged wherever the shade is 0.  Defined bit for bit in include/monoport_hip.h
    (mp_picture_shadow).  No host sync."""
    _check_light("shade_shadow", light)
    return ops.picture_shadow_batch([picture[0].contiguous()], [positions.contiguous()], [picture[2].contiguous()],
                                    [maps[0]], [maps[1]], light.calib, light.projection, light.nearest, light.bias,
                                    light.radius, light.strength, with_shade=True, who="shade_shadow")[0]


@torch.no_grad()
def light_picture(picture, normals, lighting, calibs=None, visibility=None):
    """``picture`` (image [...,3] f32 or None, depth, face [...] int32; a ``MeshRender`` or a tuple) lit by ``lighting``
    at the ``normals`` [...,3] f32 of its pixels (a render with the mesh's normals as the attribute and the paint (1, 0,
    -inf, inf)): the generic call of ``render_mesh(lighting=)``.  The image is the albedo; with a constant
    ``lighting.albedo`` it is not read and may be None.  ``calibs``: the picture's cameras ([4,4] / [3,4] for a picture
    [H,W,3], [n_views, ...] for [n_views,H,W,3]), needed for ``frame="camera"``; ``visibility``: None, or the shade
    [...] of ``shade_shadow`` (1 = the direct light is occluded; ``lighting.self_shadow`` is not looked at here).
    Returns (image, shading): fresh tensors [...,3]; uncovered pixels keep the albedo's bits (1.0 without an image) and
    have shading 0.  Defined bit for bit in include/monoport_hip.h (mp_picture_light).  No host sync."""
    who = "light_picture"
    if not isinstance(lighting, Lighting):
        raise ValueError("%s: lighting must be a recon.Lighting, got %r" % (who, type(lighting).__name__))
    image, face = picture[0], picture[2]
    if (image is None) == (lighting.albedo is None):
        raise ValueError("%s: the albedo is either the picture's image or lighting.albedo, not %s"
                         % (who, "neither" if image is None else "both"))
    nv = int(normals.shape[0]) if normals.dim() == 4 else 1
    mats = None
    if lighting.frame == "camera":
        if calibs is None:
            raise ValueError("%s: frame='camera' needs the picture's calibs" % who)
        mats = ops.normal_mats_of(who, calibs)
        if mats.shape[0] != nv:
            raise ValueError("%s: a picture of %d views, %d cameras" % (who, nv, mats.shape[0]))
    return ops.picture_light_batch([normals.contiguous()], [face.contiguous()],
                                   None if image is None else [image.contiguous()], lighting.sh, lighting.direct,
                                   lighting.gamma, mats, None if visibility is None else [visibility.contiguous()],
                                   lighting.albedo, nv, with_shading=True, who=who)[0]


class Jpeg:
    """How pictures are encoded on the device (mp_picture_jpeg in include/monoport_hip.h: baseline JFIF with restart
    intervals, byte for byte this library's own definition; what the reference's server loop does with cv2.imencode).
    ``quality``: 1..100, scaled as the IJG library scales the Annex K tables; ``subsampling``: "420" (chroma 2 x 2, the
    default) or "444"; ``restart``: MCUs per restart interval, 1..65535, or None = the MCUs of one MCU row (the unit of
    parallel work; the marker and the padding cost a few percent of the file).  ``capacity``: bytes reserved per picture,
    at least the 629-byte header; None = ``4096 + H * W * 3 // 4`` -- a quarter of the 8-bit picture, several times a
    typical file at quality 90 --, never more than ``ops.jpeg_max_bytes``.  A file that does not fit is reported by the
    device and encoded again alone at its exact size (``encode_jpeg``, ``FrameSlot.jpegs``): the capacity never
    changes the bytes.  Everything is validated here; a Jpeg holds host values only."""

    def __init__(self, quality=90, subsampling="420", restart=None, capacity=None):
        who = "Jpeg"
        self.quality, sub, restart = ops.jpeg_params(who, quality, subsampling, restart)
        self.subsampling = {v: k for k, v in ops.JPEG_SUBSAMPLINGS.items()}[sub]
        self.restart = restart or None
        if capacity is not None:
            if (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer))
                    or not ops.JPEG_HEADER_BYTES <= capacity <= 2 ** 31):
                raise ValueError("%s: capacity must be None or an int in %d..2^31 bytes, got %r"
                                 % (who, ops.JPEG_HEADER_BYTES, capacity))
            capacity = int(capacity)
        self.capacity = capacity

    def capacity_for(self, h, w):
        """Bytes reserved per [h,w,3] picture."""
        if self.capacity is not None:
            return self.capacity
        return min(4096 + h * w * 3 // 4, ops.jpeg_max_bytes(h, w, self.subsampling, self.restart))


def picture_u8(image):
    """``image`` float32 [...,3] (a picture of this module: values in [0, 1]) -> uint8 of the same shape on the device:
    (int)(clamp(x, 0, 1) * 255 + 0.5), a NaN gives 0 -- the reference's np.uint8 of its pictures, and step 1 of the
    JPEG definition in include/monoport_hip.h.  For a display or a video encoder.  No host sync."""
    return ops.picture_u8_raw(image)


def _jpeg_images(who, pictures):
    """(images [n,H,W,3] contiguous float32, whether ``pictures`` was one [H,W,3] picture)."""
    image = pictures.image if hasattr(pictures, "image") and not torch.is_tensor(pictures) else pictures
    if image is None:
        raise ValueError("%s: the picture has no image (it was rendered with shade=None)" % who)
    if not torch.is_tensor(image) or image.dtype != torch.float32 or image.dim() not in (3, 4) or image.shape[-1] != 3:
        raise ValueError("%s: pictures must be a MeshRender, a ScenePicture or a float32 tensor [H,W,3] / [n,H,W,3]" % who)
    return (image[None] if image.dim() == 3 else image).contiguous(), image.dim() == 3


def _collect_files(who, out, info, again):
    """The files that an encoding call left in ``out`` [n,capacity] under the HOST rows ``info`` [n,2]: one copy of the
    used prefixes; a picture that overflowed is encoded again alone, ``again(i, size)`` -> (out, info) at the size the
    device reported, which gives the bytes a sufficient capacity would have given."""
    fits = [i for i in range(len(info)) if not info[i][1]]
    used = max([int(info[i][0]) for i in fits], default=0)
    host = out[:len(info), :used].cpu().numpy() if fits else None
    files = []
    for i in range(len(info)):
        size = int(info[i][0])
        if info[i][1]:
            bytes_again, again_info = again(i, size)
            row = again_info.cpu().numpy()[0]
            if tuple(row) != (size, 0):
                raise RuntimeError("%s: a picture of %d bytes gave %s at that capacity" % (who, size, tuple(row)))
            files.append(bytes_again[0].cpu().numpy().tobytes())
        else:
            files.append(host[i, :size].tobytes())
    return files


def _collect_jpegs(images, out, info, jpeg):
    """``_collect_files`` for what mp_picture_jpeg left of ``images`` [n,H,W,3]."""
    return _collect_files("encode_jpeg", out, info, lambda i, size: ops.picture_jpeg_raw(
        images[i:i + 1], jpeg.quality, jpeg.subsampling, jpeg.restart, capacity=size))


def encode_jpeg(pictures, jpeg=None):
    """The JPEG files of ``pictures`` (a ``MeshRender`` / ``ScenePicture`` with an image, or a float32 image tensor
    [H,W,3] or [n,H,W,3] on the device) under ``jpeg`` (a ``Jpeg``; None: its defaults), encoded on the device:
    ``bytes`` for one [H,W,3] picture, a list of ``bytes`` for [n,H,W,3].  One device-to-host copy of the sizes, then
    one of the used prefixes; a picture whose file exceeded ``jpeg``'s capacity is encoded again alone at the size the
    device reported.  Any JPEG decoder reads the files; tests/jpeg_ref.py restates them byte for byte."""
    who = "encode_jpeg"
    jpeg = Jpeg() if jpeg is None else jpeg
    if not isinstance(jpeg, Jpeg):
        raise ValueError("%s: jpeg must be a recon.Jpeg, got %r" % (who, type(jpeg).__name__))
    images, single = _jpeg_images(who, pictures)
    out, info = ops.picture_jpeg_raw(images, jpeg.quality, jpeg.subsampling, jpeg.restart,
                                     capacity=jpeg.capacity_for(int(images.shape[1]), int(images.shape[2])))
    files = _collect_jpegs(images, out, info.cpu().numpy(), jpeg)
    return files[0] if single else files


class Png:
    """How pictures are encoded losslessly on the device (mp_picture_png in include/monoport_hip.h: this library's own
    deflate inside a standard PNG container, byte for byte defined; the reference's .png files).  ``filter``: "none",
    "sub", "up", "average", "paeth", or "adaptive" (per scanline the smallest sum of absolute values, the default).
    ``alpha``: None = 8-bit RGB; "coverage" = 8-bit RGBA with a ``ResolvedPicture``'s coverage (``samples`` > 1);
    "subject" = RGBA with 1.0 where the mask says subject (2) -- without a mask where a face shows -- else 0.0.
    ``unmatte``: None, or the background value the pictures were rendered over: the colour then becomes the subject's
    own, (c - (1 - a) * unmatte) / a, so that the file composites over anything.  ``plane="depth"`` with
    ``depth_range=(lo, hi)`` writes the depth picture as 16-bit grey, (d - lo) / (hi - lo) clamped to [0, 1] times 65535,
    and refuses alpha.  ``capacity``: bytes reserved per picture, at least 57; None = ``4096 + raw // 2`` with raw the
    bytes of the samples, never more than ``ops.png_max_bytes``.  A file that does not fit is reported by the device
    and encoded again alone at its exact size: the capacity never changes the bytes.  Everything is validated here; a
    Png holds host values only."""

    def __init__(self, filter="adaptive", alpha=None, unmatte=None, plane="image", depth_range=None, capacity=None):
        who = "Png"
        if plane not in ("image", "depth"):
            raise ValueError("%s: plane must be 'image' or 'depth', got %r" % (who, plane))
        if alpha not in (None, "coverage", "subject"):
            raise ValueError("%s: alpha must be None, 'coverage' or 'subject', got %r" % (who, alpha))
        lo, scale = 0.0, 1.0
        if plane == "depth":
            if alpha is not None or unmatte is not None:
                raise ValueError("%s: plane='depth' is 16-bit grey: it takes no alpha and no unmatte" % who)
            ok = isinstance(depth_range, (tuple, list)) and len(depth_range) == 2
            if ok:
                lo, hi = (ops._finite_float(who, "depth_range", v) for v in depth_range)
                with np.errstate(all="ignore"):
                    scale = float(np.float32(1) / (np.float32(hi) - np.float32(lo)))
                ok = hi > lo and np.isfinite(scale)
            if not ok:
                raise ValueError("%s: plane='depth' needs depth_range=(lo, hi) with finite lo < hi, got %r"
                                 % (who, depth_range))
            depth_range = (lo, hi)
        elif depth_range is not None:
            raise ValueError("%s: depth_range goes with plane='depth'" % who)
        if unmatte is not None and alpha is None:
            raise ValueError("%s: unmatte needs an alpha" % who)
        self.format = "gray16" if plane == "depth" else ("rgb8" if alpha is None else "rgba8")
        _, flt, self.lo, self.scale, _, bg = ops.png_params(who, self.format, filter, lo, scale, unmatte)
        self.filter = {v: k for k, v in ops.PNG_FILTERS.items()}[flt]
        self.alpha, self.plane, self.depth_range = alpha, plane, depth_range
        self.unmatte = None if unmatte is None else bg
        if capacity is not None:
            if (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer))
                    or not ops.PNG_MIN_BYTES <= capacity <= 2 ** 31):
                raise ValueError("%s: capacity must be None or an int in %d..2^31 bytes, got %r"
                                 % (who, ops.PNG_MIN_BYTES, capacity))
            capacity = int(capacity)
        self.capacity = capacity

    def capacity_for(self, h, w):
        """Bytes reserved per [h,w] picture."""
        if self.capacity is not None:
            return self.capacity
        raw = h * w * {"rgb8": 3, "rgba8": 4, "gray16": 2}[self.format]
        return min(4096 + raw // 2, ops.png_max_bytes(h, w, self.format))


def picture_u16(depth, lo=0.0, hi=1.0):
    """``depth`` float32 [...] -> uint16 of the same shape on the device: (int)(clamp((d - lo) / (hi - lo), 0, 1) * 65535
    + 0.5) with the scale 1 / (hi - lo) taken once in f32, a NaN gives 0: the samples of ``Png(plane="depth",
    depth_range=(lo, hi))``.  No host sync."""
    p = Png(plane="depth", depth_range=(lo, hi))
    return ops.picture_u16_raw(depth, p.lo, p.scale)


def picture_rgba8(image, alpha, unmatte=None):
    """``image`` float32 [...,3] and ``alpha`` float32 [...] -> uint8 [...,4] on the device: the samples of an RGBA
    ``Png`` (``unmatte``: None, or the background the colour is freed of).  No host sync."""
    return ops.picture_rgba8_raw(image, alpha, unmatte)


def _subject_alpha(mask, face, out=None):
    """1.0 where the mask says subject (2) -- without a mask where a face shows --, else 0.0: one op on the stream."""
    if out is None:
        out = torch.empty((face if mask is None else mask).shape, dtype=torch.float32,
                          device=(face if mask is None else mask).device)
    return torch.ge(face, 0, out=out) if mask is None else torch.eq(mask, 2, out=out)


def _png_inputs(who, pictures, png, alpha):
    """(planes [n,H,W,3] or [n,H,W] contiguous float32, alpha [n,H,W] or None, whether ``pictures`` was one picture)."""
    plain = torch.is_tensor(pictures)
    depth = png.plane == "depth"
    if plain:
        plane = pictures
    else:
        plane = getattr(pictures, "depth" if depth else "image", None) if hasattr(pictures, "face") else pictures
        if plane is None and hasattr(pictures, "face"):
            raise ValueError("%s: the picture has no image (it was rendered with shade=None)" % who)
    dims = (2, 3) if depth else (3, 4)
    if (not torch.is_tensor(plane) or plane.dtype != torch.float32 or plane.dim() not in dims
            or (not depth and plane.shape[-1] != 3)):
        raise ValueError("%s: pictures must be a MeshRender, a ScenePicture, a ResolvedPicture or a float32 tensor %s"
                         % (who, "[H,W] / [n,H,W]" if depth else "[H,W,3] / [n,H,W,3]"))
    single = plane.dim() == dims[0]
    if alpha is not None:
        if not plain or png.alpha is None:
            raise ValueError("%s: the alpha keyword goes with a plain image tensor and a Png with an alpha" % who)
        want = tuple(plane.shape[:-1])
        if (not torch.is_tensor(alpha) or alpha.dtype != torch.float32 or tuple(alpha.shape) != want
                or alpha.device != plane.device):
            raise ValueError("%s: alpha must be a float32 tensor %s on %s" % (who, want, plane.device))
    elif png.alpha is not None:
        if plain:
            raise ValueError("%s: a plain tensor needs the alpha keyword for a Png with alpha=%r" % (who, png.alpha))
        if png.alpha == "coverage":
            alpha = getattr(pictures, "coverage", None)
            if alpha is None:
                raise ValueError("%s: alpha='coverage' needs a ResolvedPicture (samples > 1)" % who)
        else:
            alpha = _subject_alpha(getattr(pictures, "mask", None), pictures.face)
    lead = (lambda t: (t[None] if single else t).contiguous())
    return lead(plane), None if alpha is None else lead(alpha), single


def _png_raw(png, planes, alpha, **kw):
    return ops.picture_png_raw(planes, alpha, png.format, png.filter, png.lo, png.scale, png.unmatte, **kw)


def encode_png(pictures, png=None, alpha=None):
    """The PNG files of ``pictures`` (what ``encode_jpeg`` takes, or a ``ResolvedPicture``; with ``plane="depth"`` the
    depth picture, or a float32 tensor [H,W] / [n,H,W]) under ``png`` (a ``Png``; None: its defaults), encoded on the
    device: ``bytes`` for one picture, a list of ``bytes`` for n.  ``alpha``: for a plain image tensor and a ``Png`` with
    an alpha, the float32 [H,W] / [n,H,W] tensor that is it.  One device-to-host copy of the sizes, then one of the used
    prefixes; a picture whose file exceeded ``png``'s capacity is encoded again alone at the size the device reported.
    zlib and any PNG reader give back exactly the 8-bit or 16-bit samples; tests/png_ref.py restates the files byte for
    byte."""
    who = "encode_png"
    png = Png() if png is None else png
    if not isinstance(png, Png):
        raise ValueError("%s: png must be a recon.Png, got %r" % (who, type(png).__name__))
    planes, alpha, single = _png_inputs(who, pictures, png, alpha)
    out, info = _png_raw(png, planes, alpha, capacity=png.capacity_for(int(planes.shape[1]), int(planes.shape[2])))
    files = _collect_files(who, out, info.cpu().numpy(), lambda i, size: _png_raw(
        png, planes[i:i + 1], None if alpha is None else alpha[i:i + 1], capacity=size))
    return files[0] if single else files


class Atlas:
    """The texture of a mesh file (mp_mesh_atlas in include/monoport_hip.h): a square picture of side ``size`` (a power
    of two in 64..4096) cut into cells of side ``cell`` (4..64), two faces per cell, each face a right triangle of its
    own with a gutter, so that a viewer's bilinear lookup never leaves the face.  ``faces`` = 2 (size // cell)^2 is what
    the atlas holds; the detail is ``cell`` texels along a face's legs whatever the mesh density.  ``filter``: the PNG
    filter of the image (``Png``'s); ``background``: the colour of texels no face owns; ``png_capacity``: bytes
    reserved per image, None = ``Png``'s own default for a picture of that size.  Everything is validated here; an
    Atlas holds host values only."""

    def __init__(self, size=1024, cell=8, filter="adaptive", background=0.5, png_capacity=None):
        who = "Atlas"
        self.size, self.cell = ops.atlas_params(who, size, cell)
        self.background = ops._finite_float(who, "background", background)
        self.png = Png(filter=filter, capacity=png_capacity)
        self.filter = self.png.filter
        self.faces = ops.atlas_faces(self.size, self.cell)

    def png_capacity(self):
        """Bytes reserved per image."""
        return self.png.capacity_for(self.size, self.size)


def _check_colour_field(who, colors, points):
    """``colors(points)`` of ``bake_texture``: raw predictions [3,K] f32 for points [3,K]."""
    got = colors(points)
    if (not torch.is_tensor(got) or got.dtype != torch.float32 or got.shape != points.shape
            or got.device != points.device):
        raise ValueError("%s: colors(points [3,K]) must return a float32 tensor [3,K] on the points' device, got %r"
                         % (who, tuple(got.shape) if torch.is_tensor(got) else type(got).__name__))
    return got.contiguous()


def _atlas_query(who, meshes, netC, feat_tensors_C, calib_tensors, view, colors):
    """The counted colour query ``(points, counts) -> predictions`` of ``bake_texture`` / ``encode_glb``: netC on the
    meshes' own maps and calibrations, as ``render_mesh_many(shade="netC")`` binds it, or the caller's ``colors``."""
    if (netC is None) == (colors is None):
        raise ValueError("%s: a texture is baked from netC= (with its feature maps and calibrations) or from colors=, "
                         "one of the two" % who)
    if colors is not None:
        if not callable(colors) or feat_tensors_C is not None or calib_tensors is not None or view is not None:
            raise ValueError("%s: colors= is a callable points [3,K] -> [3,K] and takes no maps, calibrations or view"
                             % who)
        return lambda pts, counts: [_check_colour_field(who, colors, p) for p in pts]
    _check_colour_view(who, netC, view)
    if feat_tensors_C is None or calib_tensors is None:
        raise ValueError("%s: netC needs feat_tensors_C and calib_tensors" % who)
    if len(feat_tensors_C) != len(meshes) or len(calib_tensors) != len(meshes):
        raise ValueError("%s: %d meshes, %d feature sets, %d calibrations"
                         % (who, len(meshes), len(feat_tensors_C), len(calib_tensors)))
    bindings = _bind_netC(who, netC, [(feat_tensors_C[i], calib_tensors[i], m.verts.device)
                                      for i, m in enumerate(meshes)], view)
    return lambda pts, counts: _counted_colours(bindings, pts, counts, view=view or 0)


def _bake(who, subjects, atlas, query, out=None):
    """THE baked texture of a set of subjects (a ``_Subjects``: a call's meshes or a slot's chains), for
    ``bake_texture``, ``encode_glb`` and a slot alike: ``ops.mesh_atlas_raw_batch`` -- the G-buffer in texture space --
    then ``ops.paint_netc``, the body of ``shade="netC"``: the covered texels' points, ``query``, the paint in place.
    -> (images, face_ids, infos), lists with one entry per subject.  ``out``: None (fresh tensors), or a dict of the
    caller's buffers, each [n, ...]: ``face``, ``image``, ``info`` and ``lists`` = (points, pixels, count)."""
    s, out = subjects, out or {}
    buffers = (out["face"], out["image"], out["info"]) if "face" in out else None
    if s.capacity is None or all(v.shape[0] == s.verts[0].shape[0] for v in s.verts) \
            and all(f.shape[0] == s.faces[0].shape[0] for f in s.faces):
        made = ops.mesh_atlas_raw_batch(s.verts, s.faces, s.counts, atlas.size, atlas.cell, atlas.background, buffers)
    else:  # meshes cut to their own sizes: one launch each
        made = [ops.mesh_atlas_raw(v, f, c, atlas.size, atlas.cell, atlas.background,
                                   None if buffers is None else tuple(b[i] for b in buffers))
                for i, (v, f, c) in enumerate(zip(s.verts, s.faces, s.counts))]
    faces, images = [m[0] for m in made], [m[1] for m in made]
    ops.paint_netc(who, faces, images, query, out.get("lists"))
    return images, faces, [m[2] for m in made]


def _texture_meshes(who, meshes):
    single = isinstance(meshes, Mesh)
    meshes = [meshes] if single else list(meshes)
    for k, m in enumerate(meshes):
        if not isinstance(m, Mesh):
            raise ValueError("%s: mesh %d is not a recon.Mesh but %r" % (who, k, type(m).__name__))
    return meshes, single


@torch.no_grad()
def bake_texture(meshes, atlas, netC=None, feat_tensors_C=None, calib_tensors=None, view=None, colors=None):
    """The texture of ``meshes`` (a ``Mesh`` on the device, or a list of them) in ``atlas`` (an ``Atlas``), baked on
    the device: (image [n,A,A,3] f32, face_id [n,A,A] int32) -- without the leading n for a single ``Mesh``.  Every
    texel a face owns holds ``netC.query(point) * 0.5 + 0.5`` at the surface point under it (gutter texels: the face's
    plane extrapolated), every other texel ``atlas.background`` and face id -1: what ``render_mesh(shade="netC")`` is
    for one camera, for the whole surface.  ``netC`` with ``feat_tensors_C`` / ``calib_tensors`` (for a list one entry per
    mesh, as ``render_mesh_many`` takes them; for a single ``Mesh`` its own, as ``render_mesh``'s ``feat_tensor_C`` /
    ``calib_tensor``) and ``view``; or ``colors``: a callable ``points [3,K] -> [3,K]`` raw
    predictions that takes the place of the netC query (a colour field of the caller's own; only the covered texels'
    values are used).  Faces beyond ``atlas.faces`` are laid out nowhere (``encode_glb`` refuses such a mesh).  One
    atlas launch, the point lists, one counted query, one paint: no host sync."""
    who = "bake_texture"
    if not isinstance(atlas, Atlas):
        raise ValueError("%s: atlas must be a recon.Atlas, got %r" % (who, type(atlas).__name__))
    meshes, single = _texture_meshes(who, meshes)
    if single and feat_tensors_C is not None and calib_tensors is not None:  # a single mesh's own, as render_mesh's
        feat_tensors_C, calib_tensors = [feat_tensors_C], [calib_tensors]
    query = _atlas_query(who, meshes, netC, feat_tensors_C, calib_tensors, view, colors)
    if not meshes:
        return []
    images, faces, _ = _bake(who, _mesh_subjects(who, meshes), atlas, query)
    if single:
        return images[0], faces[0]
    return torch.stack(list(images)), torch.stack(list(faces))


class Glb:
    """How meshes are written on the device (mp_mesh_glb in include/monoport_hip.h: binary glTF 2.0 under
    KHR_mesh_quantization, byte for byte this library's own definition; what the reference's ``save_obj_mesh*`` write as
    text on the host): 16-bit positions on the reconstruction box, with ``normals`` signed bytes, with ``colors`` bytes,
    16-bit indices below 65 536 vertices.  ``capacity``: bytes reserved per mesh, at least the empty file's 100; None =
    the file of a mesh of a quarter of the buffers' capacities (the 257^3 body fills about a ninth of a slot's 12 r^2
    vertices and 24 r^2 faces), never more than ``ops.glb_max_bytes``.  A file that does not fit is reported by the
    device and encoded again alone at its exact size (``encode_glb``, ``FrameSlot.glbs``): the capacity never changes
    the bytes.  ``texture``: None, or an ``Atlas``: the file then carries netC as a base colour texture instead of
    COLOR_0 (mp_mesh_glb_textured: an unindexed primitive with TEXCOORD_0 and the atlas's PNG inside the file);
    ``colors`` then defaults to False, and ``colors=True`` is refused, because glTF multiplies COLOR_0 into the texture.
    Everything is validated here; a Glb holds host values only."""

    _UNSET = object()  # ``colors`` left to its default: True without a texture, False with one

    def __init__(self, normals=True, colors=_UNSET, capacity=None, texture=None):
        who = "Glb"
        if texture is not None and not isinstance(texture, Atlas):
            raise ValueError("%s: texture must be None or a recon.Atlas, got %r" % (who, type(texture).__name__))
        if colors is Glb._UNSET:
            colors = texture is None
        for name, flag in (("normals", normals), ("colors", colors)):
            if not isinstance(flag, (bool, np.bool_)):
                raise ValueError("%s: %s must be a bool, got %r" % (who, name, flag))
        if colors and texture is not None:
            raise ValueError("%s: colors=True together with texture=: glTF multiplies COLOR_0 into the texture" % who)
        self.normals, self.colors, self.texture = bool(normals), bool(colors), texture
        if capacity is not None:
            if (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer))
                    or not ops.GLB_MIN_BYTES <= capacity <= 2 ** 31):
                raise ValueError("%s: capacity must be None or an int in %d..2^31 bytes, got %r"
                                 % (who, ops.GLB_MIN_BYTES, capacity))
            capacity = int(capacity)
        self.capacity = capacity

    def capacity_for(self, max_verts, max_faces):
        """Bytes reserved per mesh in buffers of these capacities."""
        if self.capacity is not None:
            return self.capacity
        if self.texture is not None:  # no more faces than the atlas holds, and the image at its own capacity
            t = self.texture
            return min(ops.glb_textured_bytes(min(max_faces // 4, t.faces), t.png_capacity(), self.normals),
                       ops.glb_textured_max_bytes(max_faces, t.size, self.normals))
        return min(ops.glb_bytes(max_verts // 4, max_faces // 4, self.normals, self.colors),
                   ops.glb_max_bytes(max_verts, max_faces, self.normals, self.colors))


def _encode_glb_textured(who, meshes, glb, b_min, b_max, query):
    """``encode_glb`` under ``glb.texture``: the bake (``_bake``), ONE mp_picture_png over the atlases' images, one
    mp_mesh_glb_textured per mesh.  Two device-to-host copies of sizes (the PNGs', the files'), then the used prefixes;
    an image that exceeded the atlas's PNG capacity is encoded again at the size the device reported, and so is a file."""
    atlas = glb.texture
    for k, m in enumerate(meshes):
        if m.verts.shape[0] and m.faces.shape[0] > atlas.faces:
            raise ValueError("%s: mesh %d has %d faces and Atlas(%d, %d) holds %d: simplify the mesh, or take a larger "
                             "atlas or smaller cells" % (who, k, m.faces.shape[0], atlas.size, atlas.cell, atlas.faces))
    subjects = _mesh_subjects(who, meshes)
    images, _, _ = _bake(who, subjects, atlas, query)
    images = torch.stack(list(images))
    png, png_info = _png_raw(atlas.png, images, None, capacity=atlas.png_capacity())
    sizes = png_info.cpu().numpy()
    if sizes[:, 1].any():  # the same bytes at a sufficient capacity
        png, png_info = _png_raw(atlas.png, images, None, capacity=int(sizes[:, 0].max()))
        sizes = png_info.cpu().numpy()
    shapes = [(int(m.verts.shape[0]), int(m.faces.shape[0])) for m in meshes]
    capacity = glb.capacity
    if capacity is None:
        capacity = max(ops.glb_textured_bytes(nf if nv else 0, int(size), glb.normals)
                       for (nv, nf), size in zip(shapes, sizes[:, 0]))
    out = torch.empty((len(meshes), capacity), dtype=torch.uint8, device=images.device)
    info = torch.empty((len(meshes), 2), dtype=torch.int32, device=images.device)

    def encode(i, **kw):
        return ops.mesh_glb_textured_raw(subjects.verts[i], subjects.faces[i], subjects.counts[i], atlas.size,
                                         atlas.cell, png[i:i + 1], png_info[i:i + 1],
                                         meshes[i].normals.contiguous() if glb.normals else None, None, b_min, b_max, **kw)
    for i in range(len(meshes)):
        encode(i, out=out[i:i + 1], info=info[i:i + 1])
    host = info.cpu().numpy()
    if (host[:, 1] == 2).any():
        raise RuntimeError("%s: the device refused mesh %d (info %s)" % (who, int(np.argmax(host[:, 1] == 2)), host))
    return _collect_files(who, out, host, lambda i, size: encode(i, capacity=size))


def encode_glb(meshes, glb=None, b_min=(-1, -1, -1), b_max=(1, 1, 1), netC=None, feat_tensors_C=None,
               calib_tensors=None, view=None, colors=None):
    """The binary glTF files of ``meshes`` (a ``Mesh`` on the device, or a list of them) under ``glb`` (a ``Glb``; None:
    its defaults), laid out on the device: ``bytes`` for one mesh, a list of ``bytes`` for a list.  ``b_min`` / ``b_max``:
    the box the 16-bit positions span (the reconstruction's; a vertex outside is clamped onto it).  A mesh without the
    normals or colours ``glb`` asks for is a ValueError that names it.  Without a ``glb.capacity`` every file gets its
    exact size, which the host knows from the shapes; one host-to-device copy of the counts, one device-to-host copy of
    the sizes, then one of the used prefixes; a mesh whose file exceeded ``glb.capacity`` is encoded again alone at the
    size the device reported.  Any glTF 2.0 reader that knows KHR_mesh_quantization loads the files; tests/glb_ref.py
    restates them byte for byte.  With ``glb.texture`` (an ``Atlas``) the texture is baked first, as ``bake_texture``
    does from ``netC`` / ``feat_tensors_C`` / ``calib_tensors`` / ``view`` or from ``colors`` (all refused without a
    texture), encoded as a PNG on the device and written into the file (tests/glb_texture_ref.py); a mesh with more
    faces than the atlas holds is a ValueError raised before anything is enqueued."""
    who = "encode_glb"
    glb = Glb() if glb is None else glb
    if not isinstance(glb, Glb):
        raise ValueError("%s: glb must be a recon.Glb, got %r" % (who, type(glb).__name__))
    meshes, single = _texture_meshes(who, meshes)
    for k, m in enumerate(meshes):
        for name, wanted, have in (("normals", glb.normals, m.normals), ("colors", glb.colors, m.colors)):
            if wanted and have is None:
                raise ValueError("%s: mesh %d has no %s and glb asks for them" % (who, k, name))
    if glb.texture is None:
        if any(a is not None for a in (netC, feat_tensors_C, calib_tensors, view, colors)):
            raise ValueError("%s: netC=, its maps, view= and colors= bake glb.texture, and this Glb has none" % who)
    else:
        if single and feat_tensors_C is not None and calib_tensors is not None:  # a single mesh's own
            feat_tensors_C, calib_tensors = [feat_tensors_C], [calib_tensors]
        query = _atlas_query(who, meshes, netC, feat_tensors_C, calib_tensors, view, colors)
    if not meshes:
        return []
    if glb.texture is not None:
        files = _encode_glb_textured(who, meshes, glb, b_min, b_max, query)
        return files[0] if single else files
    dev = meshes[0].verts.device
    sizes = [(int(m.verts.shape[0]), int(m.faces.shape[0])) for m in meshes]
    capacity = glb.capacity
    if capacity is None:
        capacity = max(ops.glb_bytes(nv, nf, glb.normals, glb.colors) for nv, nf in sizes)
    counts = torch.tensor(sizes, dtype=torch.int32).to(dev)
    out = torch.empty((len(meshes), capacity), dtype=torch.uint8, device=dev)
    info = torch.empty((len(meshes), 2), dtype=torch.int32, device=dev)

    def encode(i, **kw):  # the meshes differ in size: one call each, into their rows
        m = meshes[i]
        return ops.mesh_glb_raw(m.verts.contiguous(), m.faces.contiguous(), counts[i],
                                m.normals.contiguous() if glb.normals else None,
                                m.colors.contiguous() if glb.colors else None, "rows", 1.0, 0.0, b_min, b_max, **kw)
    for i in range(len(meshes)):
        encode(i, out=out[i:i + 1], info=info[i:i + 1])
    files = _collect_files(who, out, info.cpu().numpy(), lambda i, size: encode(i, capacity=size))
    return files[0] if single else files


def _scene_pictures(who, scene, cams, ras, maps=None, fronts=None, composite="depth", out=None, back=None):
    """THE scene behind a set of pictures, for the render calls, a slot and a slot's re-run alike -> (per camera set the
    raw picture (image, depth, face; each [n_views, ...]) of ``scene`` under the ``ops.Raster`` ``ras``, per camera set
    the composite (image, depth, mask) or None).  (1) ``ops.render_scene_batch``, with the scene's positions where
    there is a shadow to cast -- or ``back`` = (images, depths, faces, positions), the caller's own pictures of the
    scene, which are then only read; (2) ``maps`` (None: no light, or no caster) = the (depths, faces) of
    ``_shadow_maps``, one per camera set: ``ops.picture_shadow_batch`` with ``scene.light`` on the scene's image;
    (3) ``fronts`` (None: the scene alone): per camera set the subject's raw picture, put over the scene by
    ``ops.picture_composite_batch`` in the mode ``composite``.  ``out``: None (fresh tensors; the shadow falls on the
    scene's image in place), or a dict of the caller's buffers, each [n, ...]: ``scene_image``, ``scene_depth``,
    ``scene_face``, ``scene_uv``, with ``maps`` ``scene_pos`` and ``scene_lit`` -- a separate lit image, which the
    composite then takes while ``scene_image`` stays unshadowed --, with ``fronts`` ``pictures_image``,
    ``pictures_depth`` (they may be the fronts' own: the composite in place) and ``pictures_mask``."""
    out = out or {}
    if back is None:
        positions = None
        if maps is not None:
            positions = out.get("scene_pos")
            if positions is None:
                nv = ops._view_calibs(who, cams[0]).shape[0]
                positions = torch.empty((len(cams), nv) + ras.res + (3,), dtype=torch.float32,
                                        device=scene.verts.device).unbind(0)
        pics = (out["scene_image"], out["scene_depth"], out["scene_face"]) if "scene_image" in out else None
        backs = ops.render_scene_batch(who, scene, cams, ras, out=pics, uv=out.get("scene_uv"), positions=positions)
        lit = out.get("scene_lit", [b[0] for b in backs])
    else:
        backs, positions, lit = list(zip(*back[:3])), back[3], None
    if maps is not None:
        light = scene.light
        lit = ops.picture_shadow_batch([b[0] for b in backs], list(positions), [b[2] for b in backs], maps[0], maps[1],
                                       light.calib, light.projection, light.nearest, light.bias, light.radius,
                                       light.strength, out=None if lit is None else (list(lit), None), who=who)
        backs = [(shadowed[0], b[1], b[2]) for shadowed, b in zip(lit, backs)]
    if fronts is None:
        return backs, None
    pics = (out["pictures_image"], out["pictures_depth"], out["pictures_mask"]) if "pictures_mask" in out else None
    return backs, ops.picture_composite_batch(fronts, backs, composite, ras.nearest, ras.background, out=pics, who=who)


@torch.no_grad()
def render_scene(scene, calibs, res=257, projection="orthogonal", nearest="max", near=None, perspective_correct=False,
                 background=1.0, samples=1, casters=None):
    """The textured picture of a ``Scene`` under ``calibs`` ([4,4] / [3,4], or [n_views, ...]): the rasteriser writes a
    UV picture (``near`` / ``perspective_correct`` as in ``render_mesh``), ``ops.picture_texture_batch`` looks the
    texture up per pixel at the nearest mip level, bilinearly.  Returns a ``MeshRender``; pixels the scene does not
    cover hold ``background``.  No host sync.  The scene goes through the rasteriser as any mesh does: a clipped face
    that still projects beyond its 2^22 snap guard is dropped whole (``near`` far below 0.05 with a 3 m floor at
    1024^2); the side planes are not clipped.  ``casters``: None, or the ``Mesh`` whose shadow falls on the scene under
    ``scene.light`` (ignored without a light): the picture is then the shadowed one.  ``samples``: as in
    ``render_mesh`` -- 1 changes nothing; 2..4 run the UV pass, the texture lookup (whose mip level then follows the
    finer uv steps) and the shadow at ``samples`` times ``res`` and return the ``ResolvedPicture`` (mask None; coverage =
    the scene's own)."""
    who = "render_scene"
    _check_scene(who, scene)
    ras = ops.raster(who, res, projection, nearest, background, near, perspective_correct, samples)
    maps = None
    if scene.light is not None and casters is not None:
        maps = tuple(zip(*shadow_map([casters], scene.light, device=scene.verts.device)))
    _, backs, resolved = _resolved_pictures(who, None, [calibs], ras, None, scene=scene, maps=maps)
    if resolved is not None:
        return ResolvedPicture(*_squeezed(resolved[0], calibs))
    return MeshRender(*_squeezed(backs[0], calibs))


@torch.no_grad()
def composite(front, back, mode="depth", nearest="max", background=1.0):
    """``front`` over ``back`` (``MeshRender``s of one size, each with an image): ``mode="over"`` is the reference's
    mask composite -- the front wherever it is covered --, ``mode="depth"`` also lets the back hide the front where the
    back is strictly nearer under ``nearest`` ("max" / "min", as both were rendered).  Returns a ``ScenePicture`` of
    fresh tensors.  Defined bit for bit in include/monoport_hip.h (mp_picture_composite).  No host sync."""
    image, depth, mask = ops.picture_composite_batch([tuple(front)[:3]], [tuple(back)[:3]], mode, nearest, background,
                                                     who="composite")[0]
    return ScenePicture(image, depth, front[2], mask)


@torch.no_grad()
def resolve_picture(picture, samples, nearest="max"):
    """The final picture of ``picture`` -- a ``MeshRender`` or a ``ScenePicture`` (or such a tuple) rendered at
    ``samples`` (2..4) times the final size, [s H,s W,...] or [n_views,s H,s W,...] -- as a ``ResolvedPicture`` of fresh
    tensors: the generic call of the render calls' ``samples=``, which give the same bits.  Per pixel over its s x s
    samples: the mean of the image (None stays None), the depth and face of the nearest sample that shows under
    ``nearest`` ("max" / "min", as the picture was rendered), the largest mask, and ``coverage`` = the fraction of
    samples that is the subject's (mask == 2; without a mask face >= 0).  Defined bit for bit in include/monoport_hip.h
    (mp_picture_resolve).  No host sync."""
    who = "resolve_picture"
    picture = tuple(picture)
    if len(picture) not in (3, 4) or picture[1] is None or picture[2] is None:
        raise ValueError("%s: picture must be a MeshRender (image, depth, face) or a ScenePicture (image, depth, face, "
                         "mask)" % who)
    image, depth, face = picture[:3]
    mask = picture[3] if len(picture) == 4 else None
    return ResolvedPicture(*ops.picture_resolve_batch(
        None if image is None else [image.contiguous()], [depth.contiguous()], [face.contiguous()],
        None if mask is None else [mask.contiguous()], samples, nearest, who=who)[0])


@torch.no_grad()
def render_mesh_many_in_scene(meshes, scene, calibs, res=257, shade="colors", projection="orthogonal", nearest="max",
                              background=1.0, near=None, perspective_correct=False, composite="depth", netC=None,
                              feat_tensors_C=None, calib_tensors=None, view=None, samples=1, lighting=None):
    """``render_mesh_many`` of ``meshes`` composited over ``render_scene`` of ``scene`` under the same cameras
    (``calibs``: one camera set for all, or a list with one per mesh), ``composite``: "depth" or "over".  Returns a
    list of ``ScenePicture``s; a ``None`` mesh gives the bare scene (mask in {0, 1}, face -1).  ``shade`` may not be
    None: the composite is of images.  Two more launches per ops.MAX_FRAMES pictures than the two renders; no host
    sync.  With ``scene.light`` every mesh also casts its shadow on its own picture of the scene before the composite;
    without a light nothing more is enqueued than before.  ``lighting`` (a ``Lighting``; None: nothing more is
    enqueued) lights the subject's image as in ``render_mesh``, before the composite; the scene keeps its texture and
    its shadow.  With ``lighting.self_shadow`` (it needs ``scene.light``) the subject is also looked up in its own
    shadow map, with that bias, which takes the direct term away where the shade is 1.  What is enqueued, and in which
    order: ``_shadow_maps``, ``_subject_pictures``, ``_scene_pictures`` -- all through ``_resolved_pictures``.
    ``samples``: as in ``render_mesh`` -- 1 changes nothing; with 2..4 the subject's passes, the scene's and the
    composite run at ``samples`` times ``res`` (the shadow map keeps the light's own size), so that the edges between
    subject and scene are blended from composited samples, and one resolve at the end gives ``ResolvedPicture``s:
    ``mask`` the largest of the composite's masks, ``coverage`` the fraction of samples where the subject shows."""
    who = "render_mesh_many_in_scene"
    _check_scene(who, scene)
    if shade is None:
        raise ValueError("%s: the composite is of images; shade=None renders none" % who)
    ops._named_mode(who, "composite", ops.COMPOSITE_MODES, composite)
    meshes = list(meshes)
    if lighting is not None:
        _check_lighting(who, lighting, shade, meshes, scene.light)
    if not meshes:
        return []
    cams = _camera_sets(who, calibs, len(meshes))
    ras = ops.raster("render_mesh_many", res, projection, nearest, background, near, perspective_correct, samples)
    fronts, _, done, resolved = _render_mesh_many("render_mesh_many", meshes, calibs, ras, shade, netC, feat_tensors_C,
                                                  calib_tensors, view, lighting, scene, composite, who)
    if resolved is not None:
        return [ResolvedPicture(*_squeezed(pic, cam)) for pic, cam in zip(resolved, cams)]
    return [ScenePicture(*_squeezed((image, depth, front[2], mask), cam))
            for (image, depth, mask), front, cam in zip(done, fronts, cams)]


@torch.no_grad()
def prepare_inputs(segm, mean, std, with_color=True):
    """The two "update input by removing bg" processors of RTL/main.py:352-364 as one HIP kernel:
    returns (input_netG, input_netC)."""
    return ops.prepare_inputs(segm, mean, std, with_color)


@torch.no_grad()
def visulization(render_norm, render_tex=None, render_size=256):
    """(sic) RTL/main.py:252-281: both renders scaled to 0..255, rotated by 90 degrees,
    nearest-resized to 256x256 and moved to the host as [256,256,3] numpy arrays, plus the
    foreground mask (pixels that are not pure white) of the last render present."""
    if render_norm is None and render_tex is None:
        return None, None, None
    outs, mask = [], None
    for img in (render_norm, render_tex):
        if img is None:
            outs.append(None)
            continue
        out, m = ops.visualize(img.detach(), render_size)
        outs.append(out.cpu().numpy())
        mask = m
    return outs[0], outs[1], mask.cpu().numpy().astype(bool).reshape(render_size, render_size, 1)
