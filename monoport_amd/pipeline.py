"""Per-frame reconstruction pipeline with several frames in flight on one GPU.

The reference overlaps frames with one Python thread per stage (RTL/dataloader.py:734-751,
:1026-1053).  On an MI355X the stages are so short (tens of microseconds to a few milliseconds)
that host-side launch latency and GPU fill, not thread parallelism, are what matter:

* a ``FrameSlot`` owns a HIP stream and the static buffers of ``batch`` frames.  The image
  encoder -- 137 launches of the hand-written kernels of csrc/conv3x3.hip, convim2col.hip and
  encoder_ops.hip, no MIOpen / torch op -- runs ONCE per slot on the whole batch (a batch-1
  convolution on a 32^2 / 64^2 map under-fills 256 CUs: 3.8 ms/frame at batch 1, 2.1 ms/frame at
  batch 16) and is replayed as a hipGraph; the slot's skip tables (csrc/query_table.hip) are made
  in one launch behind it; then each frame goes through

      channels-last pack -> octree (5 levels, fused query) -> forward_vertices -> render

  as asynchronous C-ABI calls on the slot's stream, the octree level by level for the whole
  batch (``mp_recon_batch``: one fused-query launch per level covers all frames of the slot --
  a single frame's coarse levels, 5-25 k points, leave most of the 256 CUs idle);
* a ``FramePipeline`` round-robins over ``depth`` slots, so independent frames on different
  streams fill the CUs that the coarse octree levels and the small encoder kernels leave idle
  (``depth`` x ``batch`` frames in flight; BASELINE configs[3] asks for 8);
* a ``ViewsSlot`` is the FrameSlot of a multi-view netG (a capture rig: ``batch`` frames of V views each): one
  encoder pass over batch x V images, the octree of all frames through ``mp_recon_views_batch``, then the same
  per-volume stages (``FramePipeline(..., slot_class=ViewsSlot)``); a ``ColorViewsSlot`` adds a multi-view netC: one
  more encoder pass and the colours of all frames through ``mp_query_views_counted_batch``.
"""
import collections

import numpy as np
import torch

from . import ops
from .synthetic import Z_SCALE

import os

RESOLUTIONS = (17, 33, 65, 129, 257)  # RTL/main.py:187
# frames per forward_vertices / paint launch set (results are identical): "on" = all frames of the slot, "off" = one,
# or a number.  4: measured on 20-frame single submissions 185.8 (1) / 189.2 (4) / 189.8 (all) recon/s -- and with three
# slots overlapping, launches over all 16 frames of a slot (first_hit: 37 k workgroups) hold up the other slots'
# chains of small dependent kernels: passes of 5.4-5.6 ms per frame against 5.2-5.4 with 1 or 4 frames per launch
_vb = os.environ.get("MONOPORT_VERTEX_BATCH", "4")
VERTEX_BATCH = 0 if _vb == "off" else (int(_vb) if _vb.isdigit() else 10 ** 6)
MAX_RECON_BATCH = ops.MAX_FRAMES  # kMaxFrames of the C-ABI (include/monoport_hip.h, mp_recon_batch): 32
# frames per launch set of the mesh chain of a slot (FrameSlot(mesh=...); results are identical): "on" = all frames of
# the slot (at most MAX_RECON_BATCH), "off" = one, or a number.  The chunk trades launches against the stream's scratch
# arena (68 MB of marching-cubes vbase + 48 MB of normals scratch per frame at 257^3: 2.3 GB for 20 frames) and against
# holding up the other slots' chains.  on: measured on 20-frame slots with netC colours and accumulate normals
# (tools/mesh_timing.py --batched --passes 9, median ms per frame, meshes() included) 9.09 (1) / 8.87 (4) / 8.80 (all)
# on single submissions, min-max spreads <= 0.06; with three slots submitted back to back 8.94 / 8.78 / 8.76, where
# 4 and all lie inside each other's spread (0.16-0.19).  The same slots without mesh output: 6.34 / 6.31
_mb = os.environ.get("MONOPORT_MESH_BATCH", "on")
MESH_BATCH = 1 if _mb == "off" else min(int(_mb) if _mb.isdigit() and int(_mb) > 0 else MAX_RECON_BATCH, MAX_RECON_BATCH)
MESH_KEYS = ("normals", "level", "colors", "clean", "simplify", "smooth")
PICTURE_KEYS = ("views", "res", "shade", "projection", "nearest", "near", "perspective_correct", "background", "scene",
                "composite")
PICTURE_OPTION_KEYS = PICTURE_KEYS + ("samples",)  # what a ``pictures`` dict may hold


class PictureOptions(collections.namedtuple("PictureOptions", PICTURE_KEYS, defaults=(None, "depth"))):
    """What a slot's free-viewpoint pictures are asked for, validated by ``_picture_options``: the cameras per frame,
    the size (H, W), the arguments of ``recon.render_mesh``, and the ``recon.Scene`` behind the subject (None: none)
    with the ``composite`` mode ("depth" or "over") that puts the subject's picture over it.  ``samples`` (1: none), the
    anti-aliasing of the final pictures, is the record's last option but rides beside the tuple's fields, as in
    ``ops.Raster``: the tuple stays what one pass at ``res`` is asked for."""

    def __new__(cls, *args, samples=1, **kwargs):
        self = super().__new__(cls, *args, **kwargs)
        self.samples = samples
        return self

    @property
    def raster(self):
        """The fields every pass of the rasteriser takes and ``samples``, as the ``ops.Raster`` of the ``recon``
        bodies."""
        return ops.Raster(self.res, self.projection, self.nearest, self.background, self.near, self.perspective_correct,
                          self.samples)


def _mesh_options(mesh, balance, has_netc):
    """FrameSlot's ``mesh`` argument (a dict or an object with these attributes) -> recon.MeshOptions."""
    from .recon import mesh_options
    if isinstance(mesh, dict):
        unknown = sorted(set(mesh) - set(MESH_KEYS))
        if unknown:
            raise ValueError("FrameSlot(mesh=...): unknown keys %s (known: %s)" % (unknown, list(MESH_KEYS)))
        get = mesh.get
    else:
        def get(key, default=None):
            return getattr(mesh, key, default)
    level, colors = get("level"), get("colors")
    opts = mesh_options(get("normals", "accumulate"), float(balance if level is None else level),
                        has_netc if colors is None else colors, get("clean"), get("simplify"), get("smooth"))
    if opts.colors and not has_netc:
        raise ValueError("FrameSlot(mesh=...): colors need netC")
    return opts


def _picture_options(pictures, mesh, has_netc=False):
    """FrameSlot's ``pictures`` argument (a dict) -> PictureOptions; ``mesh``: the slot's validated MeshOptions or None;
    ``has_netc``: whether the slot runs a netC (``shade="netC"`` queries it per pixel).  Nothing is allocated here."""
    who = "FrameSlot(pictures=...)"
    if not isinstance(pictures, dict):
        raise ValueError("%s: a dict with any of %s, got %r" % (who, list(PICTURE_OPTION_KEYS), pictures))
    unknown = sorted(set(pictures) - set(PICTURE_OPTION_KEYS))
    if unknown:
        raise ValueError("%s: unknown keys %s (known: %s)" % (who, unknown, list(PICTURE_OPTION_KEYS)))
    if mesh is None:
        raise ValueError("%s: the pictures are of the slot's meshes; it needs mesh=..." % who)
    from .recon import SHADES
    views = pictures.get("views", 1)
    if isinstance(views, bool) or not isinstance(views, (int, np.integer)) or views < 1:
        raise ValueError("%s: views must be an int >= 1, got %r" % (who, views))
    ras = ops.raster(who, pictures.get("res", 257), pictures.get("projection", "orthogonal"),
                     pictures.get("nearest", "max"), pictures.get("background", 1.0), pictures.get("near"),
                     pictures.get("perspective_correct", False), pictures.get("samples", 1))
    default = "colors" if mesh.colors else ("normals" if mesh.normals is not None else None)
    shade = pictures.get("shade", default)
    if shade not in SHADES:
        raise ValueError("%s: shade must be one of %s, got %r" % (who, list(SHADES), shade))
    if shade == "normals" and mesh.normals is None:
        raise ValueError("%s: shade='normals', but the mesh options have normals=None" % who)
    if shade == "colors" and not mesh.colors:
        raise ValueError("%s: shade='colors' needs the mesh's colours (mesh colors, hence netC)" % who)
    if shade == "netC" and not has_netc:
        raise ValueError("%s: shade='netC' queries the slot's netC per pixel, and the slot has none" % who)
    scene, composite = pictures.get("scene"), pictures.get("composite", "depth")
    if scene is not None:
        from .recon import Scene
        if not isinstance(scene, Scene):
            raise ValueError("%s: scene must be a recon.Scene, got %r" % (who, type(scene).__name__))
        if shade is None:
            raise ValueError("%s: a scene is composited with the subject's image; shade=None renders none" % who)
    if not isinstance(composite, str) or composite not in ops.COMPOSITE_MODES:
        raise ValueError("%s: composite must be one of %s, got %r" % (who, sorted(ops.COMPOSITE_MODES), composite))
    return PictureOptions(int(views), ras.res, shade, ras.projection, ras.nearest, ras.near, ras.perspective_correct,
                          ras.background, scene, composite, samples=ras.samples)


class FrameSlot:
    """Static buffers for ``batch`` in-flight frames (geometry chain of RTL/main.py:366-428, plus
    the netC texture stages :373-441 when ``netC`` is given)."""

    view = 0  # the row of a multi-view head's result (ViewsSlot); a single-view head has the one
    jpeg = None  # the ``recon.Jpeg`` of ``encode_pictures``; None: nothing is allocated or enqueued for it
    png = None   # the ``recon.Png`` of ``encode_pictures``; None likewise
    glb = None   # the ``recon.Glb`` of ``encode_meshes``; None likewise
    _chained = False  # the chain has been enqueued at least once (``prepare`` / ``submit``)

    def __init__(self, netG, device, resolutions=RESOLUTIONS, b_min=(-1, -1, -1), b_max=(1, 1, 1),
                 balance=0.5, feature_hook=None, use_graph=False, netC=None, batch=1, skip_table=None,
                 final_level="dilate3", mesh=None, pictures=None, lighting=None):
        """``mesh``: None (no mesh output; nothing is allocated or enqueued for it), or a dict / options object with
        ``normals`` ("accumulate" -- the default --, "reference" or None), ``level`` (the iso-level; default: the
        slot's ``balance``) and ``colors`` (per-vertex netC colours; default: ``netC is not None``) and ``clean`` (None
        -- the default: nothing is allocated or enqueued for it --, or 6 / 26: marching cubes sees only the largest connected body of each
        volume, ``recon.keep_largest`` into copies that live in mesh buffers of one mesh chunk of frames;
        ``volumes``, the renders and every other consumer see the unchanged volume) and ``simplify`` (None -- the
        default: nothing is allocated or enqueued for it --, or the cells per axis, 1..512, of ``recon.simplify_mesh``
        over the slot's box: the vertex clustering runs between marching cubes and the normals / colours, into a second
        set of vertex / face / count buffers plus the vertex map, 40 bytes per vertex of capacity; normals and colours
        are those of the simplified mesh and the colour query shrinks with it) and ``smooth`` (None -- the default:
        nothing is allocated or enqueued for it --, the iterations, or the dict of ``recon.reconstruct_mesh``'s
        ``smooth``: Taubin passes behind marching cubes / the clustering, into one more vertex buffer, 12 bytes per vertex
        of capacity; vertices and normals are the smoothed mesh's, the colours are queried before smoothing).  ``self.mesh``
        is the validated ``recon.MeshOptions`` of all six (None without mesh output).  The slot then
        owns static per-frame mesh buffers at the capacities of ``ops.marching_cubes_raw`` (12 r^2 vertices and
        24 r^2 faces: vertices, faces, normals, query points and predictions are about 57 MB per frame at 257^3), the
        batched mesh chain runs behind the octree on the slot's stream, and ``meshes()`` hands the results out.

        ``pictures``: None (no free-viewpoint pictures; nothing is allocated or enqueued for them), or a dict with any
        of ``views`` (cameras per frame, default 1), ``res`` (int or (H, W), default 257), ``shade`` ("normals",
        "colors" or None; default: what the mesh options provide, colours first) and ``projection``, ``nearest``,
        ``near``, ``perspective_correct``, ``background`` as ``recon.render_mesh`` takes them.  It needs ``mesh``.
        ``self.picture_options`` is the validated ``PictureOptions`` (None without pictures).  ``submit`` then takes
        ``cameras``, the pictures are rendered behind the mesh chain on the slot's stream, with no host value in
        between (``_render_pictures``: what is enqueued is written once, in ``recon._resolved_pictures`` and the two
        bodies it runs, ``recon._subject_pictures`` and ``recon._scene_pictures``, and this docstring only names the
        buffers), and ``pictures()`` hands the results out:
        the static ``pictures_image`` [batch,views,H,W,3] (None with ``shade=None``), ``pictures_depth`` and
        ``pictures_face`` [batch,views,H,W].  ``shade="netC"`` colours the
        pictures per pixel (``recon.render_mesh(shade="netC")``): it needs the slot's ``netC`` but NOT the mesh's
        colours -- with ``mesh={"colors": False}`` the per-vertex colour query is never enqueued, which is the saving --
        and the slot then also owns, per frame of L = views * H * W pixels, the static lists of the covered pixels
        (points [3,L], pixels [L], predictions [3,L], count [2]: 28 bytes per pixel); ``pictures_image`` holds the
        surface positions first and the colours in the end.  ``scene`` (a ``recon.Scene``; default None: nothing is
        allocated or enqueued for it) puts a textured scene behind the subject (``composite``: "depth", the default,
        or "over"): static ``scene_uv`` / ``scene_image`` / ``scene_depth`` / ``scene_face`` buffers, the composite in
        place in ``pictures_image`` / ``pictures_depth``, and ``pictures_mask`` [batch,views,H,W] uint8 (0 neither, 1
        scene, 2 subject); ``pictures()`` then returns ``recon.ScenePicture``s, the bare scene for an empty frame.  It
        needs a ``shade``.  A scene with a ``light`` (``recon.Scene(light=recon.Light(...))``; the light belongs to the
        scene, the option keys do not change) also shows each frame's shadow on it: the slot then owns
        ``shadow_depth`` / ``shadow_face`` [batch,Hs,Ws] (the frames' shadow maps), ``scene_pos`` (the scene's
        world-space positions) and ``scene_lit`` (the shadowed scene, which the composite takes; ``scene_image`` stays
        unshadowed).  Without a light none of them exists and nothing more is enqueued.  ``samples`` (1, the default:
        nothing is allocated or enqueued for it, and ``pictures_coverage`` is None) anti-aliases the pictures as
        ``recon.render_mesh(samples=)`` does: with s in 2..4 every pass and the composite run at s times ``res`` (s * res
        may not exceed 4096) in working buffers of that size -- ``fine_image`` / ``fine_depth`` / ``fine_face`` /
        ``fine_mask`` for the subject and the composite, and the ``scene_*``, ``light_*`` buffers and the ``shade="netC"``
        lists above, all s * s times their size --, and ONE resolve, enqueued behind the composite (behind the lighting
        without a scene) on the slot's stream, fills ``pictures_image`` / ``pictures_depth`` / ``pictures_face`` /
        ``pictures_mask``, which stay [batch,views,H,W,...], and ``pictures_coverage`` [batch,views,H,W] f32, the
        subject's alpha; ``pictures()`` then returns ``recon.ResolvedPicture``s and ``jpegs()`` encodes the resolved
        image.  Memory: the per-pixel bytes above times s * s (20 bytes per pixel of subject and composite, 44 of the
        scene, 28 of the netC lists, ...: at 1024^2, one view and s = 2 the subject and scene alone grow from 64 to
        256 MB per frame) plus 25 bytes per final pixel; ``shade="netC"`` queries s * s times the points.

        ``lighting`` (a ``recon.Lighting``; None, the default: nothing is allocated or enqueued for it, and it is not a
        ``pictures`` key) lights the subject's picture per pixel before the composite, as ``recon.render_mesh(lighting=)``
        does: the slot then owns ``light_normal`` [batch,views,H,W,3] and ``light_face`` [batch,views,H,W] and, with
        ``lighting.self_shadow`` (it needs the scene's light), ``light_shade`` [batch,views,H,W] and ``light_pos``
        [batch,views,H,W,3] (not with ``shade="netC"``, whose position picture is read before it is painted over).  It
        needs pictures with a ``shade``, the mesh's normals, and for ``shade="normals"`` a constant
        ``lighting.albedo``.  With ``lighting.transfer`` (a ``recon.Transfer``; without it none of this exists) the SH
        term is self-occluded: the slot also owns ``transfer_bits`` [batch, ops.volume_bits_words(R)] int32 (packed
        inside the mesh chunk loop from the volume marching cubes reads -- with ``clean`` the cleaned one --, under the
        frames' gates), ``transfer_prt`` [batch,cap_v,9], ``transfer_shade`` [batch,cap_v,3] and ``light_ambient``
        [batch,views,H,W,3]; a frame whose mesh ``meshes()`` made again is traced again through its bits."""
        self.views = self._head_views(netG, netC, mesh)  # images per frame; refuses what the slot class does not run
        # the option records are validated before anything is allocated
        self.mesh = None if mesh is None else _mesh_options(mesh, float(balance), netC is not None)
        self.picture_options = None if pictures is None else _picture_options(pictures, self.mesh, netC is not None)
        self.lighting = lighting
        self._traces = getattr(lighting, "transfer", None) is not None  # the SH term is self-occluded
        self._reran_transfer = {}  # frame -> the transfer ``meshes()`` traced for its re-run mesh
        if lighting is not None:
            from .recon import _check_lighting_options
            po = self.picture_options
            if po is None:
                raise ValueError("FrameSlot(lighting=...): lighting shades the slot's pictures; it needs pictures=...")
            _check_lighting_options("FrameSlot(lighting=...)", lighting, po.shade, self.mesh.normals is not None,
                                    None if po.scene is None else po.scene.light)
        self.net = netG
        self.netC = netC
        self.device = torch.device(device)
        self.res = [int(r) for r in resolutions]
        self.b_min, self.b_max, self.balance = b_min, b_max, float(balance)
        self.final_level = final_level  # the last octree level's selection rule (Seg3dLossless docstring)
        self.feature_hook = feature_hook  # optional in-place edit of the [B,C,H,W] feature map
        self.batch = int(batch)
        r = self.res[-1]
        dev = self.device
        b = self.batch
        bv = b * self.views  # images of the slot: the encoder's batch
        self.stream = torch.cuda.Stream(device=dev)
        self.image = torch.zeros((bv, 3, 512, 512), dtype=torch.float32, device=dev)
        self.calib = torch.eye(4, dtype=torch.float32, device=dev)[None].repeat(bv, 1, 1).contiguous()
        # what ``submit`` fills, one row per frame: the buffers themselves, or (ViewsSlot) their [B,V,...] form
        self.image_in, self.calib_in = self._per_frame(self.image), self._per_frame(self.calib)
        # one [B,128,128,256] channels-last map; feats_hwc[b] are its per-image views
        self.feat_hwc_all = torch.empty((bv, 128, 128, 256), dtype=torch.float32, device=dev)
        self.feats_hwc = [self.feat_hwc_all[i] for i in range(bv)]
        # skip tables of the slot's maps (ops.SKIP_TABLE unless the caller says otherwise) -- only for the MLP
        # precisions whose query kernel reads them (f32, f16x3): a table nobody reads is 16 GFLOP + 128 MB a frame
        self.skip_table = ((ops.SKIP_TABLE if skip_table is None else bool(skip_table)) and self.views == 1
                           and ops.table_precision(netG.surface_classifier.precision))
        self.tables = (torch.empty((b, 128, 128, ops.SKIP_TABLE_ROWS), dtype=torch.float32, device=dev)
                       if self.skip_table else None)
        self._table_handle = None  # registration of the tables of the last encoder pass
        # the hourglass encoder can write its last stack's features straight into that map
        # (HGFilter.forward(hwc_out=...), csrc/conv3x3.hip: conv1x1_kernel); a feature_hook must
        # then come with a channels-last twin, ``feature_hook.hwc(feat_hwc_all)``
        from .modeling import backbones
        self.hwc_direct = (isinstance(netG.image_filter, backbones.HGFilter)
                           and backbones.ENCODER_CONV == "hip"
                           and (feature_hook is None or hasattr(feature_hook, "hwc")))
        # one volume per frame of the batch: results stay readable until the next submit
        self.volumes = [torch.empty((r, r, r), dtype=torch.float32, device=dev) for _ in range(b)]
        self.status = torch.zeros((b, 1 + len(self.res)), dtype=torch.int32, device=dev)
        self.renders = [None] * b
        self.renders_tex = [None] * b
        self.vertices = [None] * b
        self.graph = None
        self._graph_feat = None
        self.use_graph = use_graph
        self._busy = False
        self.n_active = b  # frames of the current submission (a stream's last batch may be short)
        if netC is not None:
            from .recon import color_matrix
            # one channels-last netC map per image: the colour queries of the whole slot are one launch
            self.feats_hwc_c = [torch.empty((128, 128, 512), dtype=torch.float32, device=dev)
                                for _ in range(bv)]
            self.mat_color = color_matrix(b_min, b_max, r)
            self.image_c = torch.zeros((bv, 3, 512, 512), dtype=torch.float32, device=dev)
            self.image_c_in = self._per_frame(self.image_c)
        if self.mesh is not None:
            opts = self.mesh
            cap_v = 12 * r * r  # ops.marching_cubes_raw's capacities
            cap_f = 2 * cap_v
            self.mesh_buffers = {"verts": torch.empty((b, cap_v, 3), dtype=torch.float32, device=dev),
                                 "faces": torch.empty((b, cap_f, 3), dtype=torch.int32, device=dev),
                                 "counts": torch.zeros((b, 2), dtype=torch.int32, device=dev)}
            if opts.normals is not None:
                self.mesh_buffers["normals"] = torch.empty((b, cap_v, 3), dtype=torch.float32, device=dev)
            if opts.colors:
                self.mesh_buffers["points"] = torch.zeros((b, 3, cap_v), dtype=torch.float32, device=dev)
                self.mesh_buffers["point_counts"] = torch.zeros((b, 1), dtype=torch.int32, device=dev)
                self.mesh_buffers["preds"] = torch.zeros((b, 3, cap_v), dtype=torch.float32, device=dev)
            if opts.clean is not None:
                chunk = min(MESH_BATCH, b)  # the cleaned copies are consumed chunk by chunk (68 MB per frame at 257^3)
                self.mesh_buffers["cleaned"] = torch.empty((chunk, r, r, r), dtype=torch.float32, device=dev)
                self.mesh_buffers["clean_stats"] = torch.zeros((b, 4), dtype=torch.int32, device=dev)
            if opts.simplify is not None:  # buffers of its own: marching cubes' stay its input
                self.mesh_buffers["simple_verts"] = torch.empty((b, cap_v, 3), dtype=torch.float32, device=dev)
                self.mesh_buffers["simple_faces"] = torch.empty((b, cap_f, 3), dtype=torch.int32, device=dev)
                self.mesh_buffers["simple_counts"] = torch.zeros((b, 2), dtype=torch.int32, device=dev)
                self.mesh_buffers["simple_vmap"] = torch.empty((b, cap_v), dtype=torch.int32, device=dev)
            if opts.smooth is not None:  # the vertices before smoothing stay: the colour query reads them
                self.mesh_buffers["smooth_verts"] = torch.empty((b, cap_v, 3), dtype=torch.float32, device=dev)
            self._mesh_chains = [None] * b
            self._reran = []  # frames whose chain ``meshes()`` made again with exact capacities
        self.pictures_image = self.pictures_depth = self.pictures_face = self.pictures_mask = None
        self.pictures_coverage = None
        if self.picture_options is not None:
            po = self.picture_options
            fres = ops.fine_raster(po.raster).res  # the size every pass runs at: ``samples`` times ``res``

            def pictures(res, mask):
                shape = (b, po.views) + res
                return (None if po.shade is None else torch.empty(shape + (3,), dtype=torch.float32, device=dev),
                        torch.empty(shape, dtype=torch.float32, device=dev),
                        torch.empty(shape, dtype=torch.int32, device=dev),
                        torch.empty(shape, dtype=torch.uint8, device=dev) if mask else None)
            if po.samples > 1:  # the passes work in fine_*; the resolve fills pictures_*
                self.fine_image, self.fine_depth, self.fine_face, self.fine_mask = pictures(fres, po.scene is not None)
                self.pictures_coverage = torch.empty((b, po.views) + po.res, dtype=torch.float32, device=dev)
            (self.pictures_image, self.pictures_depth, self.pictures_face,
             self.pictures_mask) = pictures(po.res, po.scene is not None)
            if po.shade == "netC":  # the covered pixels of a frame's views as one counted list
                n_pix = po.views * fres[0] * fres[1]
                self.picture_lists = {"points": torch.zeros((b, 3, n_pix), dtype=torch.float32, device=dev),
                                      "pixels": torch.zeros((b, n_pix), dtype=torch.int32, device=dev),
                                      "preds": torch.zeros((b, 3, n_pix), dtype=torch.float32, device=dev),
                                      "count": torch.zeros((b, 2), dtype=torch.int32, device=dev)}
            if po.scene is not None:  # the scene's own pictures (44 bytes per pixel); the composite's mask is above
                shape = (b, po.views) + fres
                self.scene_uv = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
                self.scene_image = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
                self.scene_depth = torch.empty(shape, dtype=torch.float32, device=dev)
                self.scene_face = torch.empty(shape, dtype=torch.int32, device=dev)
                if po.scene.light is not None:  # the subjects' shadow maps, the scene's positions and its lit image
                    hs, ws = po.scene.light.res
                    self.shadow_depth = torch.empty((b, hs, ws), dtype=torch.float32, device=dev)
                    self.shadow_face = torch.empty((b, hs, ws), dtype=torch.int32, device=dev)
                    self.scene_pos = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
                    self.scene_lit = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
            if self.lighting is not None:  # the normal pass and, for the self-shadow, the subject's positions and shade
                shape = (b, po.views) + fres
                self.light_normal = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
                self.light_face = torch.empty(shape, dtype=torch.int32, device=dev)
                if self.lighting.self_shadow is not None:
                    if po.shade != "netC":
                        self.light_pos = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
                    self.light_shade = torch.empty(shape, dtype=torch.float32, device=dev)
                if self._traces:  # the volumes' bits, the vertices' transfer and its picture
                    cap_v = self.mesh_buffers["verts"].shape[1]
                    self.transfer_bits = torch.empty((b, ops.volume_bits_words(r)), dtype=torch.int32, device=dev)
                    self.transfer_prt = torch.empty((b, cap_v, 9), dtype=torch.float32, device=dev)
                    self.transfer_shade = torch.empty((b, cap_v, 3), dtype=torch.float32, device=dev)
                    self.light_ambient = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
            # the cameras of the current submission, on the host [batch,views,3,4]; the identity until the first one
            self._cameras = np.tile(np.eye(4, dtype=np.float32)[:3], (b, po.views, 1, 1))

    def _head_views(self, netG, netC, mesh):
        for name, net in (("netG", netG), ("netC", netC)):
            if net is not None and net.surface_classifier.num_views > 1:
                raise NotImplementedError("FrameSlot: %s has a multi-view head (num_views = %d); the slot runs the "
                                          "single-view octree / colour engines (pipeline.ViewsSlot runs a multi-view "
                                          "netG)" % (name, net.surface_classifier.num_views))
        return 1

    def _per_frame(self, buf):
        return buf

    def _octree(self, mlp, n):
        """The octree of all frames of the slot level by level: one fused-query launch per level covers every frame
        (mp_recon_batch takes up to MAX_RECON_BATCH frames per call)."""
        for b0 in range(0, n, MAX_RECON_BATCH):
            b1 = min(b0 + MAX_RECON_BATCH, n)
            ops.recon_batch(mlp, self.feats_hwc[b0:b1], self.calib[b0:b1], Z_SCALE, self.b_min,
                            self.b_max, self.res, self.balance, volumes=self.volumes[b0:b1],
                            status=self.status[b0:b1], final_level=self.final_level)

    # convenience views for batch == 1 callers
    @property
    def volume(self):
        return self.volumes[0]

    @property
    def render(self):
        return self.renders[0]

    @property
    def render_tex(self):
        return self.renders_tex[0]

    @torch.no_grad()
    def _encode(self):
        """Both encoders on the slot's image buffers: (featG [B,256,128,128], featC or None)."""
        if self.hwc_direct:
            feat = self.net.image_filter(self.image, last_only=True, hwc_out=self.feat_hwc_all,
                                         keep_nchw=self.netC is not None, graphed=False)[-1][0]
            if self.feature_hook is not None:
                self.feature_hook.hwc(self.feat_hwc_all)
                if feat is not None:
                    self.feature_hook(feat)
        else:
            feat = self.net.image_filter(self.image, last_only=True)[-1][0]
            if self.feature_hook is not None:
                self.feature_hook(feat)
        feat_c = None
        if self.netC is not None:
            feat_c = self.netC.image_filter(self.image_c)[-1][0]  # [B,256,128,128]
        return feat, feat_c

    @torch.no_grad()
    def _chain(self):
        self._chained = True
        mlp = self.net.surface_classifier.packed()
        if self.graph is not None:
            self.graph.replay()  # the batched encoder(s) as one hipGraph launch
            feat, feat_c = self._graph_feat
        else:
            feat, feat_c = self._encode()
        if self.netC is not None:
            mlp_c = self.netC.surface_classifier.packed()
        r = self.res[-1]
        n = self.n_active
        if not self.hwc_direct:
            for b in range(n * self.views):
                ops.pack_features(feat[b:b + 1], out=self.feats_hwc[b])
        if self.tables is not None:  # f32 / f16x3 heads blend table rows (query_table.hip, query16.hip)
            # (re)made after every encoder pass; the handle of the previous pass unregisters the same
            # pointers only if they still point at its table views, so dropping it here is harmless
            self._table_handle = ops.skip_table_batch(mlp, self.feat_hwc_all[:n], out=self.tables[:n])
        self._octree(mlp, n)
        pts_all = []
        # forward_vertices and the normal renders of all frames of the slot: one set of launches each
        # (mp_forward_vertices_batch, mp_paint_batch), results identical to the per-frame calls
        if VERTEX_BATCH:
            raws, renders = [], []
            for b0 in range(0, n, VERTEX_BATCH):
                rw = ops.forward_vertices_raw_batch(self.volumes[b0:min(b0 + VERTEX_BATCH, n)], "front")
                raws += rw
                renders += ops.paint_batch([v[0] for v in rw], [v[1] for v in rw], [v[3] for v in rw], 0,
                                           [v[4] for v in rw], r, 0.5, 0.5, 0.0, 1.0)
        else:  # A/B: one set of launches per frame
            raws = [ops.forward_vertices_raw(self.volumes[b], "front") for b in range(n)]
            renders = [ops.paint(v[0], v[1], v[3], 0, v[4], r, 0.5, 0.5, 0.0, 1.0) for v in raws]
        for b in range(n):
            x, y, z, nrm, count = raws[b]
            self.vertices[b] = raws[b]
            self.renders[b] = renders[b]
            if self.netC is not None:
                self._pack_colour_maps(b, feat, feat_c)
                pts_all.append(ops.vertex_points(x, y, z, count, r, self.mat_color))
        if self.netC is not None:
            # netC.query on the visible vertices (RTL/main.py:231-248) of ALL frames of the slot:
            # one fused-query launch per chunk of frames (14 k points per frame alone would
            # leave most CUs idle)
            step = self._colour_chunk()
            for b0 in range(0, n, step):
                b1 = min(b0 + step, n)
                preds = self._colour_query(mlp_c, b0, b1, pts_all[b0:b1], [self.vertices[b][4] for b in range(b0, b1)])
                tex = ops.paint_batch([self.vertices[b][0] for b in range(b0, b1)], [self.vertices[b][1] for b in range(b0, b1)],
                                      preds, 1, [self.vertices[b][4] for b in range(b0, b1)], r, 0.5, 0.5, -np.inf, np.inf)
                for b in range(b0, b1):
                    self.renders_tex[b] = tex[b - b0]
        if self.mesh is not None:
            self._mesh_chain(n)
        if self.picture_options is not None:
            self._render_pictures(n)
        if self.jpeg is not None:
            self._encode_pictures(n)
        if self.png is not None:
            self._encode_png(n)

    # the netC pieces of the chain that depend on the head's views (ColorViewsSlot overrides them)
    def _pack_colour_maps(self, b, feat, feat_c):
        """Frame b's netC map: netC.filter(image_c, feat_prior=featG_last) -> cat([prior, featC]) (MonoPortNet.py:41-45)
        packed straight into one channels-last map per frame."""
        ops.pack_features([feat[b:b + 1], feat_c[b:b + 1]], out=self.feats_hwc_c[b])

    def _colour_chunk(self):
        """Frames per colour-query launch."""
        return MAX_RECON_BATCH

    def _colour_query(self, mlp_c, b0, b1, pts, counts, outs=None):
        """netC's predictions [3,cap] at the counted points of frames b0..b1, one launch (``outs``: into these)."""
        return ops.query_counted_batch(mlp_c, self.feats_hwc_c[b0:b1], pts, counts, self.calib[b0:b1], Z_SCALE,
                                       outs=outs)

    def _picture_colours(self, n):
        """``ops.render_netc_batch``'s query over the slot's n frames: the ``_colour_query`` hook per chunk of frames,
        into the static predictions.  A frame's ``views`` pictures are one list, so the hook's per-frame maps and
        calibrations are the list's."""
        mlp_c = self.netC.surface_classifier.packed()
        step = self._colour_chunk()
        outs = list(self.picture_lists["preds"][:n])

        def query(pts, counts):
            for b0 in range(0, n, step):
                b1 = min(b0 + step, n)
                self._colour_query(mlp_c, b0, b1, pts[b0:b1], counts[b0:b1], outs=outs[b0:b1])
            return outs
        return query

    def _render_pictures(self, n):
        """The pictures of the slot's n frames under their ``views`` cameras each, from the mesh buffers the chain has
        just filled and its device counts, into the slot's static buffers: ``recon._shadow_maps`` (with a light in the
        scene), ``recon._subject_pictures`` and ``recon._scene_pictures`` (with a scene) with ``out=`` the slot's
        buffers -- what ``recon.render_mesh_many(_in_scene)`` enqueues, in the same order, with no host value in
        between.  A gated-off frame's counts are (0, 0): pure background, an uncovered shadow map, a picture that keeps
        its bits under the lighting.  With ``lighting.transfer`` the transfer of the n frames' vertices is traced
        first, through the bits the mesh chain packed.  The shadowed scene goes to ``scene_lit``; ``scene_image``
        stays unshadowed for ``_rerun_picture``."""
        from .recon import _chain_subjects, _resolved_pictures, _shadow_maps
        po, chains, cams = self.picture_options, self._mesh_chains[:n], list(self._cameras[:n])
        light = po.scene.light if hasattr(self, "scene_lit") else None
        image, depth, face, mask = self._working_pictures()
        out = {"image": None if image is None else image[:n], "depth": depth[:n], "face": face[:n]}
        if po.shade == "netC":
            out["lists"] = tuple(self.picture_lists[k][:n] for k in ("points", "pixels", "count"))
        transfers = None
        if self.lighting is not None:
            out["light"] = {k: getattr(self, "light_" + k)[:n] for k in ("normal", "face", "pos", "shade", "ambient")
                            if hasattr(self, "light_" + k)}
            if self._traces:
                cap = chains[0].verts.shape[0]  # the chain's capacity: the leading rows of the slot's buffers
                transfers = self._trace(chains, self.transfer_bits[:n], self.transfer_prt[:n, :cap])
                out["light"]["transfer_shade"] = self.transfer_shade[:n, :cap]
        subjects = _chain_subjects(chains, po.shade, transfers)
        maps = None if light is None else _shadow_maps("FrameSlot", subjects, light,
                                                       (self.shadow_depth[:n], self.shadow_face[:n]))
        if po.scene is not None:  # the scene under the same cameras, then the composite in place
            names = ("scene_image", "scene_depth", "scene_face", "scene_uv", "scene_pos", "scene_lit")
            out.update({k: getattr(self, k)[:n] for k in names if hasattr(self, k)})
            out.update(pictures_image=image[:n], pictures_depth=depth[:n], pictures_mask=mask[:n])
        if po.samples > 1:  # the resolve, behind the composite (the lighting without a scene), into the pictures_*
            out["resolved"] = tuple(None if t is None else t[:n] for t in (
                self.pictures_image, self.pictures_depth, self.pictures_face, self.pictures_mask, self.pictures_coverage))
        _resolved_pictures("FrameSlot", subjects, cams, po.raster, po.shade,
                           self._picture_colours(n) if po.shade == "netC" else None, self.lighting,
                           None if light is None else (light,) + maps, po.scene, maps, po.composite, out=out)

    def _working_pictures(self):
        """(image, depth, face, mask) that the passes and the composite write: the ``pictures_*`` themselves, or with
        ``samples`` > 1 the ``fine_*`` at ``samples`` times the size, which the resolve then reads."""
        if self.picture_options.samples > 1:
            return self.fine_image, self.fine_depth, self.fine_face, self.fine_mask
        return self.pictures_image, self.pictures_depth, self.pictures_face, self.pictures_mask

    def _trace(self, chains, bits, out):
        """The radiance transfer [cap,9] of the chains' vertices through their frames' ``bits`` (``out``: into it)."""
        t = self.lighting.transfer
        r = self.res[-1]
        bias_w, step_w, steps = t.rays(r, self.b_min, self.b_max)
        dirs, basis = t.tables(self.device)
        return [p[1] for p in ops.mesh_transfer_raw_batch(
            [c.verts for c in chains], [c.normals for c in chains], [c.counts for c in chains], list(bits), r,
            self.b_min, self.b_max, dirs, basis, t.weight, bias_w, step_w, steps, want=(False, True),
            out=None if out is None else (None, out))]

    def _with_transfer(self, b, mesh):
        """A re-run frame's mesh with the transfer ``meshes()`` traced for it, where the lighting wants one."""
        if mesh is None or not self._traces:
            return mesh
        from .recon import with_transfer
        return with_transfer(mesh, self._reran_transfer[b][:mesh.verts.shape[0]])

    def pictures(self):
        """The pictures of the current submission, to be called after ``wait()`` (it waits if the caller has not): a
        list of ``n_active`` entries, a ``recon.MeshRender`` per frame (image [views,H,W,3] or None, depth and face
        [views,H,W]) or None where ``meshes()`` gives None.  The entries are views of the slot's buffers, valid until
        the next ``submit``.  It goes through ``meshes()`` (its one device-to-host copy): a frame whose mesh
        overflowed the slot's capacities is rendered again from the re-run mesh (``_rerun_picture``), into fresh
        tensors: the bits the slot's own launch would have given at a sufficient capacity, except with
        ``shade="colors"``, where the re-run interpolates the Mesh's finished colours and the slot netC's raw
        predictions (the same picture, not the same last bits); with ``shade="netC"`` they are the same bits again,
        because both paths query netC at the same points.  No slot has overflowed 12 r^2 / 24 r^2 so far.  With a
        ``scene`` every entry is a ``recon.ScenePicture`` (image, depth, face, mask) of the subject composited over the
        scene -- the bare scene where ``meshes()`` gives None --, and a re-rendered frame is composited again over the
        slot's own picture of the scene.  With ``samples`` > 1 every entry is a ``recon.ResolvedPicture`` (image, depth,
        face, mask -- None without a scene --, coverage), views of the resolved ``pictures_*`` buffers; a re-rendered
        frame goes through the same fine passes and its own resolve."""
        if self.picture_options is None:
            raise RuntimeError("FrameSlot.pictures(): the slot was made without pictures=...")
        from .recon import MeshRender, ResolvedPicture, ScenePicture
        out = []
        for b, mesh in enumerate(self.meshes()):
            if mesh is not None and b in self._reran:
                out.append(self._rerun_picture(b, self._with_transfer(b, mesh)))
            elif self.picture_options.samples > 1:
                out.append(None if mesh is None and self.picture_options.scene is None else ResolvedPicture(
                    None if self.pictures_image is None else self.pictures_image[b], self.pictures_depth[b],
                    self.pictures_face[b], None if self.pictures_mask is None else self.pictures_mask[b],
                    self.pictures_coverage[b]))
            elif self.picture_options.scene is not None:
                out.append(ScenePicture(self.pictures_image[b], self.pictures_depth[b], self.pictures_face[b],
                                        self.pictures_mask[b]))
            else:
                out.append(None if mesh is None else MeshRender(
                    None if self.pictures_image is None else self.pictures_image[b], self.pictures_depth[b],
                    self.pictures_face[b]))
        return out

    def encode_pictures(self, jpeg):
        """Encode the slot's pictures on the device from now on: ``jpeg`` is a ``recon.Jpeg`` or a ``recon.Png``; a slot
        may have one of each.  To be called before the first ``prepare`` / ``submit``; a Jpeg and a Png of the image need
        pictures with a ``shade``.  The slot then owns the static ``jpeg_bytes`` [batch * views, capacity] uint8 (the
        codec's ``capacity_for`` the pictures' size) and ``jpeg_info`` [batch * views, 2] int32 -- ``png_bytes`` and
        ``png_info`` for a Png --, and the chain enqueues ONE mp_picture_jpeg (mp_picture_png) over the active frames'
        pictures behind ``_render_pictures`` on the slot's stream -- behind the composite with a scene, behind the
        lighting without one, behind the resolve with ``samples`` -- with no host value in between; ``jpegs()``
        (``pngs()``) hands the files out.  A Png with ``alpha="coverage"`` needs ``samples`` > 1; with
        ``alpha="subject"`` the slot also owns ``png_alpha`` [batch, views, H, W] f32, filled by one op per submission.
        A slot on which this was never called allocates and enqueues nothing for it."""
        from .recon import Jpeg, Png
        who = "%s.encode_pictures" % type(self).__name__
        if not isinstance(jpeg, (Jpeg, Png)):
            raise ValueError("%s: jpeg must be a recon.Jpeg (or a recon.Png), got %r" % (who, type(jpeg).__name__))
        po = self.picture_options
        if po is None:
            raise ValueError("%s: the slot was made without pictures=..." % who)
        depth = isinstance(jpeg, Png) and jpeg.plane == "depth"
        if po.shade is None and not depth:
            raise ValueError("%s: the slot's pictures have shade=None: there is no image to encode" % who)
        if isinstance(jpeg, Png) and jpeg.alpha == "coverage" and po.samples < 2:
            raise ValueError("%s: alpha='coverage' needs pictures with samples > 1" % who)
        if self._chained:
            raise RuntimeError("%s: to be called before the first prepare / submit" % who)
        n = self.batch * po.views
        out = torch.empty((n, jpeg.capacity_for(*po.res)), dtype=torch.uint8, device=self.device)
        info = torch.zeros((n, 2), dtype=torch.int32, device=self.device)
        if isinstance(jpeg, Jpeg):
            self.jpeg_bytes, self.jpeg_info, self.jpeg = out, info, jpeg
            return
        if jpeg.alpha == "subject":
            self.png_alpha = torch.empty((self.batch, po.views) + po.res, dtype=torch.float32, device=self.device)
        self.png_bytes, self.png_info, self.png = out, info, jpeg

    def _encode_pictures(self, n):
        """One mp_picture_jpeg over the n active frames' pictures: they are one contiguous [n * views,H,W,3] block."""
        po, j = self.picture_options, self.jpeg
        rows = n * po.views
        ops.picture_jpeg_raw(self.pictures_image[:n].view((rows,) + po.res + (3,)), j.quality, j.subsampling, j.restart,
                             out=self.jpeg_bytes[:rows], info=self.jpeg_info[:rows])

    def _png_planes(self, n):
        """(planes, alpha) of the n active frames for mp_picture_png: contiguous views of the slot's buffers."""
        from .recon import _subject_alpha
        po, p = self.picture_options, self.png
        rows = (n * po.views,) + po.res
        alpha = None
        if p.alpha == "coverage":
            alpha = self.pictures_coverage[:n].view(rows)
        elif p.alpha == "subject":
            mask = None if self.pictures_mask is None else self.pictures_mask[:n]
            alpha = _subject_alpha(mask, self.pictures_face[:n], out=self.png_alpha[:n]).view(rows)
        if p.plane == "depth":
            return self.pictures_depth[:n].view(rows), alpha
        return self.pictures_image[:n].view(rows + (3,)), alpha

    def _encode_png(self, n):
        """One mp_picture_png over the n active frames' pictures."""
        from .recon import _png_raw
        rows = n * self.picture_options.views
        planes, alpha = self._png_planes(n)
        _png_raw(self.png, planes, alpha, out=self.png_bytes[:rows], info=self.png_info[:rows])

    def _encoded(self, out, info, encode):
        """The files an encoding call of the chain left in ``out`` / ``info`` for the current submission: a list of
        ``n_active`` entries, each a list of ``views`` ``bytes``, or None where ``pictures()`` gives None.  One
        device-to-host copy of ``info`` and one of the used prefixes of ``out``.  A frame whose mesh ``meshes()`` made
        again, or one of whose files exceeded the capacity, is encoded from the picture ``pictures()`` returns
        (``encode(picture)``): the same bytes a sufficient capacity gives."""
        from .recon import _collect_files
        pictures = self.pictures()
        v = self.picture_options.views
        rows = self.n_active * v
        info = info[:rows].cpu().numpy()
        again = [pic is not None and (b in self._reran or bool(info[b * v:(b + 1) * v, 1].any()))
                 for b, pic in enumerate(pictures)]
        mine = info.copy()
        for b, pic in enumerate(pictures):
            if pic is None or again[b]:
                mine[b * v:(b + 1) * v] = (0, 0)  # nothing of these rows is copied
        files = _collect_files(type(self).__name__, out, mine, None)
        return [None if pic is None else (encode(pic) if again[b] else files[b * v:(b + 1) * v])
                for b, pic in enumerate(pictures)]

    def jpegs(self):
        """The JPEG files of the current submission's pictures, to be called after ``wait()`` (it waits if the caller
        has not): a list of ``n_active`` entries, each a list of ``views`` ``bytes``, or None where ``pictures()`` gives
        None.  One device-to-host copy of ``jpeg_info`` and one of the used prefixes of ``jpeg_bytes`` (besides
        ``meshes()``' own).  A frame whose mesh ``meshes()`` made again, or one of whose files exceeded the capacity,
        is encoded from the picture ``pictures()`` returns (``recon.encode_jpeg``): the same bytes a sufficient
        capacity gives."""
        if self.jpeg is None:
            raise RuntimeError("%s.jpegs(): encode_pictures(jpeg) was never called on this slot" % type(self).__name__)
        from .recon import encode_jpeg
        return self._encoded(self.jpeg_bytes, self.jpeg_info, lambda pic: encode_jpeg(pic.image, self.jpeg))

    def pngs(self):
        """The PNG files of the current submission's pictures: what ``jpegs()`` is for a ``recon.Jpeg``, for the slot's
        ``recon.Png``, with ``recon.encode_png`` for the frames that are encoded again."""
        if self.png is None:
            raise RuntimeError("%s.pngs(): encode_pictures(png) was never called on this slot" % type(self).__name__)
        from .recon import encode_png
        return self._encoded(self.png_bytes, self.png_info, lambda pic: encode_png(pic, self.png))

    def _rerun_picture(self, b, mesh):
        """Frame b again from its re-run ``Mesh``, into fresh tensors: the bodies of ``_render_pictures`` on the
        subjects of ``[mesh]`` with ``out=None`` -- netC bound to the slot's own maps, the shadow map made afresh for
        this mesh, and the slot's own unshadowed picture of the scene (and its positions) as the back picture."""
        from .recon import (MeshRender, ResolvedPicture, ScenePicture, _counted_colours, _mesh_subjects,
                            _resolved_pictures, _shadow_maps)
        po, who, cams = self.picture_options, "FrameSlot.pictures", [self._cameras[b]]
        subjects = _mesh_subjects(who, [mesh], po.shade, self.lighting)
        colours = None
        if po.shade == "netC":  # recon.render_mesh(shade="netC") on the slot's own maps
            bindings = self._colour_bindings(b, b + 1)

            def colours(pts, counts):
                return _counted_colours(bindings, pts, counts, view=self.view)
        light = po.scene.light if hasattr(self, "scene_lit") else None
        maps = None if light is None else _shadow_maps(who, subjects, light)
        back = None
        if po.scene is not None:
            back = ([self.scene_image[b]], [self.scene_depth[b]], [self.scene_face[b]],
                    None if light is None else [self.scene_pos[b]])
        fronts, done, resolved = _resolved_pictures(who, subjects, cams, po.raster, po.shade, colours, self.lighting,
                                                    None if light is None else (light,) + maps, po.scene, maps,
                                                    po.composite, back=back)
        if resolved is not None:
            return ResolvedPicture(*resolved[0])
        if po.scene is None:
            return MeshRender(*fronts[0])
        image, depth, mask = done[0]
        return ScenePicture(image, depth, fronts[0][2], mask)

    def _slot_cameras(self, cameras, n):
        """``submit``'s cameras ([n,views,>=3,4], or [views,>=3,4] / [>=3,4] shared by all frames; tensor or array)
        -> host float32 [n,views,3,4].  Read on the host, as the rasteriser's calibrations are."""
        po = self.picture_options
        c = cameras.detach().cpu().numpy() if torch.is_tensor(cameras) else np.asarray(cameras)
        c = np.asarray(c, np.float32)
        if c.ndim == 2:
            c = c[None]
        if c.ndim == 3:
            c = np.broadcast_to(c[None], (n,) + c.shape)
        if c.ndim != 4 or c.shape[0] != n or c.shape[1] != po.views or c.shape[2] < 3 or c.shape[3] != 4:
            raise ValueError("submit: cameras must be [%d,%d,4,4] (or [%d,4,4] for all frames), got %s"
                             % (n, po.views, po.views, tuple(np.shape(cameras))))
        return np.ascontiguousarray(c[:, :, :3, :])

    def _mesh_bindings(self, b0, b1):
        """The colour queries of frames b0..b1 as recon._mesh_chains takes them (netC's head on the slot's own maps and
        calibrations), None without colours."""
        return self._colour_bindings(b0, b1) if self.mesh.colors else None

    def _colour_bindings(self, b0, b1):
        """netC's head on the slot's own maps and calibrations, one query binding per frame b0..b1."""
        from .modeling.MonoPortNet import QueryBinding
        mlp_c = self.netC.surface_classifier.packed()
        return [QueryBinding(self.netC, mlp_c, self.feats_hwc_c[b], self.calib[b:b + 1], Z_SCALE)
                for b in range(b0, b1)]

    def _mesh_chunk(self):
        """Frames per set of launches of the mesh chain."""
        return MESH_BATCH

    def _mesh_chain(self, n):
        """Marching cubes -> normals -> points -> netC colours of the slot's n frames into the slot's mesh buffers,
        MESH_BATCH frames per set of launches, each frame gated by its status[b, 0] (the volume of a frame whose
        coarsest octree level is empty is unspecified: its counts become (0, 0) and nothing else of it is touched).  With
        ``clean`` the chain starts with recon.keep_largest of the chunk's volumes, under the same gates."""
        from .recon import _mesh_chains
        chunk = self._mesh_chunk()
        if self.mesh.clean is not None:  # one chunk's cleaned volumes at a time, in the same buffer
            chunk = min(chunk, self.mesh_buffers["cleaned"].shape[0])
        for b0 in range(0, n, chunk):
            b1 = min(b0 + chunk, n)
            out = {k: v[b0:b1] for k, v in self.mesh_buffers.items()}
            if self.mesh.clean is not None:
                out["cleaned"] = self.mesh_buffers["cleaned"][:b1 - b0]
            if self.mesh.colors:
                out["preds"] = list(out["preds"])
            self._mesh_chains[b0:b1] = _mesh_chains(
                self.volumes[b0:b1], self.b_min, self.b_max, self.mesh, self._mesh_bindings(b0, b1),
                gates=[self.status[b, 0:1] for b in range(b0, b1)], out=out, view=self.view,
                bits_out=self.transfer_bits[b0:b1] if self._traces else None)
            if self.glb is not None:
                self._encode_meshes(b0, b1)

    def encode_meshes(self, glb):
        """Encode the slot's meshes on the device from now on: ``glb`` is a ``recon.Glb``.  To be called before the first
        ``prepare`` / ``submit``, on a slot with ``mesh=...`` whose options provide what ``glb`` asks for (normals,
        colours).  The slot then owns the static ``glb_bytes`` [batch, capacity] uint8 (``glb.capacity_for`` the mesh
        buffers' capacities) and ``glb_info`` [batch, 2] int32, and the chain enqueues ONE mp_mesh_glb_batch per chunk
        of the mesh chain, behind that chunk on the slot's stream, with no host value in between: the chain's raw netC
        predictions go in as planes with (0.5, 0.5), which gives the bytes of the finished colours.  ``glbs()`` hands the
        files out.  A slot on which this was never called allocates and enqueues nothing for it.

        With ``glb.texture`` (a ``recon.Atlas`` of side A) the slot needs its ``netC`` -- not the mesh's colours: with
        ``mesh={"colors": False}`` the per-vertex query is never enqueued -- and also owns ``atlas_face`` [batch,A,A],
        ``atlas_image`` [batch,A,A,3], ``atlas_info`` [batch,2], the point / pixel / prediction / count lists of A^2
        entries per frame (``atlas_lists``), ``atlas_png`` [batch, the atlas's PNG capacity] and ``atlas_png_info``.
        Behind each chunk of the mesh chain it then enqueues the atlas, the covered texels' lists, netC through the
        ``_colour_query`` hook (a ``ColorViewsSlot``'s with its ``view``), the paint, one mp_picture_png and one
        mp_mesh_glb_textured_batch.  A slot with a plain ``Glb`` has none of these attributes."""
        from .recon import Glb
        who = "%s.encode_meshes" % type(self).__name__
        if not isinstance(glb, Glb):
            raise ValueError("%s: glb must be a recon.Glb, got %r" % (who, type(glb).__name__))
        if self.mesh is None:
            raise ValueError("%s: the slot was made without mesh=..." % who)
        if glb.normals and self.mesh.normals is None:
            raise ValueError("%s: glb asks for normals and the slot's meshes have none (mesh normals=None)" % who)
        if glb.colors and not self.mesh.colors:
            raise ValueError("%s: glb asks for colors and the slot's meshes have none (no netC, or colors=False)" % who)
        if glb.texture is not None and self.netC is None:
            raise ValueError("%s: glb.texture is baked from netC, which this slot does not run" % who)
        if self._chained:
            raise RuntimeError("%s: to be called before the first prepare / submit" % who)
        cap_v, cap_f = self.mesh_buffers["verts"].shape[1], self.mesh_buffers["faces"].shape[1]
        self.glb_bytes = torch.empty((self.batch, glb.capacity_for(cap_v, cap_f)), dtype=torch.uint8,
                                     device=self.device)
        self.glb_info = torch.zeros((self.batch, 2), dtype=torch.int32, device=self.device)
        if glb.texture is not None:  # 28 bytes per texel of lists, as ``picture_lists``, and 16 of pictures
            b, a, dev = self.batch, glb.texture.size, self.device
            self.atlas_face = torch.empty((b, a, a), dtype=torch.int32, device=dev)
            self.atlas_image = torch.empty((b, a, a, 3), dtype=torch.float32, device=dev)
            self.atlas_info = torch.zeros((b, 2), dtype=torch.int32, device=dev)
            self.atlas_lists = {"points": torch.zeros((b, 3, a * a), dtype=torch.float32, device=dev),
                                "pixels": torch.zeros((b, a * a), dtype=torch.int32, device=dev),
                                "preds": torch.zeros((b, 3, a * a), dtype=torch.float32, device=dev),
                                "count": torch.zeros((b, 2), dtype=torch.int32, device=dev)}
            self.atlas_png = torch.empty((b, glb.texture.png_capacity()), dtype=torch.uint8, device=dev)
            self.atlas_png_info = torch.zeros((b, 2), dtype=torch.int32, device=dev)
        self.glb = glb

    def _encode_meshes(self, b0, b1):
        """One mp_mesh_glb_batch over the chains of frames b0..b1 as the chunk left them."""
        chains = self._mesh_chains[b0:b1]
        if self.glb.texture is not None:
            return self._encode_textured_meshes(b0, b1)
        ops.mesh_glb_raw_batch([c.verts for c in chains], [c.faces for c in chains], [c.counts for c in chains],
                               [c.normals for c in chains] if self.glb.normals else None,
                               [c.preds for c in chains] if self.glb.colors else None, "planes", 0.5, 0.5,
                               self.b_min, self.b_max, out=self.glb_bytes[b0:b1], info=self.glb_info[b0:b1])

    def _encode_textured_meshes(self, b0, b1):
        """The textured files of frames b0..b1 behind their chunk of the mesh chain, into the slot's static buffers, with
        no host value in between: ``recon._bake`` (one mp_mesh_atlas_batch, the covered texels' lists, the
        ``_colour_query`` hook per chunk of frames, the paint), ONE mp_picture_png, ONE mp_mesh_glb_textured_batch."""
        from .recon import _bake, _chain_subjects, _png_raw
        who, atlas, chains = "%s.encode_meshes" % type(self).__name__, self.glb.texture, self._mesh_chains[b0:b1]
        mlp_c = self.netC.surface_classifier.packed()
        step = self._colour_chunk()
        outs = list(self.atlas_lists["preds"][b0:b1])

        def query(pts, counts):
            for c0 in range(0, b1 - b0, step):
                c1 = min(c0 + step, b1 - b0)
                self._colour_query(mlp_c, b0 + c0, b0 + c1, pts[c0:c1], counts[c0:c1], outs=outs[c0:c1])
            return outs
        out = dict(face=self.atlas_face[b0:b1], image=self.atlas_image[b0:b1], info=self.atlas_info[b0:b1],
                   lists=tuple(self.atlas_lists[k][b0:b1] for k in ("points", "pixels", "count")))
        _bake(who, _chain_subjects(chains, None), atlas, query, out)
        _png_raw(atlas.png, self.atlas_image[b0:b1], None, out=self.atlas_png[b0:b1], info=self.atlas_png_info[b0:b1])
        ops.mesh_glb_textured_raw_batch([c.verts for c in chains], [c.faces for c in chains], [c.counts for c in chains],
                                        atlas.size, atlas.cell, self.atlas_png[b0:b1], self.atlas_png_info[b0:b1],
                                        [c.normals for c in chains] if self.glb.normals else None, None, self.b_min,
                                        self.b_max, out=self.glb_bytes[b0:b1], info=self.glb_info[b0:b1])

    def _glb_again(self, b, mesh):
        """Frame b's file from its ``Mesh`` at the file's own size: ``recon.encode_glb``; a textured one with the
        slot's own maps and calibration (``_colour_bindings``)."""
        from .recon import Glb, _counted_colours, _encode_glb_textured, encode_glb
        exact = Glb(self.glb.normals, self.glb.colors, texture=self.glb.texture)  # no second overflow
        if self.glb.texture is None:
            return encode_glb(mesh, exact, self.b_min, self.b_max)
        bindings = self._colour_bindings(b, b + 1)
        return _encode_glb_textured("%s.glbs" % type(self).__name__, [mesh], exact, self.b_min, self.b_max,
                                    lambda pts, counts: _counted_colours(bindings, pts, counts, view=self.view or 0))[0]

    def glbs(self):
        """The binary glTF files of the current submission's meshes, to be called after ``wait()`` (it waits if the
        caller has not): a list of ``n_active`` entries, ``bytes`` per frame or None where ``meshes()`` gives None.  One
        device-to-host copy of ``glb_info`` and one of the used prefixes of ``glb_bytes`` (besides ``meshes()``' own).  A
        frame whose mesh ``meshes()`` made again, or whose file exceeded the capacity, is encoded from its ``Mesh``
        (``recon.encode_glb``): the same bytes a sufficient capacity gives.  With ``glb.texture`` such a frame's texture
        is baked again with the slot's own maps and calibration, and so is one whose image exceeded the atlas's PNG
        capacity; a mesh with more faces than the atlas holds raises a ValueError that names both numbers."""
        if self.glb is None:
            raise RuntimeError("%s.glbs(): encode_meshes(glb) was never called on this slot" % type(self).__name__)
        from .recon import _collect_files
        meshes = self.meshes()
        info = self.glb_info[:self.n_active].cpu().numpy()
        again = [m is not None and (b in self._reran or bool(info[b, 1])) for b, m in enumerate(meshes)]
        mine = info.copy()
        for b, m in enumerate(meshes):
            if m is None or again[b]:
                mine[b] = (0, 0)  # nothing of this row is copied
        files = _collect_files(type(self).__name__, self.glb_bytes, mine, None)
        return [None if m is None else (self._glb_again(b, m) if again[b] else files[b]) for b, m in enumerate(meshes)]

    def meshes(self):
        """The meshes of the current submission, to be called after ``wait()`` (it waits if the caller has not): a
        list of ``n_active`` entries, a ``recon.Mesh`` per frame or None where the frame's coarsest octree level
        was empty (status[b, 0] == 0).  ONE device-to-host copy (counts and status of all frames).  verts, faces and
        normals are views of the slot's buffers, valid until the next ``submit`` (colours are fresh tensors).  A
        frame whose mesh overflowed the slot's capacities (12 r^2 vertices, 24 r^2 faces) is re-run alone with
        exact capacities here: all of its tensors are then fresh ones."""
        if self.mesh is None:
            raise RuntimeError("FrameSlot.meshes(): the slot was made without mesh=...")
        from .recon import _collect_meshes, _mesh_chains
        self.wait()
        n = self.n_active
        self._reran = []
        self._reran_transfer = {}
        # per frame: alive, (vertices, faces) of the mesh [, with ``simplify``: those marching cubes needed]
        cols = [self.status[:n, 0:1], self.mesh_buffers["counts"][:n]]
        if self.mesh.simplify is not None:
            cols.insert(1, self.mesh_buffers["simple_counts"][:n])
        host = torch.cat(cols, dim=1).cpu().tolist()

        def rerun(b, max_verts, max_faces):
            self._reran.append(b)
            chain = _mesh_chains([self.volumes[b]], self.b_min, self.b_max, self.mesh, self._mesh_bindings(b, b + 1),
                                 max_verts=max_verts, max_faces=max_faces, view=self.view)[0]
            if self._traces:  # traced again through the frame's bits, which the slot still holds
                self._reran_transfer[b] = self._trace([chain], self.transfer_bits[b:b + 1], None)[0]
            return chain

        return _collect_meshes([chain if row[0] else None for chain, row in zip(self._mesh_chains, host)],
                               [row[1:] for row in host], rerun)

    def prepare(self, warmup=2):
        """Warm up (scratch arenas, GroupNorm accumulator arena); with ``use_graph`` capture the ENCODER into a
        hipGraph.  The C-ABI stages stay eager: they are a handful of asynchronous calls, and a
        graph that also holds them faulted on ROCm 7.2 once tensors were allocated after
        capture."""
        self.graph = None  # warm up eagerly with the CURRENT settings, then (re-)capture
        with torch.cuda.stream(self.stream):
            for _ in range(warmup):
                self._chain()
        self.stream.synchronize()
        if self.use_graph:
            graph = torch.cuda.CUDAGraph()
            # thread_local: RCCL's watchdog thread (multi-GPU runs) and the other slots' host
            # threads may touch the HIP runtime while this thread captures
            with torch.cuda.graph(graph, stream=self.stream, capture_error_mode="thread_local"):
                self._graph_feat = self._encode()
            self.stream.synchronize()
            self.graph = graph
            # first launch of an instantiated graph uploads it: keep that out of the caller's first frame
            with torch.cuda.stream(self.stream):
                self.graph.replay()
            self.stream.synchronize()

    def submit(self, images, calibs, images_c=None, cameras=None):
        """Enqueue the reconstruction of n <= ``batch`` frames: ``images`` [n,3,512,512] (or a list
        of [1,3,512,512]), ``calibs`` [n,4,4] (or a list of [1,4,4]); returns immediately.  ``cameras``: with
        ``pictures``, the free cameras of the frames' pictures, [n,views,4,4] or [views,4,4] for all frames (read
        on the host); required then, refused otherwise.  Results
        (``renders``, ``volumes``, ``status``, ``vertices``; entries 0..n-1) are valid after
        ``stream.synchronize()`` and until the next submit on this slot.  A short batch (the tail of
        a stream) still runs the encoder at the slot's batch size -- the graph is captured for it --
        on stale images in the unused entries; the octree and everything after it see n frames."""
        n = images.shape[0] if torch.is_tensor(images) else len(images)
        if not 1 <= n <= self.batch:
            raise ValueError("slot of %d frames got %d" % (self.batch, n))
        if (cameras is None) != (self.picture_options is None):
            raise ValueError("submit: cameras are %s" % ("required by the slot's pictures" if cameras is None else
                                                         "taken only by a slot made with pictures=..."))
        host_cameras = None if cameras is None else self._slot_cameras(cameras, n)
        self.wait()  # a slot holds ONE batch: its previous results are overwritten from here on
        self.n_active = n
        if host_cameras is not None:
            self._cameras[:n] = host_cameras
        # the caller may have produced the frames asynchronously on ITS stream (segmentation,
        # prepare_inputs, an H2D copy from pinned memory): order the slot's copies behind that work
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            self._load(self.image_in, images)
            self._load(self.calib_in, calibs)
            if self.netC is not None:
                self._load(self.image_c_in, images if images_c is None else images_c)
            self._chain()
        self._busy = True

    def _load(self, dst, src):
        if torch.is_tensor(src):
            n = src.shape[0]
            dst[:n].copy_(src.reshape(dst[:n].shape), non_blocking=True)
            srcs = [src]
        else:
            srcs = list(src)
            if len(srcs) > 1 and all(s.is_cuda and s.device == dst.device and s.dtype == dst.dtype for s in srcs):
                # one gather launch for the frames of a submission instead of one copy per frame
                torch.cat([s.reshape(dst[:1].shape) for s in srcs], out=dst[:len(srcs)])
            else:
                for b, s in enumerate(srcs):
                    dst[b].copy_(s.reshape(dst[b].shape), non_blocking=True)
        for s in srcs:
            if s.is_cuda:  # the caching allocator must not recycle a source the copy still reads
                s.record_stream(self.stream)

    def wait(self):
        """Block the host until this slot's batch (and anything queued after it on the slot's
        stream before the next submit) has finished.  Results are to be consumed after ``wait()``
        or on a stream that has done ``wait_stream(slot.stream)``."""
        if self._busy:
            self.stream.synchronize()
            self._busy = False

    def close(self):
        """Release the C-ABI scratch arena keyed by this slot's stream (mp_stream_release)."""
        self.wait()
        self.graph = None
        if self.tables is not None:
            if self._table_handle is not None:
                self._table_handle.release()
            self._table_handle = None
            self.tables = None
        ops.stream_release(self.stream)


class ViewsSlot(FrameSlot):
    """A FrameSlot for a MULTI-VIEW netG (SurfaceClassifier num_views = V > 1, multi-view PIFu): static buffers for
    ``batch`` in-flight frames of V views each.  ``submit(images [n,V,3,512,512], calibs [n,V,4,4])``; ONE encoder
    pass over the slot's batch * V images (``use_graph`` and the direct channels-last output as in FrameSlot), then the
    octree of all frames level by level through ``ops.recon_views_batch`` (mp_recon_views_batch: one launch of the
    multi-view kernel per level covers every frame of a chunk of ``ops.max_view_frames(V)``), then FrameSlot's
    per-volume stages unchanged: forward_vertices / paint renders and, with ``mesh={...}``, the mesh chain.

    ``view`` (0..V-1): the row of the [V,1,N] result the volumes hold -- the view-averaged prediction times that
    view's in-image mask (Seg3dLossless(fuse_views=True, view=...)); ``projection``: the one mode of all cameras.
    No skip tables (the multi-view kernel does not read them).  This slot runs no ``netC``: it and hence ``mesh``
    colours raise NotImplementedError at construction; ``ColorViewsSlot`` is the slot with a multi-view ``netC``."""

    def __init__(self, netG, device, *args, view=0, projection="orthogonal", **kwargs):
        self.view = int(view)
        self.projection = ops._projection(projection)
        super().__init__(netG, device, *args, **kwargs)

    def _netg_views(self, netG):
        v_n = netG.surface_classifier.num_views
        if v_n < 2:
            raise ValueError("%s: netG has a single-view head; use FrameSlot" % type(self).__name__)
        if not 0 <= self.view < v_n:
            raise ValueError("%s(view=%d): the head has %d views (rows 0..%d)"
                             % (type(self).__name__, self.view, v_n, v_n - 1))
        return v_n

    def _head_views(self, netG, netC, mesh):
        v_n = self._netg_views(netG)
        if netC is not None:
            raise NotImplementedError("ViewsSlot: netC (multi-view colours over device-counted vertex lists) is not built")
        colors = None if mesh is None else (mesh.get("colors") if isinstance(mesh, dict) else getattr(mesh, "colors", None))
        if colors:
            raise NotImplementedError("ViewsSlot(mesh=...): colours need netC, which the slot does not run")
        return v_n

    def _per_frame(self, buf):
        return buf.view(self.batch, self.views, *buf.shape[1:])

    def _octree(self, mlp, n):
        v_n = self.views
        step = ops.max_view_frames(v_n)
        maps = [self.feats_hwc[b * v_n:(b + 1) * v_n] for b in range(n)]
        for b0 in range(0, n, step):
            b1 = min(b0 + step, n)
            ops.recon_views_batch(mlp, maps[b0:b1], self.calib_in[b0:b1], self.projection, Z_SCALE, self.b_min,
                                  self.b_max, self.res, self.balance, final_level=self.final_level, view=self.view,
                                  volumes=self.volumes[b0:b1], status=self.status[b0:b1])


class ColorViewsSlot(ViewsSlot):
    """A ViewsSlot with a MULTI-VIEW netC (num_views = netG's V): the texture stages of FrameSlot for frames of V views.
    ``submit(images [n,V,3,512,512], calibs [n,V,4,4], images_c=None, cameras=None)``.  Behind the geometry of
    ViewsSlot: ONE netC encoder pass over the slot's batch * V images (``feat_prior`` = the netG map of the same image),
    packed into batch * V channels-last maps [128,128,512]; ``renders_tex`` from forward_vertices -> vertex_points ->
    ``ops.query_views_counted_batch`` (mp_query_views_counted_batch: the colours of all frames of a chunk in one launch
    of the multi-view kernel, on vertex lists counted on the device) -> paint_batch; and with ``mesh={"colors": True}``
    the mesh chain's colour query through ``ViewsBinding``s on the slot's own maps, which ``pictures={"shade":
    "colors"}`` rasterises unchanged.  The colours are row ``view`` of netC's [V,3,N] result: the view-averaged
    prediction under view ``view``'s in-image mask, the row the volumes hold of netG's.  Chunks:
    ``min(FrameSlot's chunk, ops.max_view_frames(V))`` frames.  A frame whose coarsest octree level is empty stays
    gated off: the counts it leaves on the device are 0, so it owns no tile of the colour launch."""

    def _head_views(self, netG, netC, mesh):
        v_n = self._netg_views(netG)
        if netC is None:
            raise ValueError("ColorViewsSlot: a multi-view netC is required (ViewsSlot is the slot without colours)")
        c_n = netC.surface_classifier.num_views
        if c_n != v_n:
            raise ValueError("ColorViewsSlot: netC has num_views = %d, netG has %d%s"
                             % (c_n, v_n, "; a single-view netC cannot colour frames of several views" if c_n < 2 else ""))
        return v_n

    def _pack_colour_maps(self, b, feat, feat_c):
        v_n = self.views
        for i in range(b * v_n, (b + 1) * v_n):
            ops.pack_features([feat[i:i + 1], feat_c[i:i + 1]], out=self.feats_hwc_c[i])

    def _colour_chunk(self):
        return min(MAX_RECON_BATCH, ops.max_view_frames(self.views))

    def _mesh_chunk(self):
        return min(MESH_BATCH, ops.max_view_frames(self.views))

    def _colour_maps(self, b0, b1):
        v_n = self.views
        return [self.feats_hwc_c[b * v_n:(b + 1) * v_n] for b in range(b0, b1)]

    def _colour_query(self, mlp_c, b0, b1, pts, counts, outs=None):
        return ops.query_views_counted_batch(mlp_c, self._colour_maps(b0, b1), pts, counts, self.calib_in[b0:b1],
                                             self.projection, Z_SCALE, view=self.view, outs=outs)

    def _colour_bindings(self, b0, b1):
        from .modeling.MonoPortNet import ViewsBinding
        mlp_c = self.netC.surface_classifier.packed()
        return [ViewsBinding(self.netC, mlp_c, maps, self.calib_in[b], Z_SCALE, self.projection)
                for b, maps in zip(range(b0, b1), self._colour_maps(b0, b1))]


class FramePipeline:
    """Round-robin over ``depth`` slots (``slot_class``: FrameSlot; ViewsSlot for a multi-view netG; ColorViewsSlot for
    a multi-view netG and netC) of ``batch`` frames each."""

    def __init__(self, netG, device, depth=2, batch=1, slot_class=FrameSlot, **slot_kwargs):
        self.slots = [slot_class(netG, device, batch=batch, **slot_kwargs) for _ in range(depth)]
        self.batch = int(batch)
        self.n_submitted = 0

    def prepare(self):
        for s in self.slots:
            s.prepare()

    def submit(self, images, calibs, images_c=None, cameras=None):
        slot = self.slots[self.n_submitted % len(self.slots)]
        slot.submit(images, calibs, images_c, cameras)
        self.n_submitted += 1
        return slot

    def encode_pictures(self, jpeg):
        """``FrameSlot.encode_pictures`` on every slot: before ``prepare`` / the first ``submit``."""
        for s in self.slots:
            s.encode_pictures(jpeg)

    def encode_meshes(self, glb):
        """``FrameSlot.encode_meshes`` on every slot: before ``prepare`` / the first ``submit``."""
        for s in self.slots:
            s.encode_meshes(glb)

    def synchronize(self):
        for s in self.slots:
            s.wait()
            s.stream.synchronize()

    def close(self):
        for s in self.slots:
            s.close()
