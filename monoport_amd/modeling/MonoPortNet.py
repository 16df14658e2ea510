"""MonoPortNet: the PIFu geometry / colour network wrapper (mirror of
monoport/lib/modeling/MonoPortNet.py, same constructor, attributes and method signatures).

``filter`` runs the image encoder once per frame as a chain of hand-written HIP kernels
(modeling/backbones.py over csrc/conv3x3.hip, convim2col.hip, encoder_ops.hip; torch ops only in
train mode / on CPU tensors).  ``query`` -- the hot path, called once per octree level on
10^4..10^5 points -- is one fused HIP kernel launch: projection, in-image mask, depth feature,
bilinear gather, the skip-connected MLP on f32 MFMA, final activation and mask.  Which kernel:
csrc/query_table.hip when the bound feature map has a skip table (``_skip_table`` below: the
octree engine's maps, and maps that have served 16 k points), else csrc/query.hip /
query_small.hip; netC (C = 512) always csrc/query.hip.
"""
import collections
import threading
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .backbones import PIFuHGFilters, PIFuResBlkFilters
from .geometry import index, orthogonal, perspective  # noqa: F401
from .heads import PIFuNetCMLP, PIFuNetGMLP
from .normalizers import PIFuNomalizer

# the reference resolves these names through globals() (MonoPortNet.py:23-28)
_REGISTRY = {
    "PIFuHGFilters": PIFuHGFilters,
    "PIFuResBlkFilters": PIFuResBlkFilters,
    "PIFuNetGMLP": PIFuNetGMLP,
    "PIFuNetCMLP": PIFuNetCMLP,
    "PIFuNomalizer": PIFuNomalizer,
    "orthogonal": orthogonal,
    "perspective": perspective,
}

_tls = threading.local()


class QueryBinding:
    """What one ``MonoPortNet.query`` call binds together for one frame: packed MLP + channels-last
    features + calibration + projection (ops.PROJECTIONS: MP_PROJ_*).  The octree engine records it once
    per frame and drives all levels natively."""

    batchable = True  # the frames of several such bindings can share one ops.recon_batch call

    def __init__(self, net, mlp, feat_hwc, calib, z_scale, projection=ops.PROJECTIONS["orthogonal"]):
        self.net, self.mlp, self.feat_hwc, self.calib, self.z_scale = net, mlp, feat_hwc, calib, z_scale
        self.projection = projection

    def trust_key(self, view=0):
        """What must stay the same between calls for Seg3dLossless to keep trusting a validated ``query_func``."""
        return (id(self.mlp), self.mlp.precision, float(self.z_scale), self.projection)

    def check_view(self, view):
        """One view: the engine's ``view`` is not looked at."""

    def recon(self, b_min, b_max, resolutions, balance, final_level, view=0, early=None, expect_level0=None):
        """The fused reconstruction of the bound frame (ops.recon) -> (volume, status) on the device."""
        return ops.recon(self.mlp, self.feat_hwc, self.calib, self.z_scale, b_min, b_max, resolutions, balance,
                         final_level=final_level, early=early, expect_level0=expect_level0,
                         projection=self.projection)


class ViewsBinding:
    """What one ``MonoPortNet.query`` call of a multi-view head (num_views = V > 1) binds together for one point
    set: packed MLP + the V views' channels-last maps + [V,4,4] calibrations + z scale + the one projection.  The
    octree engine records it (``record_query(views=True)``) and drives all levels through ops.recon_views."""

    batchable = False  # one point set per call (mp_recon_views)

    def __init__(self, net, mlp, maps, calibs, z_scale, projection=ops.PROJECTIONS["orthogonal"]):
        self.net, self.mlp, self.maps, self.calibs, self.z_scale = net, mlp, maps, calibs, z_scale
        self.projection = projection

    def trust_key(self, view=0):
        return (id(self.mlp), self.mlp.precision, float(self.z_scale), self.num_views, view, self.projection)

    def check_view(self, view):
        if view >= self.num_views:
            raise ValueError("Seg3dLossless(view=%d): the head has %d views (rows 0..%d)"
                             % (view, self.num_views, self.num_views - 1))

    def recon(self, b_min, b_max, resolutions, balance, final_level, view=0, early=None, expect_level0=None):
        """The fused reconstruction of the V bound views (ops.recon_views, row ``view``) -> (volume, status)."""
        return ops.recon_views(self.mlp, self.maps, self.calibs, self.projection, self.z_scale, b_min, b_max,
                               resolutions, balance, final_level=final_level, view=view, early=early,
                               expect_level0=expect_level0)

    @property
    def num_views(self):
        return len(self.maps)

    def batch_key(self, view=0):
        """Bindings with equal keys can share one ops.recon_views_batch call: the same head, V, ``view``, projection
        and map size.  (``batchable`` stays False: that flag says "a frame of ops.recon_batch".)"""
        return self.trust_key(view) + (tuple(self.maps[0].shape),)

    @staticmethod
    def batch_many(bindings, b_min, b_max, resolutions, balance, final_level, view=0, early_flags=None):
        """The fused reconstructions of several bindings with one ``batch_key``, ops.recon_views_batch in chunks of
        ``ops.max_view_frames(V)`` -> (volumes, status rows) on the device and, with ``early_flags`` (n ->
        ops.EarlyFlags for n frames), the frames' (non-empty, differs) flags [n,2] on the host: one wait per chunk,
        for its coarsest level only.  Results equal the per-frame ``recon`` calls bit for bit."""
        b0 = bindings[0]
        key = b0.batch_key(view)
        if any(b.batch_key(view) != key for b in bindings):
            raise ValueError("ViewsBinding.batch_many: the bindings differ in head, views, view, projection or map size")
        step = ops.max_view_frames(b0.num_views)
        volumes, rows, flags = [], [], []
        for f0 in range(0, len(bindings), step):
            chunk = bindings[f0:f0 + step]
            early = None if early_flags is None else early_flags(len(chunk))
            vols, status = ops.recon_views_batch(b0.mlp, [b.maps for b in chunk], [b.calibs for b in chunk],
                                                 b0.projection, b0.z_scale, b_min, b_max, resolutions, balance,
                                                 final_level=final_level, view=view, early=early)
            volumes += vols
            rows += list(status)
            if early is not None:
                flags.append(early.wait().clone())
        return volumes, rows, (torch.cat(flags) if flags else None)


class record_query:
    """Context manager (per host thread): counts the ``MonoPortNet.query`` calls made inside it
    and keeps the QueryBinding of the first one in ``.binding``.  The calls run normally.  With
    ``capture_only=True`` the first call returns zeros instead of launching (a probe).  Used by
    Seg3dLossless to see through an opaque ``query_func`` closure such as RTL/main.py:169-183.
    ``views=True``: the capture also takes the ViewsBinding of a multi-view head's call (by default
    such a call is counted and never bound)."""

    def __init__(self, capture_only=False, views=False):
        self.capture_only = capture_only
        self.views = views

    def __enter__(self):
        self.binding = None
        self.calls = 0
        self._prev = getattr(_tls, "capture", None)
        _tls.capture = self
        return self

    def __exit__(self, *exc):
        _tls.capture = self._prev
        return False


def capture_query():
    """Probe form of ``record_query`` (the first query call is recorded, not executed)."""
    return record_query(capture_only=True)


class _AttrDict(dict):
    """yacs-free stand-in for CfgNode in the factories below."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class MonoPortNet(nn.Module):
    def __init__(self, opt_net):
        super().__init__()
        self.opt = opt_net
        assert opt_net.projection in ["orthogonal", "perspective"]
        self.image_filter = _REGISTRY[opt_net.backbone.IMF](opt_net.backbone)
        self.surface_classifier = _REGISTRY[opt_net.head.IMF](opt_net.head)
        self.projection = _REGISTRY[opt_net.projection]
        self.normalizer = _REGISTRY[opt_net.normalizer.IMF](opt_net.normalizer)
        # per bound feature map, most recent last (a stage pipeline keeps several frames in flight, and a
        # coalescing recon stage binds up to 16 of them before it launches): key -> (weakrefs of the
        # source maps, packed channels-last map); id(packed) -> [packed, its version, mlp, skip table or
        # None, mlp generation, query points served so far]
        self._hwc_cache = collections.OrderedDict()
        self._table_cache = collections.OrderedDict()

    # ---- encoder ---------------------------------------------------------------------------------
    def filter(self, images, feat_prior=None):
        """images [B,3,512,512] -> list(stages) of list(levels) of [B,C,128,128]
        (MonoPortNet.py:31-46).  With ``feat_prior`` (netC) the prior is nearest-resized to
        128x128 and concatenated FIRST (:42-44)."""
        feats_stages = self.image_filter(images)
        if feat_prior is not None:
            feat_prior = F.interpolate(feat_prior, size=(128, 128))
            feats_stages = [[torch.cat([feat_prior, f], dim=1) for f in feats]
                            for feats in feats_stages]
        return feats_stages

    # ---- hot path --------------------------------------------------------------------------------
    MAX_BOUND_MAPS = ops.MAX_FRAMES  # packed maps / skip tables kept at most (a coalescing stage binds up to kMaxFrames)

    def _drop_dead_maps(self):
        """Forget the packed copy and the skip table (128 MB) of every feature map whose source tensors
        have been freed: the reference's one-frame-at-a-time usage then holds ONE map, a pipeline with k
        frames in flight k of them (the LRU bound only caps a caller that keeps every map alive)."""
        for key in [k for k, (refs, _) in self._hwc_cache.items() if any(r() is None for r in refs)]:
            _, packed = self._hwc_cache.pop(key)
            e = self._table_cache.pop(id(packed), None)
            if e is not None and e[3] is not None:
                e[3].release()

    def _packed_features(self, feats, frame=0):
        """Channels-last copy of frame ``frame`` of this stage's maps, cached per source tensors and frame
        so the five octree levels of one frame (and repeated calls) pack once."""
        key = (frame,) + tuple((f.data_ptr(), f._version, tuple(f.shape)) for f in feats)
        c = self._hwc_cache.get(key)
        if c is not None and all(r() is f for r, f in zip(c[0], feats)):
            self._hwc_cache.move_to_end(key)
            return c[1]
        self._drop_dead_maps()
        packed = ops.pack_features([f[frame:frame + 1] for f in feats] if feats[0].shape[0] != 1 else list(feats))
        self._hwc_cache[key] = ([weakref.ref(f) for f in feats], packed)
        while len(self._hwc_cache) > self.MAX_BOUND_MAPS:
            self._hwc_cache.popitem(last=False)
        return packed

    def bind(self, feats_stages, calibs, n_points=0, for_engine=False, frame=0):
        """QueryBinding for eval-mode queries against frame ``frame`` of ``feats_stages`` / ``calibs``.
        ``n_points``: how many points the caller is about to query; ``for_engine``: the caller is
        the octree engine (a whole reconstruction follows) -- both feed the decision whether the
        map gets a skip table (``_skip_table``)."""
        if self.surface_classifier.num_views > 1:
            # a binding is one frame on the single-view kernels (octree engine, skip tables, colour queries); a
            # multi-view head runs through query() only
            raise NotImplementedError("bind(): the head has num_views = %d; multi-view heads are served by query() "
                                      "(mp_query_views), not by the single-view engines" % self.surface_classifier.num_views)
        feats, calibs, projection, mlp = self._bind_common(feats_stages, calibs)
        if calibs.dim() == 3:  # [B,4,4]; one [4,4] (or none: the identity) serves every frame
            calibs = calibs[frame:frame + 1]
        packed = self._packed_features(feats, frame)
        self._skip_table(mlp, packed, int(n_points), for_engine)
        return QueryBinding(self, mlp, packed, calibs, self.normalizer.scale, projection)

    def _bind_common(self, feats_stages, calibs):
        """What ``bind`` and ``bind_views`` share -> (last stage's maps, calibs, projection, packed head): eval mode
        only; no calibration = identity under the orthogonal projection; head and maps on one GPU."""
        if self.training:
            raise NotImplementedError("monoport_amd implements the inference path (net.eval())")
        feats = list(feats_stages[-1])  # eval keeps the last stage only (MonoPortNet.py:63-64)
        dev = feats[0].device
        if calibs is None:
            # xyz = points (MonoPortNet.py:66-67): no projection at all, whatever opt_net.projection says
            calibs = torch.eye(4, device=dev)
            projection = ops.PROJECTIONS["orthogonal"]
        else:
            projection = ops.PROJECTIONS["perspective" if self.projection is perspective else "orthogonal"]
        mlp = self.surface_classifier.packed()
        if mlp.ctx.device_index != (dev.index if dev.index is not None else torch.cuda.current_device()):
            raise RuntimeError("surface_classifier and the feature maps must be on one GPU "
                               "(RTL/main.py:382-387 moves the features first)")
        return feats, calibs, projection, mlp

    def _skip_table(self, mlp, packed, n_points=0, for_engine=True):
        """The skip table of the bound feature map (ops.skip_table: the MLP's products with the
        sampled feature, taken once per texel instead of once per query point), registered for the
        map so that every query of the frame -- this module's and the octree engine's -- blends
        table rows.  A table costs 16 GFLOP / 126 MB whatever follows, the work of ~16 k plain-path
        points: it is made when the octree engine binds the map (a reconstruction of ~3e5 points
        follows) or once the map has served ops.SKIP_TABLE_MIN_POINTS query points; a few small
        ``query`` calls stay on the plain kernels (the two paths differ by f32 rounding, 1-5e-7).
        netG heads (C = 256) whose precision the C side routes through tables (ops.table_precision: exact
        f32 and f16x3; f16w / f16 measured slower through them and stay on the plain kernel, so no table
        is built for them); the table itself is always exact f32; MONOPORT_SKIP_TABLE=off (ops.SKIP_TABLE)
        switches it off.  The tables of live bound maps stay registered, at most MAX_BOUND_MAPS.
        Determinism: for plain ``query`` calls the threshold is CUMULATIVE per map, so the same call can
        return results that differ in the last bits (<= 5e-7, the distance between the two kernels) before
        and after the map has earned its table; MONOPORT_SKIP_TABLE_MIN_POINTS=0 (always) or
        MONOPORT_SKIP_TABLE=off (never) make every call take the same path."""
        cache = self._table_cache
        for k in [k for k, e in cache.items()  # entries of recycled / rewritten maps or of other weights
                  if e[0]._version != e[1] or e[2] is not mlp or e[4] != mlp.generation or not ops.SKIP_TABLE]:
            e = cache.pop(k)
            if e[3] is not None:
                e[3].release()
        e = cache.get(id(packed))
        if e is None or e[0] is not packed:
            e = cache[id(packed)] = [packed, packed._version, mlp, None, mlp.generation, 0]
        cache.move_to_end(id(packed))
        e[5] += n_points
        h, w, ch = packed.shape
        wanted = ops.SKIP_TABLE and ch == 256 and (h * w) % 64 == 0 and ops.table_precision(mlp.precision)
        if wanted and e[3] is None and (for_engine or e[5] >= ops.SKIP_TABLE_MIN_POINTS):
            # the handle keeps map and table alive and unregisters them when it is dropped
            e[3] = ops.skip_table(mlp, packed)
        while len(cache) > self.MAX_BOUND_MAPS:
            _, old = cache.popitem(last=False)
            if old[3] is not None:
                old[3].release()

    def has_skip_table(self, packed=None):
        """Whether the most recently bound map (or ``packed``) has a registered skip table."""
        if not self._table_cache:
            return False
        e = self._table_cache.get(id(packed)) if packed is not None else next(reversed(self._table_cache.values()))
        return e is not None and e[3] is not None

    def query(self, feats_stages, points, calibs=None, transforms=None):
        """points [B,3,N] world coords (any strides) -> [ [B,Cout,N] ] (MonoPortNet.py:48-91, eval mode).
        Out-of-image points come back as exactly 0 (:89); under the perspective projection a point with
        z == 0 comes back as NaN, as in the reference (0 * the NaN grid_sample samples there).  B > 1 runs as
        one mp_query_batch launch per ops.MAX_FRAMES frames; each frame's map keeps its own skip-table policy.
        A multi-view head (num_views = V > 1) takes points [V,3,N] of one point set and returns [V,Cout,N]
        (``_query_views``)."""
        if transforms is not None:
            raise NotImplementedError("query(transforms=...): the reference's own orthogonal() / perspective() "
                                      "fail on every shape of it (transforms[:2, 2:3] is empty, baddbmm raises)")
        cap = getattr(_tls, "capture", None)
        if points.dim() != 3 or points.shape[1] != 3:
            raise ValueError("points must be [B,3,N], got %s" % (tuple(points.shape),))
        if self.surface_classifier.num_views > 1:
            if cap is not None:
                # a binding only for a capture that asks for view bindings (Seg3dLossless(fuse_views=True)): the
                # default fused octree engine is single-view
                cap.calls += 1
                if cap.views and cap.binding is None:
                    self._check_view_rows(feats_stages, points, calibs)
                    cap.binding = self.bind_views(feats_stages, calibs)
                    if cap.capture_only:
                        return [torch.zeros((points.shape[0], cap.binding.mlp.cout, points.shape[2]),
                                            dtype=torch.float32, device=points.device)]
            return [self._query_views(feats_stages, points, calibs)]
        if points.shape[0] != 1:
            if cap is not None:
                cap.calls += 1  # B > 1 is not a binding of the fused octree engine (RTL/main.py:175 is B = 1)
            return [self._query_frames(feats_stages, points, calibs)]
        binding = self.bind(feats_stages, calibs, n_points=points.shape[2], for_engine=cap is not None)
        if cap is not None:
            cap.calls += 1
            if cap.binding is None:
                cap.binding = binding
                if cap.capture_only:
                    return [torch.zeros((points.shape[0], binding.mlp.cout, points.shape[2]),
                                        dtype=torch.float32, device=points.device)]
        return [ops.query(binding.mlp, binding.feat_hwc, points, binding.calib, binding.z_scale,
                          binding.projection)]

    def _query_frames(self, feats_stages, points, calibs):
        """B > 1: frame b of the features, calibrations and points -> out[b]; one launch per chunk of
        ops.MAX_FRAMES frames (a chunk's maps and skip tables stay bound until it has launched)."""
        b_n, n = points.shape[0], points.shape[2]
        feats = feats_stages[-1]
        if any(f.shape[0] != b_n for f in feats) or (calibs is not None and calibs.dim() == 3
                                                      and calibs.shape[0] != b_n):
            raise ValueError("query: %d point sets, feature maps of batch %s, calibrations %s"
                             % (b_n, [f.shape[0] for f in feats], None if calibs is None else tuple(calibs.shape)))
        out = None
        for b0 in range(0, b_n, ops.MAX_FRAMES):
            b1 = min(b_n, b0 + ops.MAX_FRAMES)
            bs = [self.bind(feats_stages, calibs, n_points=n, frame=b) for b in range(b0, b1)]
            if out is None:
                out = torch.empty((b_n, bs[0].mlp.cout, n), dtype=torch.float32, device=bs[0].feat_hwc.device)
            ops.query_batch(bs[0].mlp, [b.feat_hwc for b in bs], points[b0:b1], [b.calib for b in bs],
                            [b.projection for b in bs], bs[0].z_scale, out=out[b0:b1])
        return out

    def _query_views(self, feats_stages, points, calibs):
        """Multi-view head (SurfaceClassifier num_views = V > 1): rows = B*V views of B point sets.  The
        reference's result is [B*V,Cout,N] only for B = 1 (MonoPortNet.py:89 broadcasts in_img [B*V,1,N] against
        pred [B,Cout,N]); like it, B > 1 and rows that are not groups of V raise RuntimeError.  One
        mp_query_views launch; skip tables are not made or used."""
        self._check_view_rows(feats_stages, points, calibs)
        b = self.bind_views(feats_stages, calibs)
        return ops.query_views(b.mlp, b.maps, points, b.calibs, b.projection, b.z_scale)

    def _check_view_rows(self, feats_stages, points, calibs):
        """The shape rules of a multi-view query (see ``_query_views``)."""
        if self.training:
            raise NotImplementedError("monoport_amd implements the inference path (net.eval())")
        v_n, rows = self.surface_classifier.num_views, points.shape[0]
        if rows % v_n:
            raise RuntimeError("query: %d point rows are not groups of num_views = %d (the reference's "
                               "view(-1, %d, C, N) raises)" % (rows, v_n, v_n))
        if rows != v_n:
            raise RuntimeError("query: a multi-view head takes ONE point set of %d views; %d rows would be %d sets, "
                               "and the reference's in_img * pred cannot broadcast [%d,1,N] against [%d,Cout,N]"
                               % (v_n, rows, rows // v_n, rows, rows // v_n))
        feats = feats_stages[-1]
        if any(f.shape[0] != v_n for f in feats) or (calibs is not None and calibs.dim() == 3
                                                      and calibs.shape[0] != v_n):
            raise ValueError("query: %d views, feature maps of batch %s, calibrations %s"
                             % (v_n, [f.shape[0] for f in feats], None if calibs is None else tuple(calibs.shape)))

    def bind_views(self, feats_stages, calibs):
        """ViewsBinding for eval-mode queries of a multi-view head (num_views = V > 1) against the V views of
        ``feats_stages`` (batch V) / ``calibs`` ([V,4,4], one [4,4] for all views, or None).  No skip tables."""
        v_n = self.surface_classifier.num_views
        if v_n <= 1:
            raise NotImplementedError("bind_views(): the head has num_views = %d; single-view heads bind through "
                                      "bind()" % v_n)
        if any(f.shape[0] != v_n for f in feats_stages[-1]) or (calibs is not None and calibs.dim() == 3
                                                      and calibs.shape[0] != v_n):
            raise ValueError("bind_views: %d views, feature maps of batch %s, calibrations %s"
                             % (v_n, [f.shape[0] for f in feats_stages[-1]],
                                None if calibs is None else tuple(calibs.shape)))
        feats, calibs, projection, mlp = self._bind_common(feats_stages, calibs)
        if calibs.dim() == 2:  # one calibration (or none: the identity) for every view
            calibs = calibs[None].expand(v_n, *calibs.shape)
        maps = [self._packed_features(feats, v) for v in range(v_n)]
        return ViewsBinding(self, mlp, maps, calibs, self.normalizer.scale, projection)

    def get_loss(self, pred_stages, labels):
        """Average MSE / L1 over stages (MonoPortNet.py:93-117); plain tensor ops."""
        kind = self.opt.loss.IMF
        if kind not in ("MSE", "L1"):
            raise NotImplementedError(kind)
        fn = F.mse_loss if kind == "MSE" else F.l1_loss
        return sum(fn(p, labels) for p in pred_stages) / len(pred_stages)

    def forward(self, images, points, calibs, transforms=None, labels=None, feat_prior=None):
        feats_stages = self.filter(images, feat_prior)
        pred_stages = self.query(feats_stages, points, calibs, transforms)
        if labels is not None:
            return pred_stages[-1], self.get_loss(pred_stages, labels)
        return pred_stages[-1]

    def load_legacy_pifu(self, ckpt_path):
        """Flat legacy PIFu checkpoints: ``image_filter.*`` and ``surface_classifier.conv{i}.*``
        (renamed to ``filters.{i}.*``) -- MonoPortNet.py:153-160."""
        ckpt = torch.load(ckpt_path, map_location="cpu")
        self.image_filter.load_state_dict(
            {k.replace("image_filter.", ""): v for k, v in ckpt.items() if "image_filter" in k})
        self.surface_classifier.load_state_dict(
            {k.replace("surface_classifier.conv", "filters."): v
             for k, v in ckpt.items() if "surface_classifier" in k})


def _options(backbone, head, loss):
    opt = _AttrDict(projection="orthogonal")
    opt.backbone = _AttrDict(IMF=backbone)
    opt.normalizer = _AttrDict(IMF="PIFuNomalizer")
    opt.head = _AttrDict(IMF=head)
    opt.loss = _AttrDict(IMF=loss)
    return opt


def PIFuNetG():
    """netG: hourglass encoder + [257,1024,512,256,128,1] sigmoid head (MonoPortNet.py:163-184)."""
    return MonoPortNet(_options("PIFuHGFilters", "PIFuNetGMLP", "MSE"))


def PIFuNetC():
    """netC: ResNet encoder + [513,1024,512,256,128,3] tanh head (MonoPortNet.py:187-208)."""
    return MonoPortNet(_options("PIFuResBlkFilters", "PIFuNetCMLP", "L1"))
