"""``implicit_seg.functional``: the coarse-to-fine ("lossless octree") reconstruction engines.

``Seg3dLossless`` keeps the constructor and call surface the reference uses
(RTL/main.py:185-195, :392-394) but runs every level on the GPU: upsample + boundary ballot,
dilation + compaction, fused PIFu query with scatter (csrc/octree.hip, csrc/query.hip).

``Seg3dTopk`` is the fixed-budget engine with the same contract (its docstring; csrc/topk.hip).

PARITY NOTE: the upstream package is not vendored and not version-pinned by the reference, so the
algorithm here is our restatement of its published scheme; it is checked bit for
bit against the CPU restatement in oracle/pifu_oracle.py and against dense evaluation.

Constructor flags (upstream names):
  ``faster=True``   dilation boxes 9^3 / 7^3 / 3^3 by level, no conflict re-examination.  With a
                    ``query_func`` that is a plain MonoPortNet.query call (RTL/main.py:169-183) the
                    whole reconstruction is ONE asynchronous C-ABI call (fused path).
  ``faster=False``  3^3 boxes at every level plus the conflict re-examination loop (nodes whose
                    exact value contradicts the interpolated one get their 3x3x3 neighbourhood
                    evaluated, repeated until none is left); level-at-a-time engine, one host sync
                    per round as upstream.
  ``use_cuda_impl`` upstream switches the implementation of its interpolation, not its results:
                    accepted, both values run the same HIP kernels.
  ``debug``         accepted (upstream only prints timings).
  ``final_level``   (monoport_amd extension, faster=True only) the selection rule of the LAST level:
                    "dilate3" (default) -- the boundary nodes dilated by 3^3 like every level >= 3: the
                    lossless schedule, thresholded volume == thresholded dense evaluation on ordinary
                    bodies; "upstream" -- only nodes whose upsampled inside-mask is exactly 0.5
                    (``is_boundary = valid == 0.5``, no dilation), the rule we recall from the upstream
                    package's faster mode: ~4x fewer points at that level, ~0.4 % of the inside voxels
                    differ from dense evaluation; "interpolate" -- nothing is evaluated at the last
                    level (the other reading of upstream's "last step no examine").  Nothing under the
                    reference pins this; a maintainer who has implicit_seg
                    installed picks the mode that reproduces it.
  ``fuse_views``    (monoport_amd extension, faster=True only) serve a ``query_func`` whose one call is a
                    MULTI-VIEW MonoPortNet.query (SurfaceClassifier num_views = V > 1) through the fused
                    engine too (ops.recon_views: one asynchronous call, every level on the multi-view
                    kernel).  ``view`` (0..V-1) names the row of the [V,1,N] result the caller's
                    ``query_func`` returns: the view-averaged prediction times THAT view's in-image mask
                    (``[:1]`` of RTL/main.py's get_preds()[0][0] is view 0).  Off by default: a multi-view
                    ``query_func`` then runs on the level-at-a-time engine.  ``forward_many`` of a trusted engine
                    serves such frames through ops.recon_views_batch (all frames of a chunk per octree level).
  ``align_corners=True``, ``visualize=True``, ``use_shadow=True``, ``channels != 1``: not built,
                    NotImplementedError at construction.
"""
import threading
import warnings

import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ...modeling.MonoPortNet import record_query
from . import utils  # noqa: F401


class _Seg3dEngine(nn.Module):
    """What Seg3dLossless and Seg3dTopk share: the constructor checks of the upstream surface, and the contract
    around ``query_func`` -- the coarsest level always goes through it, the fused call serves the rest only if that
    was one plain MonoPortNet.query whose values the fused kernel reproduces, validated calls build trust
    (``validate="first"``), everything else runs level by level through ``query_func``.  A subclass says how a level
    is selected: ``_level_engine`` / ``_generic`` (level-at-a-time) and ``_recon`` / ``_recon_many`` (fused)."""

    faster = True       # the fused path is allowed
    fuse_views = False  # bind a multi-view query_func to the fused engine
    view = 0

    def _init_common(self, query_func, b_min, b_max, resolutions, channels, balance_value, align_corners, visualize,
                     debug, use_cuda_impl, use_shadow, validate, kwargs):
        name = type(self).__name__
        if kwargs:  # the upstream constructor swallows **kwargs: stay drop-in, but say so
            warnings.warn("%s: ignoring unknown arguments %s" % (name, sorted(kwargs)))
        self.query_func = query_func
        self.b_min = np.asarray(b_min, np.float32).reshape(-1, 3)
        self.b_max = np.asarray(b_max, np.float32).reshape(-1, 3)
        if self.b_min.shape[0] != 1:
            raise NotImplementedError("batch size 1 (the upstream engine asserts the same)")
        res = []
        for r in resolutions:
            r = np.asarray(r).reshape(-1)
            if r.size == 3 and not (r[0] == r[1] == r[2]):
                raise NotImplementedError("cubic resolutions only")
            res.append(int(r[0]))
        for r in res:
            if r % 2 != 1:
                raise AssertionError("resolution %d need to be odd because of align_corner" % r)
        for a, b in zip(res[:-1], res[1:]):
            if b != 2 * a - 1:
                raise NotImplementedError("resolutions must follow r -> 2r-1 (e.g. 17,33,65,129,257)")
        if channels != 1:
            raise NotImplementedError("one occupancy channel")
        if align_corners:
            raise NotImplementedError("align_corners=False lattice only (the reference's setting)")
        if visualize:
            raise NotImplementedError("visualize=True (upstream's interactive plots) is not built")
        if use_shadow:
            raise NotImplementedError("use_shadow=True is not built (the reference leaves it off)")
        self.resolutions = res
        self.channels = channels
        self.balance_value = float(balance_value)
        self.use_cuda_impl = bool(use_cuda_impl)  # same kernels either way (see module docstring)
        self.debug = bool(debug)
        self._status = None    # CPU tensor, or the device tensor of a call whose refinement may still be running
        self._early = threading.local()  # per host thread: the EarlyFlags buffers of its fused calls
        self.last_path = None  # "fused" | "generic": which engine served the last call
        # "always" (the default of the drop-in classes): every call evaluates the coarsest level through
        # query_func for real and compares it with the fused kernel -- a closure whose arithmetic changes
        # between frames (a flag, `1 - pred` from some frame on) is honoured on the frame it changes; costs
        # one 17^3 query and one host sync per frame (~0.3 ms).
        # "first": the first VALIDATE_CALLS calls are validated; once that many in a row agreed with the
        # fused kernel, later calls with the same network head are trusted and skip the validation query --
        # except every REVALIDATE_EVERY-th one.  For callers that vouch for their query_func
        # (stage_pipeline users that never rebind it).
        if validate not in ("always", "first"):
            raise ValueError("validate must be 'always' or 'first', got %r" % (validate,))
        self.validate = validate
        self._agreed = 0          # consecutive validated calls that agreed
        self._since_check = 0     # trusted calls since the last validated one
        # (id(packed head), precision, z scale, [views, view,] projection) those calls were bound to
        self._trusted_key = None
        # nn.Module.to(device) is called on the engine (RTL/main.py:195): carry a buffer so it
        # has a device like the upstream module does
        self.register_buffer("_device_tag", torch.zeros(1), persistent=False)

    # ---- what a subclass defines: how a level's nodes are selected ----
    def _level_engine(self, dev):
        """The level-at-a-time engine (ops.LevelEngine) of one call."""
        raise NotImplementedError

    def _generic(self, kwargs, dev, level0=None):
        """ops.recon_generic of one call -> (volume or None, per-level counts)."""
        raise NotImplementedError

    def _recon(self, b, early=None, expect_level0=None):
        """The fused reconstruction of a recorded binding -> (volume, status) on the device."""
        raise NotImplementedError

    def _recon_many(self, bindings, early):
        """The fused reconstruction of several single-view bindings in one call -> (volumes, status [n,1+levels])."""
        raise NotImplementedError

    def _recon_many_views(self, bindings):
        """The fused reconstruction of several multi-view bindings of one ``batch_key`` -> (volumes, status rows,
        early flags [n,2] on the host)."""
        raise NotImplementedError

    @property
    def last_status(self):
        """int32 [1 + levels] on the CPU: (coarsest level non-empty, points queried per level) of the last call.
        A fused call returns as soon as its coarsest level is known (mp_recon_batch_early): reading this waits
        for the call's stream to finish the remaining levels."""
        st = self._status
        if st is not None and st.is_cuda:
            st = self._status = st.cpu()
        return st

    @last_status.setter
    def last_status(self, value):
        self._status = value

    def _early_flags(self, dev, n=1):
        cache = self._early.__dict__.setdefault("flags", {})
        e = cache.get(n)
        if e is None:
            e = cache[n] = ops.EarlyFlags(dev, n)
        return e

    def forward(self, **kwargs):
        """engine(**kwargs) -> [1,1,R,R,R] f32 occupancy volume (z,y,x) or None when the coarsest
        level has nothing above ``balance_value`` (consumed at RTL/recon.py:32-35).

        The coarsest level (17^3 = 4913 points for the reference's settings) is ALWAYS evaluated
        through the caller's ``query_func``, for real.  If that call was exactly one
        MonoPortNet.query and ``faster`` is on, the fused engine runs the whole reconstruction and
        its coarsest level is compared with what ``query_func`` returned; only if they are
        identical is the fused volume returned.  Anything else -- another network, extra
        arithmetic around the call (1 - pred, scaled points, ...), several calls -- goes through
        the level-at-a-time engine, which evaluates every level with ``query_func`` itself.

        Limits of the check: only the coarsest lattice is compared, so a ``query_func`` that equals
        MonoPortNet.query there but post-processes finer levels differently (resolution-dependent
        logic) would pass; and after VALIDATE_CALLS agreeing calls in a row the check is skipped
        for later calls bound to the same head, except every REVALIDATE_EVERY-th one
        (``self.validate = "always"`` keeps it on for every call)."""
        dev = self._device_tag.device
        if (self.faster and self.validate != "always" and self._agreed >= self.VALIDATE_CALLS
                and self._since_check + 1 < self.REVALIDATE_EVERY):
            out = self._forward_trusted(kwargs)
            if out is not NotImplemented:
                self._since_check += 1
                return out
        self._since_check = 0
        eng = self._level_engine(dev)
        pts0 = eng.select()
        with record_query(views=self.fuse_views) as rec:
            occ0 = self.query_func(points=pts0[None], **kwargs)
        binding = rec.binding if rec.calls == 1 else None
        if binding is not None and self.faster:
            binding.check_view(self.view)
            eng.scatter(occ0)  # the caller's values on the coarsest lattice, [r0,r0,r0]
            early = self._early_flags(dev)
            volume, status = self._recon(binding, early, eng.cur)
            # the one host sync of a reconstruction (upstream syncs at every level) -- and it waits for the
            # coarsest level only: "None or a volume" and "is query_func the fused kernels' function" are both
            # known there, the finer levels go on refining `volume` on this stream after the call has returned
            nonempty, differs = (int(v) for v in early.wait()[0])
            if differs == 0:
                self.last_status, self.last_path = status, "fused"
                key = binding.trust_key(self.view)
                self._agreed = self._agreed + 1 if key == self._trusted_key else 1
                self._trusted_key = key
                return None if nonempty == 0 else volume[None, None]
            self._agreed, self._trusted_key = 0, None
            warnings.warn("%s: query_func is not a plain MonoPortNet.query call (its values differ from the fused "
                          "kernel's); using the level-at-a-time engine" % type(self).__name__)
            volume, counts = self._generic(kwargs, dev)
        else:
            volume, counts = self._generic(kwargs, dev, level0=(eng, occ0))
        self.last_path = "generic"
        self.last_status = torch.tensor([int(volume is not None)] + counts, dtype=torch.int32)
        return None if volume is None else volume[None, None]

    VALIDATE_CALLS = 3
    REVALIDATE_EVERY = 32  # a trusted query_func is validated again on every 32nd call

    def _forward_trusted(self, kwargs):
        """A query_func whose last VALIDATE_CALLS calls were plain MonoPortNet.query calls agreeing
        with the fused kernel: bind this frame's features / calibration through a one-point probe
        (recorded, not launched) and run the fused engine without the 17^3 validation query (one
        host sync instead of two).  NotImplemented = the binding changed: validate again."""
        probe = torch.zeros((1, 1, 3), dtype=torch.float32, device=self._device_tag.device)
        with record_query(capture_only=True, views=self.fuse_views) as rec:
            self.query_func(points=probe, **kwargs)
        b = rec.binding
        if b is None or rec.calls != 1 or b.trust_key(self.view) != self._trusted_key:
            self._agreed, self._trusted_key = 0, None
            return NotImplemented
        early = self._early_flags(self._device_tag.device)
        volume, status = self._recon(b, early)
        nonempty = int(early.wait()[0, 0])  # waits for the coarsest level only (see forward)
        self.last_status, self.last_path = status, "fused"
        return None if nonempty == 0 else volume[None, None]

    def forward_many(self, kwargs_list):
        """``[self(**kw) for kw in kwargs_list]`` for up to ops.MAX_FRAMES frames at once (monoport_amd extension;
        the hook of a coalescing recon stage, stage_pipeline.Coalesced).  When the engine is in its
        trusted state (see ``forward``) every frame is bound through its one-point probe and ALL of
        them go through one ``mp_recon_batch`` -- every octree level of all frames in one fused-query
        launch, one host sync for all statuses -- with results identical to the per-frame calls bit
        for bit.  With ``fuse_views`` the frames' multi-view bindings, if they share head, V, ``view``, projection
        and map size (``ViewsBinding.batch_key``), go through ``ops.recon_views_batch`` in chunks of
        ``ops.max_view_frames(V)`` frames, one early wait per chunk.  In any other state (not yet validated,
        ``validate = "always"``, a re-validation due, a binding that changed, bindings that do not batch together) the
        frames are served one by one by ``forward``."""
        n = len(kwargs_list)
        if n >= 2 and self.validate == "always" and not getattr(self, "_warned_many", False):
            self._warned_many = True
            warnings.warn("%s.forward_many on an engine with validate='always' (the class default) serves the frames "
                          "one by one; construct it with validate='first' to let a coalescing stage batch them"
                          % type(self).__name__)
        if (n < 2 or n > ops.MAX_FRAMES or not self.faster or self.validate == "always" or self._agreed < self.VALIDATE_CALLS
                or self._since_check + n >= self.REVALIDATE_EVERY):
            return [self(**kw) for kw in kwargs_list]
        probe = torch.zeros((1, 1, 3), dtype=torch.float32, device=self._device_tag.device)
        bindings = []
        for kw in kwargs_list:
            with record_query(capture_only=True, views=self.fuse_views) as rec:
                self.query_func(points=probe, **kw)
            b = rec.binding
            # single-view bindings share one ops.recon_batch call (``batchable``); multi-view bindings of one
            # ``batch_key`` share ops.recon_views_batch calls (``batch_many``); anything else goes frame by frame
            many = getattr(b, "batch_many", None)
            if (b is None or rec.calls != 1 or not (b.batchable or many is not None)
                    or b.trust_key(self.view) != self._trusted_key
                    or (many is not None and b.batch_key(self.view) != (bindings or [b])[0].batch_key(self.view))):
                return [self(**kw) for kw in kwargs_list]  # forward() re-validates
            bindings.append(b)
        if getattr(bindings[0], "batch_many", None) is not None:
            # one wait per chunk of ops.max_view_frames(V) frames, each for its coarsest level only
            volumes, status, flags = self._recon_many_views(bindings)
        else:
            early = self._early_flags(self._device_tag.device, n)
            volumes, status = self._recon_many(bindings, early)
            flags = early.wait().clone()  # the one host sync of the whole batch: its coarsest level (see forward)
        self._since_check += n
        self.last_status, self.last_path = status[-1], "fused"
        return [None if int(flags[i, 0]) == 0 else volumes[i][None, None] for i in range(n)]

    def forward_async(self, **kwargs):
        """Fused path only, no host sync and no validation of ``query_func`` (the caller vouches
        that it is a plain MonoPortNet.query call): (volume [R,R,R], status int32[1+levels]) on
        the device."""
        if not self.faster:
            raise NotImplementedError("forward_async is the faster=True schedule")
        probe = torch.zeros((1, 1, 3), dtype=torch.float32, device=self._device_tag.device)
        with record_query(capture_only=True, views=self.fuse_views) as rec:
            self.query_func(points=probe, **kwargs)
        b = rec.binding
        if b is None:
            raise NotImplementedError("forward_async needs a query_func ending in MonoPortNet.query")
        b.check_view(self.view)
        return self._recon(b)


class Seg3dLossless(_Seg3dEngine):
    def __init__(self, query_func, b_min, b_max, resolutions, channels=1, balance_value=0.5,
                 align_corners=False, visualize=False, debug=False, use_cuda_impl=False,
                 faster=False, use_shadow=False, final_level="dilate3", validate="always", fuse_views=False,
                 view=0, **kwargs):
        super().__init__()
        self._init_common(query_func, b_min, b_max, resolutions, channels, balance_value, align_corners, visualize,
                          debug, use_cuda_impl, use_shadow, validate, kwargs)
        self.faster = bool(faster)
        ops._final_level(final_level)  # ValueError for an unknown name
        if final_level != "dilate3" and not self.faster:
            raise NotImplementedError("final_level=%r is a variant of the faster=True schedule" % final_level)
        self.final_level = final_level
        if fuse_views and not self.faster:
            raise NotImplementedError("fuse_views=True is a variant of the faster=True schedule")
        if int(view) != view or view < 0:
            raise ValueError("view must be a row 0..V-1 of the multi-view result, got %r" % (view,))
        self.fuse_views = bool(fuse_views)
        self.view = int(view)

    def _level_engine(self, dev):
        return ops.LevelEngine(dev, self.b_min[0], self.b_max[0], self.resolutions,
                               self.balance_value, self.faster, self.final_level)

    def _generic(self, kwargs, dev, level0=None):
        return ops.recon_generic(self.query_func, kwargs, dev, self.b_min[0], self.b_max[0], self.resolutions,
                                 self.balance_value, self.faster, level0=level0, final_level=self.final_level)

    def _recon(self, b, early=None, expect_level0=None):
        """The fused reconstruction of a recorded binding: one frame (ops.recon) or, with ``fuse_views``, the V
        views of one subject (ops.recon_views, row ``self.view``) -> (volume, status) on the device."""
        return b.recon(self.b_min[0], self.b_max[0], self.resolutions, self.balance_value, self.final_level,
                       view=self.view, early=early, expect_level0=expect_level0)

    def _recon_many(self, bindings, early):
        b0 = bindings[0]
        return ops.recon_batch(b0.mlp, [b.feat_hwc for b in bindings], [b.calib for b in bindings],
                               b0.z_scale, self.b_min[0], self.b_max[0], self.resolutions,
                               self.balance_value, final_level=self.final_level, early=early,
                               projections=[b.projection for b in bindings])

    def _recon_many_views(self, bindings):
        dev = self._device_tag.device
        return type(bindings[0]).batch_many(bindings, self.b_min[0], self.b_max[0], self.resolutions,
                                            self.balance_value, self.final_level, view=self.view,
                                            early_flags=lambda n: self._early_flags(dev, n))


class Seg3dTopk(_Seg3dEngine):
    """The upstream package's fixed-budget engine (imported at RTL/main.py:28): level l >= 1 evaluates the
    ``num_points[l]`` most UNCERTAIN nodes -- those whose upsampled value is closest to ``balance_value`` -- instead of
    as many as the surface needs, so the cost of a frame is bounded and known in advance (entry 0 is ignored: the
    coarsest level is always evaluated whole).  The signature is recalled from upstream, which the reference neither
    vendors nor pins; the definition is ours (include/monoport_hip.h, restated in tests/topk_ref.py): ties go to the
    smaller linear index, the result is the same bits in every run.

    ``clip_mins``: upstream keeps the nodes with uncertainty = -|occ - balance| >= clip_mins[l]; here that is the bound
    |occ - balance| <= -clip_mins[l] on the candidates of level l (None, or None entries: no bound).
    ``use_cuda_impl`` and ``faster`` are accepted and select nothing: there is one implementation, the HIP kernels of
    csrc/topk.hip.  ``align_corners=True``, ``visualize=True``, ``use_shadow=True``, ``channels != 1`` and
    ``fuse_views`` are not built: NotImplementedError at construction.

    The contract around ``query_func`` is Seg3dLossless's: the coarsest level always goes through it; one plain
    MonoPortNet.query whose values the fused kernel reproduces is served by ONE asynchronous call
    (ops.recon_topk), anything else level by level through ``query_func`` (ops.recon_generic with ``num_points``);
    ``None`` for an empty coarsest level; ``last_status`` / ``last_path``, ``forward_many``, ``forward_async`` and
    ``validate="first"`` as there."""

    def __init__(self, query_func=None, b_min=None, b_max=None, resolutions=None, num_points=None, clip_mins=None,
                 channels=1, balance_value=0.5, align_corners=False, visualize=False, debug=False,
                 use_cuda_impl=False, faster=False, use_shadow=False, validate="always", **kwargs):
        super().__init__()
        # the five leading arguments are upstream's required ones; the name stayed constructible without them while it
        # was a stub that raised this error, and there is no engine to build from nothing
        missing = [n for n, v in (("query_func", query_func), ("b_min", b_min), ("b_max", b_max),
                                  ("resolutions", resolutions), ("num_points", num_points)) if v is None]
        if missing:
            raise NotImplementedError("Seg3dTopk needs %s" % ", ".join(missing))
        if kwargs.pop("fuse_views", False):
            raise NotImplementedError("fuse_views: the fixed-budget engine serves single-view heads only")
        self._init_common(query_func, b_min, b_max, resolutions, channels, balance_value, align_corners, visualize,
                          debug, use_cuda_impl, use_shadow, validate, kwargs)
        res = self.resolutions
        num_points = [int(k) for k in num_points]
        if len(num_points) != len(res):
            raise ValueError("Seg3dTopk: %d resolutions, %d budgets in num_points" % (len(res), len(num_points)))
        if any(k < 0 for k in num_points):
            raise ValueError("Seg3dTopk: num_points must not be negative, got %s" % (num_points,))
        for l, (k, r) in enumerate(zip(num_points, res)):
            if k > r ** 3:
                warnings.warn("Seg3dTopk: num_points[%d] = %d clamped to the level's %d^3 nodes" % (l, k, r))
                num_points[l] = r ** 3
        self.num_points = num_points
        self.max_dist = None
        if clip_mins is not None:
            if len(clip_mins) != len(res):
                raise ValueError("Seg3dTopk: %d resolutions, %d bounds in clip_mins" % (len(res), len(clip_mins)))
            self.max_dist = [float("inf") if c is None else -float(c) for c in clip_mins]
            if any(not d >= 0 for d in self.max_dist):
                raise ValueError("Seg3dTopk: clip_mins are bounds on -|occ - balance|: none may be positive or NaN")
        self.clip_mins = clip_mins

    def _level_engine(self, dev):
        return ops.LevelEngine(dev, self.b_min[0], self.b_max[0], self.resolutions, self.balance_value,
                               num_points=self.num_points, max_dist=self.max_dist)

    def _generic(self, kwargs, dev, level0=None):
        return ops.recon_generic(self.query_func, kwargs, dev, self.b_min[0], self.b_max[0], self.resolutions,
                                 self.balance_value, level0=level0, num_points=self.num_points,
                                 max_dist=self.max_dist)

    def _recon(self, b, early=None, expect_level0=None):
        return ops.recon_topk(b.mlp, b.feat_hwc, b.calib, b.z_scale, self.b_min[0], self.b_max[0], self.resolutions,
                              self.num_points, self.max_dist, self.balance_value, early=early,
                              expect_level0=expect_level0, projection=b.projection)

    def _recon_many(self, bindings, early):
        b0 = bindings[0]
        return ops.recon_topk_batch(b0.mlp, [b.feat_hwc for b in bindings], [b.calib for b in bindings], b0.z_scale,
                                    self.b_min[0], self.b_max[0], self.resolutions, self.num_points, self.max_dist,
                                    self.balance_value, early=early, projections=[b.projection for b in bindings])
