"""Tensor-level entry points over the C-ABI (torch is only the allocator / stream provider).

Every function here enqueues hand-written HIP kernels from libmonoport_hip.so on the caller's
current HIP stream and returns ordinary ``torch.Tensor`` objects that outlive the call -- the
ownership rule of the reference's stage pipeline (RTL/dataloader.py:1048-1054).
"""
import collections
import ctypes
import math
import os
import threading

import numpy as np
import torch

from . import _lib
from .synthetic import LAST_OP, MLP_DIMS  # noqa: F401  (re-exported for callers)

DIRECTIONS = {"front": 0, "back": 1, "left": 2, "right": 3}  # RTL/recon.py:39-49

_contexts = {}
_contexts_lock = threading.Lock()


class Context:
    """One mp_ctx (calls on it are serialised inside); ``get_context`` keeps two per HIP device, by role."""

    def __init__(self, device_index):
        self.lib = _lib.load()
        assert self.lib.mp_max_frames() == MAX_FRAMES, "_lib.MAX_FRAMES and the library's kMaxFrames disagree"
        assert self.lib.mp_max_frame_views() == MAX_FRAME_VIEWS, "_lib.MAX_FRAME_VIEWS and MP_MAX_FRAME_VIEWS disagree"
        self.device_index = int(device_index)
        handle = ctypes.c_void_p()
        rc = self.lib.mp_create(self.device_index, ctypes.byref(handle))
        if rc != 0:
            msg = self.lib.mp_last_error(None)
            raise _lib.MonoportError("mp_create(%d) failed (%d): %s"
                                     % (device_index, rc, msg.decode() if msg else "?"))
        self.handle = handle

    def check(self, rc, what):
        _lib.check(self.handle, rc, what)


def get_context(device, role="query"):
    """Context for a torch device (``cuda:N``).  Raises on CPU tensors: no CPU fallback.

    Two contexts per device (include/monoport_hip.h: "calls on ONE context are serialised by an internal mutex ...
    give each stage its own context"): ``role="query"`` owns the packed heads, the skip-table registry and the
    reconstruction / vertex / render calls; ``role="encoder"`` serves the stateless encoder launches (and the plans
    recorded from them).  The reference runs netG.filter and reconEngine on different host threads
    (RTL/dataloader.py:1026-1053): with one context the filter stage's 137 launches per frame and the recon stage's
    multi-launch mp_recon_batch_early would take turns on one mutex."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.MonoportError(
            "monoport_amd runs on MI355X only (got device %s); there is no CPU path" % device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = idx if role == "query" else (idx, role)
    with _contexts_lock:
        ctx = _contexts.get(key)
        if ctx is None:
            ctx = _contexts[key] = Context(idx)
    return ctx


def get_encoder_context(device):
    return get_context(device, "encoder")


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _f32c(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


# ---- argument checks and marshalling shared by the wrappers below (no context needed: CPU tensors pass them too) ----
MAX_FRAMES = _lib.MAX_FRAMES  # kMaxFrames: frames per mp_recon_batch / mp_query_batch / mp_query_counted_batch call
MAX_VIEWS = _lib.MAX_VIEWS  # MP_MAX_VIEWS
MAX_FRAME_VIEWS = _lib.MAX_FRAME_VIEWS  # MP_MAX_FRAME_VIEWS: frames x views per mp_recon_views_batch call


def _float3(v):
    """Three numbers (sequence, array, tensor) -> the float[3] the C side reads."""
    return (ctypes.c_float * 3)(*[float(x) for x in np.asarray(v, np.float32).reshape(3)])


def _ptr_array(tensors):
    """The host array of device addresses a batched entry point takes: one per tensor (of a tensor: per row), NULL
    for None."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _cubic_volume(t, who):
    """[...,R,R,R] with leading dimensions of size 1 (the engines return [1,1,R,R,R]) -> contiguous f32 [R,R,R]."""
    while t.dim() > 3:
        t = t[0]
    if t.dim() != 3 or t.shape[0] != t.shape[1] or t.shape[1] != t.shape[2]:
        raise ValueError("%s wants a cubic volume, got %s" % (who, tuple(t.shape)))
    return _f32c(t)


def _check_count(who, what, n, most):
    if not 1 <= n <= most:
        raise ValueError("%s: 1..%d %s per call, got %d" % (who, most, what, n))


def _calib_list(calibs, n, who):
    """n calibrations given as a sequence or as one [n,>=3,4] tensor -> the list of them."""
    if torch.is_tensor(calibs) and calibs.dim() == 3:
        calibs = list(calibs)
    if len(calibs) != n:
        raise ValueError("%s: %d maps, %d calibrations" % (who, n, len(calibs)))
    return calibs


def _maps(who, maps):
    """Channels-last maps of one call -> (h, w, c, device); all contiguous float32 [h,w,c]."""
    if len(maps) == 0 or maps[0].dim() != 3:
        raise ValueError("%s: wants a non-empty list of [H,W,C] maps" % who)
    h, w, c = maps[0].shape
    for f in maps:
        if tuple(f.shape) != (h, w, c) or not f.is_contiguous() or f.dtype != torch.float32:
            raise ValueError("%s: the maps must be contiguous float32 [%d,%d,%d]" % (who, h, w, c))
    return h, w, c, maps[0].device


def _out_rows(who, out, n, cout, npts):
    """A caller's result buffer of a batched query: float32 [n,cout,npts] whose rows are each contiguous."""
    if (tuple(out.shape) != (n, cout, npts) or out.dtype != torch.float32
            or (npts > 0 and not all(o.is_contiguous() for o in out))):
        raise ValueError("%s: out must be float32 [%d,%d,%d] with contiguous rows" % (who, n, cout, npts))


def _early_arg(who, early, n, expect, r0):
    """``early`` (EarlyFlags or None) + ``expect`` (n level-0 volumes [r0,r0,r0] f32, None entries allowed; or None)
    -> the mp_recon_early* argument.  ``early`` keeps the pointer array alive, the argument the struct."""
    if early is None:
        return None
    if early.n != n:
        raise ValueError("%s: EarlyFlags for %d frames, the call has %d" % (who, early.n, n))
    if expect is not None:
        if len(expect) != n:
            raise ValueError("%s: %d frames, %d expected level-0 volumes" % (who, n, len(expect)))
        for e in expect:
            if e is not None and (e.numel() != r0 ** 3 or not e.is_contiguous() or e.dtype != torch.float32):
                raise ValueError("%s: expect_level0 must be contiguous float32 [%d,%d,%d]" % (who, r0, r0, r0))
    return ctypes.byref(early.struct(expect))


def _frame_chunks(n):
    """The slices (f0, f1) of at most MAX_FRAMES frames in which a batched entry point takes n frames."""
    for f0 in range(0, n, MAX_FRAMES):
        yield f0, min(f0 + MAX_FRAMES, n)


def _one_size_volumes(who, volumes):
    """The volumes of one mesh / render call (``_cubic_volume`` each; at least one, of one size, on one device) ->
    (vols, n, r, device)."""
    vols = [_cubic_volume(v, who) for v in volumes]
    if not vols:
        raise ValueError("%s wants at least one volume" % who)
    r, dev = vols[0].shape[0], vols[0].device
    if any(v.shape[0] != r or v.device != dev for v in vols):
        raise ValueError("%s wants cubic volumes of one size on one device" % who)
    return vols, len(vols), r, dev


def _gates(who, gates, n, device):
    """Checks the per-frame gates of a call: None, or n device int32 tensors (None entries = frame on)."""
    if gates is not None:
        if len(gates) != n:
            raise ValueError("%s: %d volumes, %d gates" % (who, n, len(gates)))
        if any(g is not None and (g.dtype != torch.int32 or g.numel() < 1 or g.device != device) for g in gates):
            raise ValueError("%s: a gate is an int32 tensor on the volumes' device" % who)


def _keep_until_done(device, *tensor_lists):
    """The call just enqueued reads these tensors on ``device``'s current stream: the allocator must not hand their
    memory to another stream before it has."""
    stream = torch.cuda.current_stream(device)
    for tensors in tensor_lists:
        for t in tensors or ():
            if t is not None:
                t.record_stream(stream)


# mp_mlp_set_precision codes (include/monoport_hip.h)
PRECISIONS = {"f32": 0, "f16x3": 1, "f16w": 2, "f16": 3}


class PackedMLP:
    """Device-resident SurfaceClassifier weights in MFMA fragment order."""

    def __init__(self, ctx, channels, last_op):
        self.ctx = ctx
        self.channels = [int(c) for c in channels]
        self.last_op = int(last_op)
        n = len(self.channels) - 1
        arr = (ctypes.c_int * (n + 1))(*self.channels)
        mid = ctypes.c_int(-1)
        ctx.check(ctx.lib.mp_mlp_create(ctx.handle, n, arr, self.last_op, ctypes.byref(mid)),
                  "mp_mlp_create")
        self.id = mid.value
        self.c = self.channels[0] - 1
        self.cout = self.channels[-1]
        self.precision = "f32"
        self.generation = 0  # bumped by every load_layer: skip tables made before it are stale

    def load_layer(self, layer, weight, bias):
        """weight [out,in] or [out,in,1] (Conv1d k=1), bias [out]; device tensors.  The C side
        forgets the skip tables made with this head (they hold products of the old weights)."""
        w = _f32c(weight.reshape(weight.shape[0], -1))
        b = _f32c(bias)
        self.generation += 1
        self.ctx.check(self.ctx.lib.mp_mlp_load(self.ctx.handle, self.id, layer, _ptr(w), _ptr(b),
                                                w.shape[0], w.shape[1], _stream(w)), "mp_mlp_load")
        # the pack kernels read w/b asynchronously: keep them alive until the stream drains
        w.record_stream(torch.cuda.current_stream(w.device))
        b.record_stream(torch.cuda.current_stream(b.device))

    def set_precision(self, precision):
        """"f32" (default: exact f32 MFMA), "f16x3" (f32 emulated with three f16 MFMAs per
        product), "f16w" (fp16 weights, split activations) or "f16" (fp16 operands); the f16
        variants are netG heads (C = 256) only.  Call after the layers are loaded."""
        code = PRECISIONS[precision]
        self.ctx.check(self.ctx.lib.mp_mlp_set_precision(self.ctx.handle, self.id, code),
                       "mp_mlp_set_precision")
        self.precision = precision

    @classmethod
    def from_layers(cls, device, layers, last_op):
        """layers = [(W[out,in], b[out])] as numpy arrays or tensors (tests / bench fixtures)."""
        ctx = get_context(device)
        ws = [torch.as_tensor(np.asarray(w) if not torch.is_tensor(w) else w) for w, _ in layers]
        dims = [ws[0].shape[1]] + [w.shape[0] for w in ws]
        mlp = cls(ctx, dims, last_op)
        for i, (w, b) in enumerate(layers):
            mlp.load_layer(i, torch.as_tensor(w).to(device), torch.as_tensor(b).to(device))
        return mlp

    def __del__(self):
        try:
            self.ctx.lib.mp_mlp_destroy(self.ctx.handle, self.id)
        except Exception:
            pass


def pack_features(feats, out=None):
    """[1,Ci,H,W] NCHW maps -> one channels-last [H,W,sum Ci] map (concat order = list order,
    i.e. MonoPortNet.py:44's cat([feat_prior, feat]) when given [prior, feat])."""
    if torch.is_tensor(feats):
        feats = [feats]
    f0 = feats[0]
    ctx = get_context(f0.device)
    h, w = f0.shape[-2], f0.shape[-1]
    total = 0
    for f in feats:
        if f.dim() != 4 or f.shape[0] != 1 or f.shape[-2:] != (h, w):
            raise ValueError("pack_features wants [1,C,H,W] maps of one size, got %s"
                             % (tuple(f.shape),))
        total += f.shape[1]
    if out is None:
        out = torch.empty((h, w, total), dtype=torch.float32, device=f0.device)
    off = 0
    for f in feats:
        fc = _f32c(f)
        ctx.check(ctx.lib.mp_feat_pack_hwc(ctx.handle, _ptr(fc), fc.shape[1], h, w, _ptr(out),
                                           total, off, _stream(out)), "mp_feat_pack_hwc")
        off += fc.shape[1]
    return out


def _calib_dev(calib, device):
    """[B,>=3,4] or [>=3,4] calibration -> contiguous f32 [rows,4] on device (rows 0-2 are read)."""
    c = calib[0] if calib.dim() == 3 else calib
    if c.shape[-1] != 4 or c.shape[0] < 3:
        raise ValueError("calibration must be [>=3,4], got %s" % (tuple(c.shape),))
    return _f32c(c.to(device))


def index(feat_hwc, uv):
    """geometry.py:4-16 on a channels-last map: uv [1,2,N] or [2,N] -> [1,C,N]."""
    ctx = get_context(feat_hwc.device)
    h, w, c = feat_hwc.shape
    u = _f32c(uv.reshape(2, -1))
    n = u.shape[1]
    out = torch.empty((1, c, n), dtype=torch.float32, device=feat_hwc.device)
    ctx.check(ctx.lib.mp_index(ctx.handle, _ptr(feat_hwc), c, h, w, _ptr(u), n, _ptr(out),
                               _stream(out)), "mp_index")
    return out


PROJECTIONS = {"orthogonal": _lib.PROJ_ORTHOGONAL, "perspective": _lib.PROJ_PERSPECTIVE}  # MP_PROJ_*


def _projection(p):
    """A projection given as MP_PROJ_* int or as its name -> the int."""
    if isinstance(p, str):
        try:
            return PROJECTIONS[p]
        except KeyError:
            raise ValueError("projection must be one of %s, got %r" % (sorted(PROJECTIONS), p)) from None
    p = int(p)
    if p not in PROJECTIONS.values():
        raise ValueError("unknown projection mode %d" % p)
    return p


def orthogonal(points, calib):
    """geometry.py:19-34 (transforms=None): points [1,3,N] -> [1,3,N]."""
    ctx = get_context(points.device)
    p = _f32c(points.reshape(3, -1))
    n = p.shape[1]
    cal = _calib_dev(calib, points.device)
    out = torch.empty((1, 3, n), dtype=torch.float32, device=points.device)
    ctx.check(ctx.lib.mp_orthogonal(ctx.handle, _ptr(p), n, _ptr(cal), _ptr(out), _stream(out)),
              "mp_orthogonal")
    return out


def perspective(points, calib):
    """geometry.py:37-55 (transforms=None): points [1,3,N] -> [1,3,N] = (u/z, v/z, z) of (u, v, z) = R p + t
    (+-inf / NaN where z == 0, as the reference)."""
    ctx = get_context(points.device)
    p = _f32c(points.reshape(3, -1))
    n = p.shape[1]
    cal = _calib_dev(calib, points.device)
    out = torch.empty((1, 3, n), dtype=torch.float32, device=points.device)
    ctx.check(ctx.lib.mp_perspective(ctx.handle, _ptr(p), n, _ptr(cal), _ptr(out), _stream(out)),
              "mp_perspective")
    return out


# Skip tables (mp_skip_table): the products of the MLP's weights with the sampled feature (layer 0
# and the skip connections, 42 % of a point's FLOPs) are taken once per texel of a frame's feature
# map instead of once per query point -- 16 GFLOP + 126 MB per frame; the field differs from the
# plain path by f32 rounding only (1-3e-7).  This flag is the default of the callers that make tables
# on their own (pipeline.FrameSlot, MonoPortNet.bind); MONOPORT_SKIP_TABLE=off keeps the plain path.
SKIP_TABLE = os.environ.get("MONOPORT_SKIP_TABLE", "on") != "off"
# MonoPortNet.bind makes a table for a map once it has served this many query points (or at once for
# the octree engine): the table costs what ~16 k points cost on the plain kernels
SKIP_TABLE_MIN_POINTS = int(os.environ.get("MONOPORT_SKIP_TABLE_MIN_POINTS", "16384"))
def table_precision(precision):
    """Whether the fused query of a netG head with this MLP precision blends table rows (mirrors
    launch_query16 in csrc/query16.hip: f16x3 by default, every f16 variant with MONOPORT_TAB16=all, none
    with =off; the exact-f32 kernels always do).  Callers that build tables on their own check it first: a
    table nobody reads costs 16 GFLOP and 128 MB per frame."""
    if precision == "f32":
        return True
    t16 = os.environ.get("MONOPORT_TAB16", "")
    if t16.startswith("a"):
        return True
    if t16.startswith("o"):
        return False
    return precision == "f16x3"


SKIP_TABLE_ROWS = 1952  # kTableRows: the feature segments of layers 0-3 (1024 + 512 + 256 + 128) + the last layer's, padded to 61 cache lines


class SkipTable:
    """A registered skip table: holds the feature map(s) and the table alive and unregisters them
    when released or garbage-collected -- a freed map's address may be handed to the next map, and a
    stale registration would then route that map's queries through this table.  A handle only
    unregisters what is still ITS registration: making a new table for the same map (same buffers,
    next frame) supersedes the old handle."""

    _latest = {}  # (context handle, feature-map address) -> id of the handle that registered it last
    # re-entrant: __del__ -> release() may run from the cyclic GC while this thread holds the lock
    _lock = threading.RLock()

    def __init__(self, ctx, feats, table):
        self.ctx, self.feats, self.table = ctx, list(feats), table
        self._tables = [table[i] for i in range(len(self.feats))] if table.dim() == 4 else [table]
        with SkipTable._lock:
            for f in self.feats:
                SkipTable._latest[(ctx.handle.value if hasattr(ctx.handle, "value") else ctx.handle, f.data_ptr())] = id(self)

    def release(self):
        with SkipTable._lock:
            for f, t in zip(self.feats, self._tables):
                key = (self.ctx.handle.value if hasattr(self.ctx.handle, "value") else self.ctx.handle, f.data_ptr())
                if SkipTable._latest.get(key) == id(self):
                    del SkipTable._latest[key]
                    self.ctx.lib.mp_skip_table_release(self.ctx.handle, _ptr(f), _ptr(t))
            self.feats, self._tables = [], []

    def __del__(self):
        try:
            self.release()
        except Exception:  # interpreter shutdown
            pass


def skip_table(mlp, feat_hwc, out=None):
    """mp_skip_table: the skip table of a channels-last feature map [H,W,256] for a netG head --
    table[y,x,:] = the products of every layer's feature-segment weights with feat[y,x,:]
    (SurfaceClassifier's layer 0 and the skip connections of layers 1-4: 1921 rows) -- computed
    once per map and REGISTERED for it: every later fused query (query / recon / recon_batch ...)
    on maps that all have a table blends four table rows per point instead of multiplying those
    weights with the sampled feature on the MFMAs (42 % of a point's FLOPs).  The result differs
    from the plain path by f32 rounding only.  Returns a SkipTable handle (``.table`` is the
    [H,W,1952] tensor); the registration lasts until ``.release()`` or the handle's collection.
    Call again after rewriting the feature map."""
    ctx = mlp.ctx
    h, w, c = feat_hwc.shape
    if out is None:
        out = torch.empty((h, w, SKIP_TABLE_ROWS), dtype=torch.float32, device=feat_hwc.device)
    elif tuple(out.shape) != (h, w, SKIP_TABLE_ROWS) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("skip_table: out must be a contiguous float32 [%d,%d,%d]" % (h, w, SKIP_TABLE_ROWS))
    ctx.check(ctx.lib.mp_skip_table(ctx.handle, mlp.id, _ptr(feat_hwc), c, h, w, _ptr(out), _stream(out)),
              "mp_skip_table")
    return SkipTable(ctx, [feat_hwc], out)


def skip_table_batch(mlp, feat_hwc_all, out=None):
    """mp_skip_table_batch: the tables of B maps stored back to back [B,H,W,256] -> [B,H,W,1952] in
    one launch; each map feat_hwc_all[i] is registered with its table out[i].  Returns a SkipTable
    handle for all of them."""
    ctx = mlp.ctx
    b, h, w, c = feat_hwc_all.shape
    if not feat_hwc_all.is_contiguous():
        raise ValueError("skip_table_batch: the maps must be contiguous")
    if out is None:
        out = torch.empty((b, h, w, SKIP_TABLE_ROWS), dtype=torch.float32, device=feat_hwc_all.device)
    elif tuple(out.shape) != (b, h, w, SKIP_TABLE_ROWS) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("skip_table_batch: out must be a contiguous float32 [%d,%d,%d,%d]"
                         % (b, h, w, SKIP_TABLE_ROWS))
    ctx.check(ctx.lib.mp_skip_table_batch(ctx.handle, mlp.id, b, _ptr(feat_hwc_all), c, h, w, _ptr(out),
                                          _stream(out)), "mp_skip_table_batch")
    return SkipTable(ctx, [feat_hwc_all[i] for i in range(b)], out)


def skip_table_release(ctx, feat_hwc=None):
    """Forget the table registered for feat_hwc (None: every table of the context), whichever handle
    made it."""
    with SkipTable._lock:
        h = ctx.handle.value if hasattr(ctx.handle, "value") else ctx.handle
        for key in [k for k in SkipTable._latest if k[0] == h and (feat_hwc is None or k[1] == feat_hwc.data_ptr())]:
            del SkipTable._latest[key]
    ctx.check(ctx.lib.mp_skip_table_release(ctx.handle, _ptr(feat_hwc) if feat_hwc is not None else None, None),
              "mp_skip_table_release")


def query(mlp, feat_hwc, points, calib, z_scale, projection=_lib.PROJ_ORTHOGONAL):
    """MonoPortNet.query (eval, one stage).  points [1,3,N] with ANY strides (the permuted view
    query_func builds at RTL/main.py:176-177 is consumed in place) -> [1,Cout,N].  ``projection``:
    MP_PROJ_* int or "orthogonal" / "perspective" (a perspective query is a one-frame ``query_batch``)."""
    ctx = mlp.ctx
    if points.dim() != 3 or points.shape[0] != 1 or points.shape[1] != 3:
        raise ValueError("points must be [1,3,N], got %s" % (tuple(points.shape),))
    projection = _projection(projection)
    if projection != _lib.PROJ_ORTHOGONAL:
        return query_batch(mlp, [feat_hwc], points, [calib], [projection], z_scale)
    if points.dtype != torch.float32:
        points = points.float()
    h, w, c = feat_hwc.shape
    n = points.shape[2]
    cal = _calib_dev(calib, feat_hwc.device)
    out = torch.empty((1, mlp.cout, n), dtype=torch.float32, device=feat_hwc.device)
    ctx.check(ctx.lib.mp_query(ctx.handle, mlp.id, _ptr(feat_hwc), c, h, w, _ptr(points), n,
                               points.stride(2), points.stride(1), _ptr(cal), float(z_scale),
                               _ptr(out), _stream(out)), "mp_query")
    return out


def _query_rows(who, entry, mlp, maps, points, calibs, projection, z_scale, out):
    """mp_query_batch / mp_query_views (``entry``; one signature but for the projection argument, marshalled by the
    caller): row i = map i, points[i] (any strides), calibration i -> out[i]."""
    ctx = mlp.ctx
    n = len(maps)
    if points.dim() != 3 or points.shape[0] != n or points.shape[1] != 3:
        raise ValueError("%s: points must be [%d,3,N], got %s" % (who, n, tuple(points.shape)))
    if points.dtype != torch.float32:
        points = points.float()
    h, w, c, dev = _maps(who, maps)
    cals = [_calib_dev(cb, dev) for cb in _calib_list(calibs, n, who)]
    npts = points.shape[2]
    if out is None:
        out = torch.empty((n, mlp.cout, npts), dtype=torch.float32, device=dev)
    else:
        _out_rows(who, out, n, mlp.cout, npts)
    ctx.check(getattr(ctx.lib, entry)(
        ctx.handle, mlp.id, n, _ptr_array(maps), c, h, w, _ptr_array(points), npts, points.stride(2), points.stride(1),
        _ptr_array(cals), projection, float(z_scale), _ptr_array(out), _stream(out)), entry)
    _keep_until_done(dev, cals)
    return out


def query_batch(mlp, feats_hwc, points, calibs, projections, z_scale, out=None):
    """mp_query_batch: MonoPortNet.query for F <= MAX_FRAMES frames in one launch.  feats_hwc: F channels-last
    maps [H,W,C]; points [F,3,N] with ANY strides; calibs: F calibrations ([>=3,4] or [1,>=3,4] each, or one
    [F,>=3,4] tensor); projections: F MP_PROJ_* ints or names.  -> [F,Cout,N] (or into ``out``, whose frames
    must each be contiguous [Cout,N])."""
    n = len(feats_hwc)
    _check_count("query_batch", "frames", n, MAX_FRAMES)
    if len(projections) != n:
        raise ValueError("query_batch: %d maps, %d projections" % (n, len(projections)))
    proj = (ctypes.c_int * n)(*[_projection(p) for p in projections])
    return _query_rows("query_batch", "mp_query_batch", mlp, feats_hwc, points, calibs, proj, z_scale, out)


def mlp_forward(mlp, feature):
    """SurfaceClassifier.forward: feature [1,C+1,N] -> [1,Cout,N] (mp_mlp_forward)."""
    ctx = mlp.ctx
    if feature.dim() != 3 or feature.shape[0] != 1 or feature.shape[1] != mlp.c + 1:
        raise ValueError("feature must be [1,%d,N], got %s" % (mlp.c + 1, tuple(feature.shape)))
    f = _f32c(feature)
    n = f.shape[2]
    out = torch.empty((1, mlp.cout, n), dtype=torch.float32, device=f.device)
    ctx.check(ctx.lib.mp_mlp_forward(ctx.handle, mlp.id, _ptr(f), n, _ptr(out), _stream(f)),
              "mp_mlp_forward")
    return out


def query_views(mlp, feats_hwc, points, calibs, projection, z_scale, out=None):
    """mp_query_views: MonoPortNet.query of a multi-view head (SurfaceClassifier num_views = V, multi-view PIFu).
    feats_hwc: V channels-last maps [H,W,C]; points [V,3,N] with ANY strides (row v = the points as view v's
    caller passes them); calibs: V calibrations ([>=3,4] each, or one [V,>=3,4] tensor); projection: ONE MP_PROJ_*
    int or name for all views.  -> [V,Cout,N] (or into ``out``, whose views must each be contiguous [Cout,N]):
    row v is the view-averaged prediction times view v's in-image mask.  f32 heads only; registered skip tables
    are not used."""
    _check_count("query_views", "views", len(feats_hwc), MAX_VIEWS)
    return _query_rows("query_views", "mp_query_views", mlp, feats_hwc, points, calibs, _projection(projection),
                       z_scale, out)


def mlp_forward_views(mlp, feature):
    """SurfaceClassifier.forward of a multi-view head on ONE point set: feature [V,C+1,N] (the V views' rows,
    SurfaceClassifier.py:60-66) -> [1,Cout,N] (mp_mlp_forward_views)."""
    ctx = mlp.ctx
    if feature.dim() != 3 or feature.shape[1] != mlp.c + 1:
        raise ValueError("feature must be [V,%d,N], got %s" % (mlp.c + 1, tuple(feature.shape)))
    v_n = feature.shape[0]
    _check_count("mlp_forward_views", "views", v_n, MAX_VIEWS)
    f = _f32c(feature)
    n = f.shape[2]
    out = torch.empty((1, mlp.cout, n), dtype=torch.float32, device=f.device)
    ctx.check(ctx.lib.mp_mlp_forward_views(ctx.handle, mlp.id, v_n, _ptr(f), n, _ptr(out), _stream(f)),
              "mp_mlp_forward_views")
    return out


def query_counted(mlp, feat_hwc, points, count, calib, z_scale, out=None):
    """mp_query_counted: points [3,cap] contiguous, count int32[1] on device -> [Cout,cap]."""
    ctx = mlp.ctx
    h, w, c = feat_hwc.shape
    cap = points.shape[1]
    cal = _calib_dev(calib, feat_hwc.device)
    if out is None:
        out = torch.zeros((mlp.cout, cap), dtype=torch.float32, device=feat_hwc.device)
    ctx.check(ctx.lib.mp_query_counted(ctx.handle, mlp.id, _ptr(feat_hwc), c, h, w, _ptr(points),
                                       cap, _ptr(count), _ptr(cal), float(z_scale), _ptr(out),
                                       _stream(out)), "mp_query_counted")
    return out


def query_counted_batch(mlp, feats_hwc, points, counts, calibs, z_scale, outs=None, projections=None):
    """mp_query_counted_batch_proj: one fused-query launch for up to MAX_FRAMES frames.  feats_hwc / points
    ([3,cap] each, one cap) / counts (int32[1] each) / calibs: lists of per-frame device tensors
    -> list of [Cout,cap].  ``projections``: per-frame MP_PROJ_* ints or names (None: all orthogonal, which is
    mp_query_counted_batch)."""
    who = "query_counted_batch"
    ctx = mlp.ctx
    n = len(feats_hwc)
    h, w, c, dev = _maps(who, feats_hwc)
    if len(points) != n or len(counts) != n or (projections is not None and len(projections) != n):
        raise ValueError("%s: %d maps, %d point sets, %d counts, %s projections"
                         % (who, n, len(points), len(counts), None if projections is None else len(projections)))
    cap = points[0].shape[-1]
    if any(tuple(p.shape) != (3, cap) or not p.is_contiguous() or p.dtype != torch.float32 for p in points):
        raise ValueError("%s: the point sets must be contiguous float32 [3,%d]" % (who, cap))
    cals = [_calib_dev(cb, dev) for cb in _calib_list(calibs, n, who)]
    if outs is None:
        outs = [torch.zeros((mlp.cout, cap), dtype=torch.float32, device=dev) for _ in range(n)]
    elif len(outs) != n:
        raise ValueError("%s: %d maps, %d outputs" % (who, n, len(outs)))
    proj = None if projections is None else (ctypes.c_int * n)(*[_projection(p) for p in projections])
    ctx.check(ctx.lib.mp_query_counted_batch_proj(
        ctx.handle, mlp.id, n, _ptr_array(feats_hwc), c, h, w, _ptr_array(points), cap, _ptr_array(counts),
        _ptr_array(cals), proj, float(z_scale), _ptr_array(outs), _stream(outs[0])), "mp_query_counted_batch_proj")
    _keep_until_done(dev, cals)
    return outs


# Selection rule of the LAST octree level (include/monoport_hip.h, MP_FINAL_*; Seg3dLossless docstring)
FINAL_LEVELS = {"dilate3": 0, "upstream": 1, "interpolate": 2}


class EarlyFlags:
    """Buffers of one mp_recon_batch_early hand-over for up to ``n`` frames: device flags, their pinned host copy
    and the event recorded behind the copy.  ``wait()`` blocks until the coarsest octree level of the call is
    done (~0.1 ms of GPU time into it) and returns [n,2] int32: (level 0 non-empty, level-0 values differ from the
    expected ones).  One object serves one call at a time (reuse it after ``wait``)."""

    def __init__(self, device, n=1):
        self.n = int(n)
        self.dev = torch.zeros(2 * self.n, dtype=torch.int32, device=device)
        self.host = torch.zeros(2 * self.n, dtype=torch.int32).pin_memory()
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(device))  # materialises the hipEvent_t the C side re-records

    def struct(self, expect):
        self._expect = None
        if expect is not None:  # the C side reads self.n entries
            self._expect = _ptr_array(list(expect) + [None] * (self.n - len(expect)))
        return _lib.ReconEarly(ctypes.cast(self._expect, ctypes.c_void_p) if self._expect is not None else None,
                               self.dev.data_ptr(), self.host.data_ptr(), self.event.cuda_event)

    def wait(self):
        self.event.synchronize()
        return self.host.view(self.n, 2)


def _final_level(final_level):
    try:
        return FINAL_LEVELS[final_level]
    except KeyError:
        raise ValueError("final_level must be one of %s, got %r" % (sorted(FINAL_LEVELS), final_level)) from None


def recon(mlp, feat_hwc, calib, z_scale, b_min, b_max, resolutions, balance=0.5, volume=None,
          status=None, final_level="dilate3", early=None, expect_level0=None, projection=_lib.PROJ_ORTHOGONAL):
    """Coarse-to-fine occupancy volume (Seg3dLossless replacement).  Returns (volume [R,R,R]
    f32, status int32[1+levels]) -- both on device, nothing synchronised.  ``early`` / ``expect_level0`` /
    ``projection``: see ``recon_batch``."""
    st = None if status is None else status.reshape(1, -1)
    volumes, st = recon_batch(mlp, [feat_hwc], [calib], z_scale, b_min, b_max, resolutions, balance,
                              None if volume is None else [volume], st, final_level, early,
                              None if expect_level0 is None else [expect_level0],
                              None if _projection(projection) == _lib.PROJ_ORTHOGONAL else [projection])
    return volumes[0], st[0]


def recon_batch(mlp, feats_hwc, calibs, z_scale, b_min, b_max, resolutions, balance=0.5,
                volumes=None, status=None, final_level="dilate3", early=None, expect_level0=None, projections=None):
    """``recon`` over up to MAX_FRAMES independent frames in one call: every octree level evaluates the
    selected nodes of all frames in ONE fused-query launch (the coarse levels of a single frame
    cannot fill 256 CUs).  feats_hwc: list of [H,W,C] maps; calibs: [B,4,4] (or list of [1,4,4]);
    volumes: list of [R,R,R]; status: [B, 1+levels] int32.  Results equal B separate ``recon``
    calls bit for bit.  ``early``: an ``EarlyFlags`` for B frames -- mp_recon_batch_early: after the coarsest level
    the call hands (non-empty, differs-from-``expect_level0[b]``) per frame to the host (``early.wait()``) and goes
    on refining; ``expect_level0``: list of [r0,r0,r0] f32 tensors (or None entries).  ``projections``: per-frame
    MP_PROJ_* ints or names (None: all orthogonal).  One mp_recon_batch_proj call, which with no projections is
    mp_recon_batch_early."""
    return _recon_frames("recon_batch", mlp, feats_hwc, calibs, z_scale, b_min, b_max, resolutions, balance, volumes,
                         status, early, expect_level0, projections, final_level=_final_level(final_level))


def _recon_frames(who, mlp, feats_hwc, calibs, z_scale, b_min, b_max, resolutions, balance, volumes, status, early,
                  expect_level0, projections, final_level=None, topk=None):
    """What ``recon_batch`` (``final_level``: the MP_FINAL_* rule, one mp_recon_batch_proj call) and
    ``recon_topk_batch`` (``topk`` = (num_points, max_dist), one mp_recon_topk_batch call) share: the frames'
    arguments checked and marshalled, buffers made where the caller gave none."""
    ctx = mlp.ctx
    n = len(feats_hwc)
    h, w, c, dev = _maps(who, feats_hwc)
    res = [int(r) for r in resolutions]
    cals = [_calib_dev(cb, dev) for cb in _calib_list(calibs, n, who)]
    if projections is not None and len(projections) != n:
        raise ValueError("%s: %d frames, %d projections" % (who, n, len(projections)))
    proj = None if projections is None else (ctypes.c_int * n)(*[_projection(p) for p in projections])
    if volumes is None:
        volumes = [torch.empty((res[-1],) * 3, dtype=torch.float32, device=dev) for _ in range(n)]
    elif len(volumes) != n:
        raise ValueError("%s: %d frames, %d volumes" % (who, n, len(volumes)))
    if status is None:
        status = torch.empty((n, 1 + len(res)), dtype=torch.int32, device=dev)
    elif tuple(status.shape) != (n, 1 + len(res)) or not status.is_contiguous() or status.dtype != torch.int32:
        raise ValueError("%s: status must be contiguous int32 [%d,%d]" % (who, n, 1 + len(res)))
    early_arg = _early_arg(who, early, n, expect_level0, res[0])
    res_arg = (ctypes.c_int * len(res))(*res)
    if topk is None:
        ctx.check(ctx.lib.mp_recon_batch_proj(
            ctx.handle, mlp.id, n, _ptr_array(feats_hwc), c, h, w, _ptr_array(cals), proj, float(z_scale),
            _float3(b_min), _float3(b_max), res_arg, len(res), float(balance), final_level,
            _ptr_array(volumes), _ptr_array(status), early_arg, _stream(volumes[0])), "mp_recon_batch_proj")
    else:
        num_points, max_dist = _topk_levels(who, res, *topk)
        ctx.check(ctx.lib.mp_recon_topk_batch(
            ctx.handle, mlp.id, n, _ptr_array(feats_hwc), c, h, w, _ptr_array(cals), proj, float(z_scale),
            _float3(b_min), _float3(b_max), res_arg, len(res), (ctypes.c_int64 * len(res))(*num_points),
            None if max_dist is None else (ctypes.c_float * len(res))(*max_dist), float(balance),
            _ptr_array(volumes), _ptr_array(status), early_arg, _stream(volumes[0])), "mp_recon_topk_batch")
    _keep_until_done(dev, cals, expect_level0)
    return volumes, status


def _topk_levels(who, res, num_points, max_dist):
    """Per-level budgets and bounds of the fixed-budget engine -> (ints, floats or None); None bounds mean +inf."""
    num_points = [int(k) for k in num_points]
    if len(num_points) != len(res):
        raise ValueError("%s: %d levels, %d budgets in num_points" % (who, len(res), len(num_points)))
    if max_dist is not None:
        max_dist = [float("inf") if d is None else float(d) for d in max_dist]
        if len(max_dist) != len(res):
            raise ValueError("%s: %d levels, %d bounds in max_dist" % (who, len(res), len(max_dist)))
    return num_points, max_dist


def recon_topk(mlp, feat_hwc, calib, z_scale, b_min, b_max, resolutions, num_points, max_dist=None, balance=0.5,
               volume=None, status=None, early=None, expect_level0=None, projection=_lib.PROJ_ORTHOGONAL):
    """``recon`` with a FIXED BUDGET per level (Seg3dTopk replacement): level l >= 1 evaluates the ``num_points[l]``
    nodes whose upsampled value is closest to ``balance`` (ties to the smaller linear index; entry 0 is ignored,
    level 0 evaluates every node), optionally only those within ``max_dist[l]`` of it -- the definition in
    include/monoport_hip.h, chosen on the device (csrc/topk.hip).  Returns (volume [R,R,R] f32, status
    int32[1+levels]) on the device, nothing synchronised; the other arguments as in ``recon``."""
    st = None if status is None else status.reshape(1, -1)
    volumes, st = recon_topk_batch(mlp, [feat_hwc], [calib], z_scale, b_min, b_max, resolutions, num_points, max_dist,
                                   balance, None if volume is None else [volume], st, early,
                                   None if expect_level0 is None else [expect_level0],
                                   None if _projection(projection) == _lib.PROJ_ORTHOGONAL else [projection])
    return volumes[0], st[0]


def recon_topk_batch(mlp, feats_hwc, calibs, z_scale, b_min, b_max, resolutions, num_points, max_dist=None,
                     balance=0.5, volumes=None, status=None, early=None, expect_level0=None, projections=None):
    """``recon_topk`` over up to MAX_FRAMES frames in one mp_recon_topk_batch call (one budget list for all frames):
    every level's nodes of all frames go through one fused-query launch sized by the budget.  Results equal the
    single-frame calls bit for bit; a frame with an empty coarsest level has status [0, r0^3, 0, ...].  Arguments as
    in ``recon_batch``."""
    return _recon_frames("recon_topk_batch", mlp, feats_hwc, calibs, z_scale, b_min, b_max, resolutions, balance,
                         volumes, status, early, expect_level0, projections, topk=(num_points, max_dist))


def recon_views(mlp, maps, calibs, projection, z_scale, b_min, b_max, resolutions, balance=0.5,
                final_level="dilate3", view=0, early=None, expect_level0=None):
    """mp_recon_views: ``recon`` for a multi-view head (SurfaceClassifier num_views = V).  maps: V channels-last
    maps [H,W,C]; calibs: V calibrations ([>=3,4] each, or one [V,>=3,4] tensor); projection: ONE MP_PROJ_* int or
    name for all views; ``view``: which row of the reference's [V,1,N] result the volume holds (the view-averaged
    prediction times view ``view``'s in-image mask).  Returns (volume [R,R,R] f32, status int32[1+levels]) -- both
    on device, nothing synchronised.  ``early``: an ``EarlyFlags`` for one frame, ``expect_level0``: [r0,r0,r0] f32
    (see ``recon_batch``).  f32 netG heads only; registered skip tables are not used."""
    who = "recon_views"
    ctx = mlp.ctx
    v_n = len(maps)
    _check_count(who, "views", v_n, MAX_VIEWS)
    h, w, c, dev = _maps(who, maps)
    cals = [_calib_dev(cb, dev) for cb in _calib_list(calibs, v_n, who)]
    res = [int(r) for r in resolutions]
    volume = torch.empty((res[-1],) * 3, dtype=torch.float32, device=dev)
    status = torch.empty((1 + len(res),), dtype=torch.int32, device=dev)
    expect = None if expect_level0 is None else [expect_level0]
    early_arg = _early_arg(who, early, 1, expect, res[0])
    ctx.check(ctx.lib.mp_recon_views(
        ctx.handle, mlp.id, v_n, _ptr_array(maps), c, h, w, _ptr_array(cals), _projection(projection), float(z_scale),
        _float3(b_min), _float3(b_max), (ctypes.c_int * len(res))(*res), len(res), float(balance),
        _final_level(final_level), int(view), _ptr(volume), _ptr(status), early_arg, _stream(volume)), "mp_recon_views")
    _keep_until_done(dev, cals, expect)
    return volume, status


def max_view_frames(n_views):
    """Frames of ``n_views`` views one ``recon_views_batch`` call accepts: callers chunk by it."""
    return min(MAX_FRAMES, MAX_FRAME_VIEWS // int(n_views))


def recon_views_batch(mlp, maps, calibs, projection, z_scale, b_min, b_max, resolutions, balance=0.5,
                      final_level="dilate3", view=0, volumes=None, status=None, early=None, expect_level0=None):
    """mp_recon_views_batch: ``recon_views`` over n independent frames of V views each in ONE call -- every octree
    level evaluates the selected nodes of all frames in one launch of the multi-view kernel.  maps: list of n lists of
    V channels-last maps [H,W,C]; calibs: [n,V,>=3,4] or n sequences of V calibrations; projection, ``view``: one for
    all frames; volumes: list of n [R,R,R] f32; status: [n, 1+levels] int32.  n <= ``max_view_frames(V)``.  Returns
    (volumes, status) on the device, nothing synchronised; frame f's equal ``recon_views`` on its maps and
    calibrations bit for bit.  ``early``: an ``EarlyFlags`` for n frames, ``expect_level0``: n [r0,r0,r0] f32 tensors
    (or None entries), as in ``recon_batch``."""
    who = "recon_views_batch"
    ctx = mlp.ctx
    n = len(maps)
    if n == 0 or len(calibs) != n:
        raise ValueError("%s: %d frames, %d sets of calibrations" % (who, n, len(calibs)))
    v_n = len(maps[0])
    _check_count(who, "views", v_n, MAX_VIEWS)
    if any(len(m) != v_n for m in maps):
        raise ValueError("%s: every frame needs the same number of views (%d)" % (who, v_n))
    _check_count(who, "frames of %d views" % v_n, n, max_view_frames(v_n))
    flat = [m for frame in maps for m in frame]
    h, w, c, dev = _maps(who, flat)
    cals = [_calib_dev(cb, dev) for frame in calibs for cb in _calib_list(frame, v_n, who)]
    res = [int(r) for r in resolutions]
    if volumes is None:
        volumes = [torch.empty((res[-1],) * 3, dtype=torch.float32, device=dev) for _ in range(n)]
    elif len(volumes) != n:
        raise ValueError("%s: %d frames, %d volumes" % (who, n, len(volumes)))
    if status is None:
        status = torch.empty((n, 1 + len(res)), dtype=torch.int32, device=dev)
    elif tuple(status.shape) != (n, 1 + len(res)) or not status.is_contiguous() or status.dtype != torch.int32:
        raise ValueError("%s: status must be contiguous int32 [%d,%d]" % (who, n, 1 + len(res)))
    early_arg = _early_arg(who, early, n, expect_level0, res[0])
    ctx.check(ctx.lib.mp_recon_views_batch(
        ctx.handle, mlp.id, n, v_n, _ptr_array(flat), c, h, w, _ptr_array(cals), _projection(projection),
        float(z_scale), _float3(b_min), _float3(b_max), (ctypes.c_int * len(res))(*res), len(res), float(balance),
        _final_level(final_level), int(view), _ptr_array(volumes), _ptr_array(status), early_arg,
        _stream(volumes[0])), "mp_recon_views_batch")
    _keep_until_done(dev, cals, expect_level0)
    return volumes, status


def query_views_counted_batch(mlp, maps, points, counts, calibs, projection, z_scale, view=0, outs=None):
    """mp_query_views_counted_batch: ``query_views`` over n independent frames of V views each in ONE launch, on point
    sets whose sizes live on the device (multi-view netC colours over counted vertex lists).  maps: list of n lists of
    V channels-last maps [H,W,C]; points: n contiguous f32 [3,cap] tensors (one cap; frame f's points are seen by all
    its views); counts: n device int32[1] tensors (<= cap); calibs: [n,V,>=3,4] or n sequences of V calibrations;
    projection, ``view``: one for all frames.  n <= ``max_view_frames(V)``.  Returns the list of n [Cout,cap] tensors
    (or ``outs``): columns [:count_f] of frame f hold row ``view`` of ``query_views`` on its maps, calibrations and
    points bit for bit, the other columns are left as they were (zeros in a fresh result).  Nothing is synchronised.
    f32 heads only; registered skip tables are not used."""
    who = "query_views_counted_batch"
    ctx = mlp.ctx
    n = len(maps)
    if n == 0 or len(points) != n or len(counts) != n or len(calibs) != n:
        raise ValueError("%s: %d frames, %d point sets, %d counts, %d sets of calibrations"
                         % (who, n, len(points), len(counts), len(calibs)))
    v_n = len(maps[0])
    _check_count(who, "views", v_n, MAX_VIEWS)
    if any(len(m) != v_n for m in maps):
        raise ValueError("%s: every frame needs the same number of views (%d)" % (who, v_n))
    _check_count(who, "frames of %d views" % v_n, n, max_view_frames(v_n))
    flat = [m for frame in maps for m in frame]
    h, w, c, dev = _maps(who, flat)
    cap = points[0].shape[-1]
    if any(tuple(p.shape) != (3, cap) or not p.is_contiguous() or p.dtype != torch.float32 for p in points):
        raise ValueError("%s: the point sets must be contiguous float32 [3,%d]" % (who, cap))
    if any(k.dtype != torch.int32 or k.numel() < 1 for k in counts):
        raise ValueError("%s: a count is an int32[1] tensor on the maps' device" % who)
    frames_cal = [_calib_list(frame, v_n, who) for frame in calibs]
    if outs is not None:
        if len(outs) != n:
            raise ValueError("%s: %d frames, %d outputs" % (who, n, len(outs)))
        if any(o.dim() != 2 or o.shape[1] != cap or not o.is_contiguous() or o.dtype != torch.float32 for o in outs):
            raise ValueError("%s: the outputs must be contiguous float32 [Cout,%d]" % (who, cap))
    cals = [_calib_dev(cb, dev) for frame in frames_cal for cb in frame]
    if outs is None:
        outs = [torch.zeros((mlp.cout, cap), dtype=torch.float32, device=dev) for _ in range(n)]
    elif any(o.shape[0] != mlp.cout for o in outs):
        raise ValueError("%s: the outputs must be contiguous float32 [%d,%d]" % (who, mlp.cout, cap))
    ctx.check(ctx.lib.mp_query_views_counted_batch(
        ctx.handle, mlp.id, n, v_n, _ptr_array(flat), c, h, w, _ptr_array(points), cap, _ptr_array(counts),
        _ptr_array(cals), _projection(projection), float(z_scale), int(view), _ptr_array(outs), _stream(outs[0])),
        "mp_query_views_counted_batch")
    _keep_until_done(dev, cals)
    return outs


class LevelEngine:
    """The coarse-to-fine engine one step at a time, for an ARBITRARY ``query_func``: node
    selection, lattice coordinates, conflict detection and scatter run as HIP kernels
    (csrc/octree.hip), the occupancies come from the caller; one host sync per step for the point
    count (as the upstream engine).  ``faster=True``: dilation boxes 9/7/3 by level, no conflict
    re-examination; ``faster=False``: 3^3 boxes at every level and, after each evaluation, the
    3x3x3 neighbourhoods of nodes whose exact value contradicts the interpolated one are evaluated
    too, until no contradiction is left."""

    def __init__(self, device, b_min, b_max, resolutions, balance=0.5, faster=True, final_level="dilate3",
                 num_points=None, max_dist=None):
        self.final_level = final_level
        _final_level(final_level)
        # the fixed-budget engine (mp_octree_select_topk): levels >= 1 select the num_points[l] most uncertain nodes
        self.num_points = self.max_dist = None
        if num_points is not None:
            if not faster or final_level != "dilate3":
                raise ValueError("LevelEngine: num_points replaces the selection rules of faster / final_level")
            self.num_points, self.max_dist = _topk_levels("LevelEngine", list(resolutions), num_points, max_dist)
        elif max_dist is not None:
            raise ValueError("LevelEngine: max_dist bounds the num_points selection")
        self.ctx = get_context(device)
        self.dev = torch.device(device)
        self.res = [int(r) for r in resolutions]
        self.rf = self.res[-1]
        self.balance = float(balance)
        self.faster = bool(faster)
        self.bmin, self.bmax = _float3(b_min), _float3(b_max)
        self.count = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.level = -1
        self.prev = self.ev_prev = None
        self.cur = self.ev_cur = self.packed = None
        self.counts = []       # points queried per level (conflict rounds included)
        self.rounds = []       # conflict rounds per level

    def _points(self, packed, n, r):
        pts = torch.empty((n, 3), dtype=torch.float32, device=self.dev)
        ctx = self.ctx
        ctx.check(ctx.lib.mp_lattice_points(ctx.handle, _ptr(packed), _ptr(self.count), n,
                                            (self.rf - 1) // (r - 1), self.rf, self.bmin, self.bmax,
                                            _ptr(pts), _stream(pts)), "mp_lattice_points")
        return pts

    def select(self):
        """Advance to the next level: returns the [n,3] world points to evaluate (n may be 0)."""
        self.level += 1
        level, r = self.level, self.res[self.level]
        ctx, dev = self.ctx, self.dev
        words = r * r * ((r + 63) // 64)
        if level > 0:
            self.prev, self.ev_prev = self.cur, self.ev_cur
        self.cur = torch.empty((r, r, r), dtype=torch.float32, device=dev)
        self.ev_cur = torch.empty((words,), dtype=torch.int64, device=dev)
        self.packed = torch.empty((r ** 3,), dtype=torch.int32, device=dev)
        if self.num_points is not None and level > 0:
            ctx.check(ctx.lib.mp_octree_select_topk(
                ctx.handle, _ptr(self.prev), self.res[level - 1], _ptr(self.cur), r, _ptr(self.ev_prev),
                _ptr(self.ev_cur), self.num_points[level], float("inf") if self.max_dist is None else self.max_dist[level],
                self.balance, _ptr(self.packed), _ptr(self.count), _stream(self.cur)), "mp_octree_select_topk")
            self.n = int(self.count.item())
            self.counts.append(self.n)
            self.rounds.append(0)
            if not self.n:
                return None
            # the list is filled through atomics: sort it for a reproducible evaluation order (as the conflict rounds)
            self.packed = torch.sort(self.packed[:self.n])[0].contiguous()
            return self._points(self.packed, self.n, r)
        bnd = torch.empty((words,), dtype=torch.int64, device=dev)
        box = 3 if not self.faster else {1: 9, 2: 7}.get(level, 3)
        if self.faster and level == len(self.res) - 1 and level > 0:
            # the last level's rule (mp_octree_select_box: 1 = upsampled mask == 0.5, undilated; 0 = none)
            box = {"dilate3": box, "upstream": 1, "interpolate": 0}[self.final_level]
        ctx.check(ctx.lib.mp_octree_select_box(
            ctx.handle, _ptr(self.prev) if level > 0 else None, self.res[level - 1] if level > 0 else 0,
            _ptr(self.cur), r, _ptr(self.ev_prev) if level > 0 else None, _ptr(self.ev_cur),
            _ptr(bnd), box, self.balance, _ptr(self.packed), _ptr(self.count), _stream(self.cur)),
            "mp_octree_select_box")
        self.n = int(self.count.item())
        self.counts.append(self.n)
        self.rounds.append(0)
        return self._points(self.packed, self.n, r) if self.n else None

    def _values(self, occ, n):
        if isinstance(occ, (list, tuple)):
            occ = torch.stack(list(occ))
        vals = _f32c(occ.reshape(-1))
        if vals.shape[0] != n:
            raise ValueError("query_func returned %d values for %d points" % (vals.shape[0], n))
        return vals

    def scatter(self, occ):
        """Hand over the occupancies of the points ``select`` (or the previous ``scatter``)
        returned.  Returns the next batch of points of THIS level to evaluate (faster=False:
        neighbourhoods of conflicting nodes) or None when the level is complete."""
        ctx, r, n = self.ctx, self.res[self.level], self.n
        vals = self._values(occ, n)
        nxt = None
        if not self.faster and self.level > 0:
            nxt = torch.empty((r ** 3,), dtype=torch.int32, device=self.dev)
            nxt_count = torch.zeros((1,), dtype=torch.int32, device=self.dev)
            ctx.check(ctx.lib.mp_octree_conflicts(
                ctx.handle, _ptr(self.packed), _ptr(self.count), n, r, _ptr(vals), _ptr(self.cur),
                self.balance, _ptr(self.ev_cur), _ptr(nxt), _ptr(nxt_count), _stream(vals)),
                "mp_octree_conflicts")
        ctx.check(ctx.lib.mp_scatter_nodes(ctx.handle, _ptr(self.packed), _ptr(self.count), n, r,
                                           _ptr(vals), _ptr(self.cur), _stream(self.cur)),
                  "mp_scatter_nodes")
        if nxt is None:
            return None
        m = int(nxt_count.item())
        if m == 0:
            return None
        # claimed through atomics: sort for a reproducible evaluation order
        self.packed = torch.sort(nxt[:m])[0].contiguous()
        self.count = nxt_count
        self.n = m
        self.counts[-1] += m
        self.rounds[-1] += 1
        return self._points(self.packed, m, r)

    def empty(self):
        """Level 0 only: nothing above the threshold (the engine then returns None)."""
        return not bool((self.cur > self.balance).any())


def recon_generic(query_func, kwargs, device, b_min, b_max, resolutions, balance=0.5, faster=True,
                  level0=None, final_level="dilate3", num_points=None, max_dist=None):
    """Seg3dLossless for an ARBITRARY ``query_func(points=[1,N,3], **kwargs) -> [1,1,N]`` on top
    of ``LevelEngine``.  ``level0`` = (engine, occupancies) when the caller has already evaluated
    the coarsest level through the engine.  ``num_points`` / ``max_dist``: the fixed-budget selection (Seg3dTopk,
    ``LevelEngine``) instead of the lossless rules.  Returns (volume [R,R,R] or None, per-level counts)."""
    if level0 is None:
        eng = LevelEngine(device, b_min, b_max, resolutions, balance, faster, final_level, num_points, max_dist)
        pts = eng.select()
        occ = query_func(points=pts[None], **kwargs)
    else:
        eng, occ = level0
    eng.scatter(occ)
    if eng.empty():
        return None, eng.counts
    for _ in range(1, len(eng.res)):
        pts = eng.select()
        while pts is not None:
            pts = eng.scatter(query_func(points=pts[None], **kwargs))
    return eng.cur, eng.counts


def octree_order_points(packed, counts, calibs, level_res, stride, res_final, b_min, b_max, h, w, projections=None):
    """mp_octree_order_points: sort each frame's node list (``packed[f]``: int32 codes x | y<<10 | z<<20, the first
    ``counts[f]`` (device int32[1]) of them) IN PLACE by the texel cell of an [h,w] map its points sample -- the step
    ``recon_batch`` runs between a level's selection and its query.  The order inside a cell is unspecified; a frame
    with more than level_res^3 / 8 points is left as it is.  Nothing is synchronised."""
    who = "octree_order_points"
    n = len(packed)
    _check_count(who, "frames", n, MAX_FRAMES)
    if len(counts) != n or (projections is not None and len(projections) != n):
        raise ValueError("%s: %d lists, %d counts, %s projections"
                         % (who, n, len(counts), None if projections is None else len(projections)))
    dev = packed[0].device
    if any(p.dtype != torch.int32 or not p.is_contiguous() for p in packed):
        raise ValueError("%s: the lists must be contiguous int32" % who)
    ctx = get_context(dev)
    cals = [_calib_dev(cb, dev) for cb in _calib_list(calibs, n, who)]
    proj = None if projections is None else (ctypes.c_int * n)(*[_projection(p) for p in projections])
    ctx.check(ctx.lib.mp_octree_order_points(
        ctx.handle, n, _ptr_array(packed), _ptr_array(counts), _ptr_array(cals), proj, int(level_res), int(stride),
        int(res_final), _float3(b_min), _float3(b_max), int(h), int(w), _stream(packed[0])), "mp_octree_order_points")
    _keep_until_done(dev, cals)


def stream_release(stream):
    """Free the scratch arena the context keeps for ``stream`` (a torch.cuda.Stream); call it when
    a stream that made C-ABI calls is retired.  Synchronises the device."""
    for ctx in (get_context(stream.device), get_encoder_context(stream.device)):
        ctx.check(ctx.lib.mp_stream_release(ctx.handle, ctypes.c_void_p(stream.cuda_stream)),
                  "mp_stream_release")


# ---- recorded launch sequences (mp_plan_*, csrc/plan.hip) --------------------------------------------
_plan_tls = threading.local()


class Plan:
    """A recorded sequence of encoder launches (mp_plan): ``run()`` replays it on the current stream with ONE
    foreign call.  Keeps every tensor the commands point at alive."""

    def __init__(self, ctx, handle, keep, n_cmds):
        self.ctx, self.handle, self.keep, self.n_cmds = ctx, handle, keep, n_cmds

    def run(self, device):
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        self.ctx.check(self.ctx.lib.mp_plan_run(self.handle, st), "mp_plan_run")

    def __del__(self):
        try:
            self.ctx.lib.mp_plan_destroy(self.handle)
        except Exception:  # interpreter shutdown
            pass


class record_plan:
    """Context manager (per host thread): the encoder wrappers below (convk, gn_apply, conv3x3_fused,
    conv1x1_fused, avgpool2_gn, upsample_add_gn, GnArena, plan_wait) run normally AND append what they
    launched to a plan; ``.finish()`` builds it.  The stream that is current on entry is slot 0, other
    streams get slots in order of first use."""

    def __init__(self, device, keep_alive=True):
        """``keep_alive=False``: the caller guarantees the lifetime of every buffer itself (a private
        allocator pool that outlives the plan); the plan then holds no tensor references, so the pass it is
        recorded from recycles its intermediates as a launch-by-launch pass does."""
        self.ctx = get_encoder_context(device)
        self.device = torch.device(device)
        self.keep_alive = bool(keep_alive)
        self.cmds, self.keep = [], []
        self.slots = {torch.cuda.current_stream(self.device).cuda_stream: 0}

    def __enter__(self):
        if getattr(_plan_tls, "rec", None) is not None:
            raise RuntimeError("record_plan does not nest")
        _plan_tls.rec = self
        return self

    def __exit__(self, *exc):
        _plan_tls.rec = None
        return False

    def slot(self, stream=None):
        h = (stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream
        if h not in self.slots:
            self.slots[h] = len(self.slots)
        return self.slots[h]

    def add(self, kind, struct, tensors=()):
        self.cmds.append((kind, bytes(struct), self.slot()))
        if self.keep_alive:
            self.keep.extend(t for t in tensors if t is not None)

    def finish(self):
        ctx = self.ctx
        handle = ctypes.c_void_p()
        ctx.check(ctx.lib.mp_plan_create(ctx.handle, len(self.slots) - 1, ctypes.byref(handle)), "mp_plan_create")
        plan = Plan(ctx, handle, self.keep, len(self.cmds))
        for kind, blob, slot in self.cmds:
            buf = ctypes.create_string_buffer(blob, len(blob))
            ctx.check(ctx.lib.mp_plan_add(handle, kind, ctypes.cast(buf, ctypes.c_void_p), len(blob), slot),
                      "mp_plan_add")
        return plan


def _recording():
    return getattr(_plan_tls, "rec", None)


def plan_wait(waiter, signaller):
    """``waiter.wait_stream(signaller)`` (torch streams) that a plan being recorded remembers."""
    waiter.wait_stream(signaller)
    rec = _recording()
    if rec is not None:
        w = _lib.PlanWaitArgs()
        w.waiter_slot, w.signaller_slot = rec.slot(waiter), rec.slot(signaller)
        rec.cmds.append((_lib.PLAN_WAIT, bytes(w), 0))


def _forward_vertices(who, volumes, direction):
    """What forward_vertices_raw and forward_vertices_raw_batch do: per volume (X, Y, Z, norm, count), rows of five
    tensors."""
    vols, n, r, dev = _one_size_volumes(who, volumes)
    ctx = get_context(dev)
    cap = r * r
    x = torch.empty((n, cap), dtype=torch.int64, device=dev).unbind(0)
    y = torch.empty((n, cap), dtype=torch.int64, device=dev).unbind(0)
    z = torch.empty((n, cap), dtype=torch.float32, device=dev).unbind(0)
    nrm = torch.empty((n, cap, 3), dtype=torch.float32, device=dev).unbind(0)
    count = torch.empty((n, 1), dtype=torch.int32, device=dev).unbind(0)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_forward_vertices_batch(
            ctx.handle, f1 - f0, _ptr_array(vols[f0:f1]), r, DIRECTIONS[direction], _ptr_array(x[f0:f1]),
            _ptr_array(y[f0:f1]), _ptr_array(z[f0:f1]), _ptr_array(nrm[f0:f1]), _ptr_array(count[f0:f1]),
            _stream(vols[0])), "mp_forward_vertices_batch")
    _keep_until_done(dev, vols)
    return list(zip(x, y, z, nrm, count))


def forward_vertices_raw(volume, direction="front"):
    """mp_forward_vertices_batch with one frame: returns capacity-sized (X, Y, Z, norm, count) device tensors."""
    return _forward_vertices("forward_vertices", [volume], direction)[0]


def forward_vertices_raw_batch(volumes, direction="front"):
    """mp_forward_vertices_batch: ``[forward_vertices_raw(v, direction) for v in volumes]`` (cubic volumes of one
    size) in one set of launches per MAX_FRAMES volumes; every frame's (X, Y, Z, norm, count) are views of five
    tensors."""
    return _forward_vertices("forward_vertices_raw_batch", volumes, direction)


def _paint(xs, ys, values, channel_major, counts, res, scale, bias, lo, hi):
    """What paint and paint_batch do: per frame an image [res,res,3], rows of one tensor."""
    n = len(xs)
    dev = xs[0].device
    ctx = get_context(dev)
    cap = xs[0].shape[0]
    vals = [_f32c(v) for v in values]
    images = torch.empty((n, res, res, 3), dtype=torch.float32, device=dev).unbind(0)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_paint_batch(
            ctx.handle, f1 - f0, _ptr_array(xs[f0:f1]), _ptr_array(ys[f0:f1]), _ptr_array(vals[f0:f1]),
            int(channel_major), _ptr_array(counts[f0:f1]), cap, int(res), float(scale), float(bias), float(lo),
            float(hi), _ptr_array(images[f0:f1]), _stream(images[0])), "mp_paint_batch")
    _keep_until_done(dev, vals)
    return list(images)


def paint_batch(xs, ys, values, channel_major, counts, res, scale, bias, lo, hi):
    """mp_paint_batch: ``[paint(x, y, v, channel_major, c, res, ...) for ...]`` (renders of one size, one capacity)
    in two launches per MAX_FRAMES renders; the images are views of one [n, res, res, 3] tensor."""
    return _paint(xs, ys, values, channel_major, counts, res, scale, bias, lo, hi)


def vertex_points(x, y, z, count, res, mat):
    """(X, Y, res - Z) through the voxel->world matrix (RTL/main.py:231-237) -> [3,cap]."""
    ctx = get_context(x.device)
    cap = x.shape[0]
    m = (ctypes.c_float * 16)(*[float(v) for v in np.asarray(mat, np.float32).reshape(16)])
    pts = torch.zeros((3, cap), dtype=torch.float32, device=x.device)
    ctx.check(ctx.lib.mp_vertex_points(ctx.handle, _ptr(x), _ptr(y), _ptr(z), _ptr(count), cap,
                                       int(res), m, _ptr(pts), _stream(pts)), "mp_vertex_points")
    return pts


def paint(x, y, values, channel_major, count, res, scale, bias, lo, hi):
    """canvas of ones [res,res,3] with image[X,Y,:] = clamp(values*scale+bias) (main.py:220-248): mp_paint_batch
    with one frame."""
    return _paint([x], [y], [values], channel_major, [count], res, scale, bias, lo, hi)[0]


def visualize(image, size=256):
    """mp_visualize: ([size,size,3] f32 = 255 * rot90 + nearest resize of ``image`` [res,res,3],
    [size,size] uint8 foreground mask) on device."""
    ctx = get_context(image.device)
    img = _f32c(image)
    res = img.shape[0]
    out = torch.empty((size, size, 3), dtype=torch.float32, device=img.device)
    mask = torch.empty((size, size), dtype=torch.uint8, device=img.device)
    ctx.check(ctx.lib.mp_visualize(ctx.handle, _ptr(img), res, int(size), _ptr(out), _ptr(mask),
                                   _stream(img)), "mp_visualize")
    return out, mask


def prepare_inputs(segm, mean, std, with_color=True):
    """RTL/main.py:352-364 in one kernel: segm [1,4,H,W] (RGB in [-1,1] + mask) ->
    (input_netG [1,3,H,W] normalised and background-zeroed, input_netC [1,3,H,W] or None)."""
    sg = _f32c(segm)
    if sg.dim() != 4 or sg.shape[0] != 1 or sg.shape[1] != 4:
        raise ValueError("segm must be [1,4,H,W], got %s" % (tuple(segm.shape),))
    ctx = get_context(sg.device)
    hw = sg.shape[2] * sg.shape[3]
    g = torch.empty((1, 3) + tuple(sg.shape[2:]), dtype=torch.float32, device=sg.device)
    c = torch.empty_like(g) if with_color else None
    ctx.check(ctx.lib.mp_prepare_inputs(ctx.handle, _ptr(sg), hw, _float3(mean), _float3(std), _ptr(g),
                                        _ptr(c) if c is not None else None, _stream(sg)),
              "mp_prepare_inputs")
    return g, c


# MP_NORMALS_* (include/monoport_hip.h): what the reference's compute_normal computes / what its comments describe
NORMALS_MODES = {"reference": _lib.NORMALS_REFERENCE, "accumulate": _lib.NORMALS_ACCUMULATE}


def _normals_mode(mode):
    if isinstance(mode, str):
        if mode not in NORMALS_MODES:
            raise ValueError("normals mode must be one of %s, got %r" % (sorted(NORMALS_MODES), mode))
        return NORMALS_MODES[mode]
    return int(mode)


def _mesh_buffers(verts, faces, counts):
    if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3 or not verts.is_contiguous():
        raise ValueError("verts must be a contiguous [V,3] float32 tensor")
    if faces is not None and (faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3
                              or not faces.is_contiguous()):
        raise ValueError("faces must be a contiguous [F,3] int32 tensor")
    if counts.dtype != torch.int32 or counts.numel() < 2 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int32 tensor of (vertices, faces)")
    for t in (faces, counts):
        if t is not None and t.device != verts.device:
            raise ValueError("verts, faces and counts must live on one device")


def _frame_rows(who, what, t, n, shape, dtype, device):
    """A caller's buffers of a mesh call, one per frame (a tensor [n, *shape], or a sequence of n tensors [*shape]) ->
    the sequence of them: ``dtype`` on ``device``, each contiguous."""
    rows = None if t is None else tuple(t)
    if rows is None or len(rows) != n or any(
            r is None or tuple(r.shape) != tuple(shape) or r.dtype != dtype or r.device != device
            or not r.is_contiguous() for r in rows):
        raise ValueError("%s: %s must be %s %s on %s with contiguous frames"
                         % (who, what, str(dtype).replace("torch.", ""), [n] + list(shape), device))
    return rows


def _mesh_frames(who, verts, faces, counts):
    """The meshes of one call (``_mesh_buffers`` each, one capacity for all) -> (n, max_v, max_f, device)."""
    n = len(verts)
    if n == 0:
        raise ValueError("%s wants at least one mesh" % who)
    if len(counts) != n or (faces is not None and len(faces) != n):
        raise ValueError("%s: %d vertex buffers, %s face buffers, %d counts"
                         % (who, n, None if faces is None else len(faces), len(counts)))
    for f in range(n):
        _mesh_buffers(verts[f], None if faces is None else faces[f], counts[f])
    max_v = verts[0].shape[0]
    max_f = 0 if faces is None else faces[0].shape[0]
    if (any(v.shape[0] != max_v or v.device != verts[0].device for v in verts)
            or (faces is not None and any(f.shape[0] != max_f for f in faces))):
        raise ValueError("%s: one capacity (and one device) serves all meshes of a call" % who)
    return n, max_v, max_f, verts[0].device


# Each stage below is one private body over lists of frames; the per-frame wrapper passes one-element lists and returns
# element 0, so it checks, allocates and launches exactly as its _batch twin does.

def _marching_cubes(who, volumes, level, b_min, b_max, max_verts, max_faces, gates, out):
    vols, n, r, dev = _one_size_volumes(who, volumes)
    _gates(who, gates, n, dev)
    if out is not None:
        verts, faces, counts = out
        if max_verts is None:
            max_verts = verts.shape[1]
        if max_faces is None:
            max_faces = faces.shape[1]
    if max_verts is None:
        max_verts = 12 * r * r  # a closed body at resolution r has O(r^2) surface cells
    if max_faces is None:
        max_faces = 2 * max_verts
    if out is None:
        verts = torch.empty((n, max_verts, 3), dtype=torch.float32, device=dev).unbind(0)
        faces = torch.empty((n, max_faces, 3), dtype=torch.int32, device=dev).unbind(0)
        counts = torch.empty((n, 2), dtype=torch.int32, device=dev).unbind(0)
    else:
        verts = _frame_rows(who, "out[0] (verts)", verts, n, (max_verts, 3), torch.float32, dev)
        faces = _frame_rows(who, "out[1] (faces)", faces, n, (max_faces, 3), torch.int32, dev)
        counts = _frame_rows(who, "out[2] (counts)", counts, n, (2,), torch.int32, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_marching_cubes_batch(
            ctx.handle, f1 - f0, _ptr_array(vols[f0:f1]), r, float(level), _float3(b_min), _float3(b_max),
            _ptr_array(verts[f0:f1]), max_verts, _ptr_array(faces[f0:f1]), max_faces, _ptr_array(counts[f0:f1]),
            None if gates is None else _ptr_array(gates[f0:f1]), _stream(vols[0])), "mp_marching_cubes_batch")
    _keep_until_done(dev, vols, gates)
    return list(zip(verts, faces, counts))


def marching_cubes_raw(volume, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1), max_verts=None,
                       max_faces=None):
    """mp_marching_cubes_batch with one frame: capacity-sized (verts [max_v,3] f32, faces [max_f,3] int32,
    counts int32[2] = needed vertices / faces) on device, no host sync."""
    return _marching_cubes("marching_cubes", [volume], level, b_min, b_max, max_verts, max_faces, None, None)[0]


def marching_cubes_raw_batch(volumes, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1), max_verts=None,
                             max_faces=None, gates=None, out=None):
    """mp_marching_cubes_batch: ``[marching_cubes_raw(v, ...) for v in volumes]`` (cubic volumes of one size, one
    capacity) in one set of four launches per MAX_FRAMES volumes; every frame's (verts [max_v,3], faces [max_f,3],
    counts int32[2]) are views of three tensors, bit for bit what the per-volume call gives.  ``gates``: per-frame
    device int32 tensors (or None entries = frame on); a frame whose gate reads 0 gets counts (0, 0) and nothing
    else of it is read or written.  ``out``: (verts [n,max_v,3] f32, faces [n,max_f,3] int32, counts [n,2] int32)
    to write into.  No host sync."""
    return _marching_cubes("marching_cubes_raw_batch", volumes, level, b_min, b_max, max_verts, max_faces, gates, out)


def _mesh_normals(who, verts, faces, counts, mode, out):
    n, max_v, max_f, dev = _mesh_frames(who, verts, faces, counts)
    code = _normals_mode(mode)
    if out is None:
        out = torch.empty((n, max_v, 3), dtype=torch.float32, device=dev).unbind(0)
    else:
        out = _frame_rows(who, "out", out, n, (max_v, 3), torch.float32, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_normals_batch(
            ctx.handle, f1 - f0, _ptr_array(verts[f0:f1]), max_v, _ptr_array(faces[f0:f1]), max_f,
            _ptr_array(counts[f0:f1]), code, _ptr_array(out[f0:f1]), _stream(verts[0])), "mp_mesh_normals_batch")
    return list(out)


def mesh_normals_raw(verts, faces, counts, mode="accumulate", out=None):
    """mp_mesh_normals_batch with one frame: verts [max_v,3] f32, faces [max_f,3] int32, counts int32[2] on device (as
    ``marching_cubes_raw`` returns them) -> normals [max_v,3] f32 (``out`` itself if given); rows beyond counts[0]
    are not written.  No host sync."""
    return _mesh_normals("mesh_normals_raw", [verts], [faces], [counts], mode, None if out is None else [out])[0]


def mesh_normals_raw_batch(verts, faces, counts, mode="accumulate", out=None):
    """mp_mesh_normals_batch: ``[mesh_normals_raw(v, f, c, mode) for v, f, c in zip(verts, faces, counts)]`` (lists
    of per-mesh device tensors as ``marching_cubes_raw_batch`` returns them, one capacity) in the launches of ONE
    mesh per MAX_FRAMES meshes; the normals are views of one [n,max_v,3] tensor (``out`` if given), bit for bit what
    the per-mesh call gives; rows beyond a mesh's counts[0] are not written.  No host sync."""
    return _mesh_normals("mesh_normals_raw_batch", verts, faces, counts, mode, out)


SIMPLIFY_MAX_CELLS = 512  # mp_mesh_simplify: cells per axis in 1..512


def _simplify_cells(who, cells):
    if isinstance(cells, bool) or not isinstance(cells, (int, np.integer)) or not 1 <= cells <= SIMPLIFY_MAX_CELLS:
        raise ValueError("%s: cells per axis must be an int in 1..%d, got %r" % (who, SIMPLIFY_MAX_CELLS, cells))
    return int(cells)


def _mesh_simplify(who, verts, faces, counts, cells, b_min, b_max, out):
    n, max_v, max_f, dev = _mesh_frames(who, verts, faces, counts)
    cells = _simplify_cells(who, cells)
    if out is None:
        verts_out = torch.empty((n, max_v, 3), dtype=torch.float32, device=dev).unbind(0)
        faces_out = torch.empty((n, max_f, 3), dtype=torch.int32, device=dev).unbind(0)
        counts_out = torch.empty((n, 2), dtype=torch.int32, device=dev).unbind(0)
        vmap = torch.empty((n, max_v), dtype=torch.int32, device=dev).unbind(0)
    else:
        verts_out = _frame_rows(who, "out[0] (verts)", out[0], n, (max_v, 3), torch.float32, dev)
        faces_out = _frame_rows(who, "out[1] (faces)", out[1], n, (max_f, 3), torch.int32, dev)
        counts_out = _frame_rows(who, "out[2] (counts)", out[2], n, (2,), torch.int32, dev)
        vmap = _frame_rows(who, "out[3] (vmap)", out[3], n, (max_v,), torch.int32, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_simplify_batch(
            ctx.handle, f1 - f0, _ptr_array(verts[f0:f1]), max_v, _ptr_array(faces[f0:f1]), max_f,
            _ptr_array(counts[f0:f1]), _float3(b_min), _float3(b_max), cells, _ptr_array(verts_out[f0:f1]),
            _ptr_array(faces_out[f0:f1]), _ptr_array(counts_out[f0:f1]), _ptr_array(vmap[f0:f1]),
            _stream(verts[0])), "mp_mesh_simplify_batch")
    return list(zip(verts_out, faces_out, counts_out, vmap))


def mesh_simplify_raw(verts, faces, counts, cells, b_min=(-1, -1, -1), b_max=(1, 1, 1), out=None):
    """mp_mesh_simplify_batch with one frame: the vertex clustering of verts [max_v,3] f32, faces [max_f,3] int32,
    counts int32[2] on device (as ``marching_cubes_raw`` returns them) on ``cells``^3 cells over the box -> (verts_out
    [max_v,3], faces_out [max_f,3], counts_out int32[2], vmap int32 [max_v] = new index of every old vertex, -1 for an
    invalid one); rows beyond the new counts (of vmap: beyond the old vertex count) are not written.  ``out``: these
    four to write into.  No host sync."""
    return _mesh_simplify("mesh_simplify_raw", [verts], [faces], [counts], cells, b_min, b_max,
                          None if out is None else [[o] for o in out])[0]


def mesh_simplify_raw_batch(verts, faces, counts, cells, b_min=(-1, -1, -1), b_max=(1, 1, 1), out=None):
    """mp_mesh_simplify_batch: ``[mesh_simplify_raw(v, f, c, cells, b_min, b_max) for v, f, c in zip(verts, faces,
    counts)]`` (lists of per-mesh device tensors, one capacity) in ONE set of launches per MAX_FRAMES meshes; the
    results are views of four tensors (``out`` = (verts [n,max_v,3], faces [n,max_f,3], counts [n,2], vmap [n,max_v])
    if given), bit for bit what the per-mesh call gives.  No host sync."""
    return _mesh_simplify("mesh_simplify_raw_batch", verts, faces, counts, cells, b_min, b_max, out)


SMOOTH_MAX_ITERATIONS = 64  # mp_mesh_smooth: 1..64 iterations of a lambda and a mu pass
SMOOTH_PIN_BORDER = 1  # MP_SMOOTH_PIN_BORDER


def _smooth_params(who, iterations, lam, mu, pin_border):
    """The parameters of mp_mesh_smooth as the C side takes them: (iterations, lambda, mu, flags)."""
    if (isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer))
            or not 1 <= iterations <= SMOOTH_MAX_ITERATIONS):
        raise ValueError("%s: iterations must be an int in 1..%d, got %r" % (who, SMOOTH_MAX_ITERATIONS, iterations))
    for name, x in (("lam", lam), ("mu", mu)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or \
                not abs(float(x)) <= float(np.finfo(np.float32).max):  # false for NaN too
            raise ValueError("%s: %s must be a finite f32 number, got %r" % (who, name, x))
    if not isinstance(pin_border, (bool, np.bool_)):
        raise ValueError("%s: pin_border must be a bool, got %r" % (who, pin_border))
    return int(iterations), float(np.float32(lam)), float(np.float32(mu)), SMOOTH_PIN_BORDER if pin_border else 0


def _mesh_smooth(who, verts, faces, counts, iterations, lam, mu, pin_border, out, ring):
    n, max_v, max_f, dev = _mesh_frames(who, verts, faces, counts)
    iterations, lam, mu, flags = _smooth_params(who, iterations, lam, mu, pin_border)
    if out is None:
        verts_out = torch.empty((n, max_v, 3), dtype=torch.float32, device=dev).unbind(0)
    else:
        verts_out = _frame_rows(who, "out", out, n, (max_v, 3), torch.float32, dev)
    if ring is True:
        ring = torch.empty((n, max_v), dtype=torch.int32, device=dev).unbind(0)
    elif ring is not False and ring is not None:
        ring = _frame_rows(who, "ring", ring, n, (max_v,), torch.int32, dev)
    else:
        ring = None
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_smooth_batch(
            ctx.handle, f1 - f0, _ptr_array(verts[f0:f1]), max_v, _ptr_array(faces[f0:f1]), max_f,
            _ptr_array(counts[f0:f1]), iterations, lam, mu, flags, _ptr_array(verts_out[f0:f1]),
            None if ring is None else _ptr_array(ring[f0:f1]), _stream(verts[0])), "mp_mesh_smooth_batch")
    return list(verts_out) if ring is None else list(zip(verts_out, ring))


def mesh_smooth_raw(verts, faces, counts, iterations, lam=0.5, mu=-0.53, pin_border=True, out=None, ring=False):
    """mp_mesh_smooth_batch with one frame: ``iterations`` (1..64) Taubin iterations -- a pass with ``lam``, then one
    with ``mu``, of the umbrella operator over the one-ring (include/monoport_hip.h) -- on verts [max_v,3] f32, faces
    [max_f,3] int32, counts int32[2] on device (as ``marching_cubes_raw`` / ``mesh_simplify_raw`` return them) ->
    verts_out [max_v,3]; rows beyond the vertex count are not written, faces and counts are the input's.
    ``pin_border``: vertices of an edge that lies in an odd number of faces keep their bits.  ``out``: the tensor to
    write into.  ``ring``: True, or an int32 [max_v] tensor to write into: the result is then (verts_out, ring), ring =
    the number of distinct neighbours of every vertex, negated for a border vertex.  No host sync."""
    return _mesh_smooth("mesh_smooth_raw", [verts], [faces], [counts], iterations, lam, mu, pin_border,
                        None if out is None else [out], ring if isinstance(ring, bool) or ring is None else [ring])[0]


def mesh_smooth_raw_batch(verts, faces, counts, iterations, lam=0.5, mu=-0.53, pin_border=True, out=None,
                          ring=False):
    """mp_mesh_smooth_batch: ``[mesh_smooth_raw(v, f, c, iterations, lam, mu, pin_border, ring=ring) for v, f, c in
    zip(verts, faces, counts)]`` (lists of per-mesh device tensors, one capacity) in ONE set of launches per MAX_FRAMES
    meshes; the results are views of one tensor each (``out`` = verts [n,max_v,3], ``ring`` = [n,max_v] if given), bit
    for bit what the per-mesh call gives.  No host sync."""
    return _mesh_smooth("mesh_smooth_raw_batch", verts, faces, counts, iterations, lam, mu, pin_border, out, ring)


# MP_GLB_* (include/monoport_hip.h)
GLB_COLOR_LAYOUTS = {"rows": _lib.GLB_COLOR_ROWS, "planes": _lib.GLB_COLOR_PLANES}
GLB_MIN_BYTES = 100  # MP_GLB_MIN_BYTES: the empty file


def _glb_flags(normals, colors):
    return (_lib.GLB_NORMALS if normals else 0) | (_lib.GLB_COLORS if colors else 0)


def glb_bytes(nv, nf, normals=True, colors=True):
    """mp_glb_bytes: the size of the binary glTF file of a mesh of ``nv`` vertices and ``nf`` faces with or without
    normals and colours -- a closed form (include/monoport_hip.h); the empty file's 100 bytes if either count is 0."""
    for v in (nv, nf):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("glb_bytes: nv and nf must be ints >= 0, got %r and %r" % (nv, nf))
    return int(_lib.load().mp_glb_bytes(int(nv), int(nf), _glb_flags(normals, colors)))


def glb_max_bytes(max_verts, max_faces, normals=True, colors=True):
    """mp_glb_max_bytes: what no file of a mesh within these capacities exceeds: ``glb_bytes`` at the capacities."""
    for v in (max_verts, max_faces):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("glb_max_bytes: the capacities must be ints >= 0, got %r and %r" % (max_verts, max_faces))
    return int(_lib.load().mp_glb_max_bytes(int(max_verts), int(max_faces), _glb_flags(normals, colors)))


def _mesh_glb(who, verts, faces, counts, normals, colors, color_layout, color_scale, color_bias, b_min, b_max,
              capacity, out, info):
    n, max_v, max_f, dev = _mesh_frames(who, verts, faces, counts)
    layout = _named_mode(who, "color_layout", GLB_COLOR_LAYOUTS, color_layout)
    scale, bias = _finite_float(who, "color_scale", color_scale), _finite_float(who, "color_bias", color_bias)
    if normals is not None:
        normals = _frame_rows(who, "normals", normals, n, (max_v, 3), torch.float32, dev)
    if colors is not None:
        colors = _frame_rows(who, "colors", colors, n, (3, max_v) if layout == _lib.GLB_COLOR_PLANES else (max_v, 3),
                             torch.float32, dev)
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != n
                or not out.is_contiguous() or out.device != dev):
            raise ValueError("%s: out must be a contiguous uint8 tensor [%d,capacity] on %s" % (who, n, dev))
        if capacity is not None and int(capacity) != out.shape[1]:
            raise ValueError("%s: capacity %r against an out of %d bytes per mesh" % (who, capacity, out.shape[1]))
        capacity = int(out.shape[1])
    elif capacity is None:
        capacity = glb_max_bytes(max_v, max_f, normals is not None, colors is not None)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < GLB_MIN_BYTES:
        raise ValueError("%s: capacity must be an int >= the empty file's %d bytes, got %r"
                         % (who, GLB_MIN_BYTES, capacity))
    if info is None:
        info = torch.empty((n, 2), dtype=torch.int32, device=dev)
    elif (not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or tuple(info.shape) != (n, 2)
          or not info.is_contiguous() or info.device != dev):
        raise ValueError("%s: info must be a contiguous int32 tensor [%d,2] on %s" % (who, n, dev))
    if out is None:
        out = torch.empty((n, int(capacity)), dtype=torch.uint8, device=dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_glb_batch(
            ctx.handle, f1 - f0, _ptr_array(verts[f0:f1]), max_v, _ptr_array(faces[f0:f1]), max_f,
            _ptr_array(counts[f0:f1]), None if normals is None else _ptr_array(normals[f0:f1]),
            None if colors is None else _ptr_array(colors[f0:f1]), layout, scale, bias, _float3(b_min), _float3(b_max),
            _ptr(out[f0:f1]), int(capacity), _ptr(info[f0:f1]), _stream(verts[0])), "mp_mesh_glb_batch")
    _keep_until_done(dev, verts, faces, counts, normals, colors)
    return out, info


def mesh_glb_raw(verts, faces, counts, normals=None, colors=None, color_layout="rows", color_scale=1.0,
                 color_bias=0.0, b_min=(-1, -1, -1), b_max=(1, 1, 1), capacity=None, out=None, info=None):
    """mp_mesh_glb_batch with one frame: the quantised binary glTF file of verts [max_v,3] f32, faces [max_f,3] int32,
    counts int32[2] on device (as the mesh chain leaves them), with ``normals`` [max_v,3] and ``colors`` ([max_v,3]
    under "rows", [3,max_v] under "planes"; byte = the 8-bit rule on ``p * color_scale + color_bias``) if given ->
    (out uint8 [1,capacity], info int32 [1,2]) as ``picture_jpeg_raw`` returns them: the file is ``out[0, :info[0, 0]]``
    where ``info[0, 1] == 0``; where it is 1 nothing was written and ``info[0, 0]`` is the capacity it needs.
    ``capacity``: None = ``glb_max_bytes`` (never overflows).  Three launches; no host sync."""
    return _mesh_glb("mesh_glb_raw", [verts], [faces], [counts], None if normals is None else [normals],
                     None if colors is None else [colors], color_layout, color_scale, color_bias, b_min, b_max,
                     capacity, out, info)


def mesh_glb_raw_batch(verts, faces, counts, normals=None, colors=None, color_layout="rows", color_scale=1.0,
                       color_bias=0.0, b_min=(-1, -1, -1), b_max=(1, 1, 1), capacity=None, out=None, info=None):
    """mp_mesh_glb_batch: the files of ``mesh_glb_raw`` for lists of per-mesh device tensors of one capacity (``normals``
    / ``colors``: None, or one tensor per mesh) in ONE set of three launches per MAX_FRAMES meshes -> (out uint8
    [n,capacity], info int32 [n,2]), row f byte for byte what the per-mesh call gives.  No host sync."""
    return _mesh_glb("mesh_glb_raw_batch", verts, faces, counts, normals, colors, color_layout, color_scale,
                     color_bias, b_min, b_max, capacity, out, info)


# MP_ATLAS_* (include/monoport_hip.h)
ATLAS_MIN_SIZE, ATLAS_MAX_SIZE = 64, 4096
ATLAS_MIN_CELL, ATLAS_MAX_CELL = 4, 64


def atlas_params(who, size, cell):
    """(A, T) of mp_mesh_atlas, checked: A a power of two in 64..4096, T in 4..64."""
    for name, v in (("size", size), ("cell", cell)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: %s must be an int, got %r" % (who, name, v))
    if not ATLAS_MIN_SIZE <= size <= ATLAS_MAX_SIZE or size & (size - 1):
        raise ValueError("%s: size must be a power of two in %d..%d, got %r" % (who, ATLAS_MIN_SIZE, ATLAS_MAX_SIZE, size))
    if not ATLAS_MIN_CELL <= cell <= ATLAS_MAX_CELL:
        raise ValueError("%s: cell must be in %d..%d, got %r" % (who, ATLAS_MIN_CELL, ATLAS_MAX_CELL, cell))
    return int(size), int(cell)


def atlas_faces(size, cell):
    """The faces an atlas of side ``size`` with cells of side ``cell`` holds: 2 G^2 with G = size // cell."""
    size, cell = atlas_params("atlas_faces", size, cell)
    return 2 * (size // cell) ** 2


def _mesh_atlas(who, verts, faces, counts, size, cell, background, out):
    n, max_v, max_f, dev = _mesh_frames(who, verts, faces, counts)
    size, cell = atlas_params(who, size, cell)
    background = _finite_float(who, "background", background)
    if out is None:
        face_id = torch.empty((n, size, size), dtype=torch.int32, device=dev).unbind(0)
        position = torch.empty((n, size, size, 3), dtype=torch.float32, device=dev).unbind(0)
        info = torch.empty((n, 2), dtype=torch.int32, device=dev).unbind(0)
    else:
        face_id = _frame_rows(who, "out[0] (face_id)", out[0], n, (size, size), torch.int32, dev)
        position = _frame_rows(who, "out[1] (position)", out[1], n, (size, size, 3), torch.float32, dev)
        info = _frame_rows(who, "out[2] (info)", out[2], n, (2,), torch.int32, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_atlas_batch(
            ctx.handle, f1 - f0, _ptr_array(verts[f0:f1]), max_v, _ptr_array(faces[f0:f1]), max_f,
            _ptr_array(counts[f0:f1]), size, cell, background, _ptr_array(face_id[f0:f1]),
            _ptr_array(position[f0:f1]), _ptr_array(info[f0:f1]), _stream(verts[0])), "mp_mesh_atlas_batch")
    _keep_until_done(dev, verts, faces, counts)
    return list(zip(face_id, position, info))


def mesh_atlas_raw(verts, faces, counts, size, cell, background=0.5, out=None):
    """mp_mesh_atlas_batch with one frame: the texture-space G-buffer of verts [max_v,3] f32, faces [max_f,3] int32,
    counts int32[2] on device in an atlas of side ``size`` (a power of two in 64..4096) with cells of side ``cell``
    (4..64), bit for bit as include/monoport_hip.h defines it -> (face_id int32 [size,size], position float32
    [size,size,3], info int32[2] = (faces laid out, faces of the mesh)): what one view of the rasteriser with ``attr =
    verts`` is in screen space, for ``picture_points`` / ``picture_paint`` / ``picture_png_raw``.  Texels of no face
    hold -1 and ``background``; every texel is written.  ``out``: these three to write into.  One launch; no host
    sync."""
    return _mesh_atlas("mesh_atlas_raw", [verts], [faces], [counts], size, cell, background,
                       None if out is None else tuple([o] for o in out))[0]


def mesh_atlas_raw_batch(verts, faces, counts, size, cell, background=0.5, out=None):
    """mp_mesh_atlas_batch: ``[mesh_atlas_raw(v, f, c, size, cell, background) for ...]`` (lists of per-mesh device
    tensors of one capacity) in ONE launch per MAX_FRAMES meshes, the same bits.  ``out``: (face_id [n,size,size],
    position [n,size,size,3], info [n,2]) to write into.  No host sync."""
    return _mesh_atlas("mesh_atlas_raw_batch", verts, faces, counts, size, cell, background, out)


def glb_textured_bytes(nf, png_bytes, normals=True):
    """mp_glb_textured_bytes: the size of the textured binary glTF file of a mesh of ``nf`` faces whose image is a PNG
    of ``png_bytes`` bytes -- a closed form (include/monoport_hip.h); the empty file's 100 bytes for ``nf`` == 0."""
    for v in (nf, png_bytes):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("glb_textured_bytes: nf and png_bytes must be ints >= 0, got %r and %r" % (nf, png_bytes))
    return int(_lib.load().mp_glb_textured_bytes(int(nf), _glb_flags(normals, False), int(png_bytes)))


def glb_textured_max_bytes(max_faces, size, normals=True):
    """mp_glb_textured_max_bytes: what no textured file of a mesh of at most ``max_faces`` faces with an atlas of side
    ``size`` exceeds: ``glb_textured_bytes`` with ``png_max_bytes(size, size)``."""
    if isinstance(max_faces, bool) or not isinstance(max_faces, (int, np.integer)) or max_faces < 0:
        raise ValueError("glb_textured_max_bytes: max_faces must be an int >= 0, got %r" % (max_faces,))
    size, _ = atlas_params("glb_textured_max_bytes", size, ATLAS_MIN_CELL)
    return int(_lib.load().mp_glb_textured_max_bytes(int(max_faces), _glb_flags(normals, False), size))


def _mesh_glb_textured(who, verts, faces, counts, normals, colors, size, cell, png, png_info, b_min, b_max, capacity,
                       out, info):
    n, max_v, max_f, dev = _mesh_frames(who, verts, faces, counts)
    size, cell = atlas_params(who, size, cell)
    if colors is not None:
        raise ValueError("%s: COLOR_0 together with a texture: glTF multiplies the two; colors must be None" % who)
    if normals is not None:
        normals = _frame_rows(who, "normals", normals, n, (max_v, 3), torch.float32, dev)
    if (not isinstance(png, torch.Tensor) or png.dtype != torch.uint8 or png.dim() != 2 or png.shape[0] != n
            or not png.is_contiguous() or png.device != dev or png.shape[1] < PNG_MIN_BYTES):
        raise ValueError("%s: png must be a contiguous uint8 tensor [%d,png_capacity >= %d] on %s"
                         % (who, n, PNG_MIN_BYTES, dev))
    if (not isinstance(png_info, torch.Tensor) or png_info.dtype != torch.int32 or tuple(png_info.shape) != (n, 2)
            or not png_info.is_contiguous() or png_info.device != dev):
        raise ValueError("%s: png_info must be a contiguous int32 tensor [%d,2] on %s" % (who, n, dev))
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != n
                or not out.is_contiguous() or out.device != dev):
            raise ValueError("%s: out must be a contiguous uint8 tensor [%d,capacity] on %s" % (who, n, dev))
        if capacity is not None and int(capacity) != out.shape[1]:
            raise ValueError("%s: capacity %r against an out of %d bytes per mesh" % (who, capacity, out.shape[1]))
        capacity = int(out.shape[1])
    elif capacity is None:
        capacity = glb_textured_bytes(max_f, int(png.shape[1]), normals is not None)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < GLB_MIN_BYTES:
        raise ValueError("%s: capacity must be an int >= the empty file's %d bytes, got %r"
                         % (who, GLB_MIN_BYTES, capacity))
    if info is None:
        info = torch.empty((n, 2), dtype=torch.int32, device=dev)
    elif (not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or tuple(info.shape) != (n, 2)
          or not info.is_contiguous() or info.device != dev):
        raise ValueError("%s: info must be a contiguous int32 tensor [%d,2] on %s" % (who, n, dev))
    if out is None:
        out = torch.empty((n, int(capacity)), dtype=torch.uint8, device=dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_glb_textured_batch(
            ctx.handle, f1 - f0, _ptr_array(verts[f0:f1]), max_v, _ptr_array(faces[f0:f1]), max_f,
            _ptr_array(counts[f0:f1]), None if normals is None else _ptr_array(normals[f0:f1]), None, size, cell,
            _ptr(png[f0:f1]), int(png.shape[1]), _ptr(png_info[f0:f1]), _float3(b_min), _float3(b_max),
            _ptr(out[f0:f1]), int(capacity), _ptr(info[f0:f1]), _stream(verts[0])), "mp_mesh_glb_textured_batch")
    _keep_until_done(dev, verts, faces, counts, normals, [png, png_info])
    return out, info


def mesh_glb_textured_raw(verts, faces, counts, size, cell, png, png_info, normals=None, colors=None,
                          b_min=(-1, -1, -1), b_max=(1, 1, 1), capacity=None, out=None, info=None):
    """mp_mesh_glb_textured_batch with one frame: the binary glTF file of verts [max_v,3] f32, faces [max_f,3] int32,
    counts int32[2] on device as a NOT indexed primitive of 3 nf corner vertices -- 16-bit positions, with ``normals``
    [max_v,3] signed bytes, TEXCOORD_0 the closed form of the atlas (``size``, ``cell``) -- and, as its base colour
    texture inside the file, the PNG ``png`` uint8 [1,png_capacity] with ``png_info`` int32 [1,2] that
    ``picture_png_raw`` ("rgb8") made of the atlas's image -> (out uint8 [1,capacity], info int32 [1,2] = (bytes, code)):
    code 0 the file is ``out[0, :bytes]``; 1 nothing was written and ``bytes`` is the capacity it needs; 2 nothing was
    written: more faces than the atlas holds, or the PNG itself had overflowed.  ``colors`` must stay None: glTF
    multiplies COLOR_0 into the texture.  ``capacity``: None = the size at ``max_f`` faces and a PNG of
    ``png_capacity`` (never code 1).  Three launches; no host sync."""
    return _mesh_glb_textured("mesh_glb_textured_raw", [verts], [faces], [counts],
                              None if normals is None else [normals], colors, size, cell, png, png_info, b_min, b_max,
                              capacity, out, info)


def mesh_glb_textured_raw_batch(verts, faces, counts, size, cell, png, png_info, normals=None, colors=None,
                                b_min=(-1, -1, -1), b_max=(1, 1, 1), capacity=None, out=None, info=None):
    """mp_mesh_glb_textured_batch: the files of ``mesh_glb_textured_raw`` for lists of per-mesh device tensors of one
    capacity (``normals``: None, or one tensor per mesh; ``png`` [n,png_capacity], ``png_info`` [n,2]) in ONE set of
    three launches per MAX_FRAMES meshes -> (out uint8 [n,capacity], info int32 [n,2]), row f byte for byte what the
    per-mesh call gives.  No host sync."""
    return _mesh_glb_textured("mesh_glb_textured_raw_batch", verts, faces, counts, normals, colors, size, cell, png,
                              png_info, b_min, b_max, capacity, out, info)


def _mesh_points(who, verts, counts, out):
    n, max_v, _, dev = _mesh_frames(who, verts, None, counts)
    if out is None:
        pts = torch.zeros((n, 3, max_v), dtype=torch.float32, device=dev).unbind(0)
        count = torch.empty((n, 1), dtype=torch.int32, device=dev).unbind(0)
    else:
        pts = _frame_rows(who, "out[0] (points)", out[0], n, (3, max_v), torch.float32, dev)
        count = _frame_rows(who, "out[1] (count)", out[1], n, (1,), torch.int32, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_points_batch(
            ctx.handle, f1 - f0, _ptr_array(verts[f0:f1]), max_v, _ptr_array(counts[f0:f1]), _ptr_array(pts[f0:f1]),
            _ptr_array(count[f0:f1]), _stream(verts[0])), "mp_mesh_points_batch")
    return list(zip(pts, count))


def mesh_points_raw(verts, counts):
    """mp_mesh_points_batch with one frame: verts [max_v,3] -> (points [3,max_v], count int32[1] = min(counts[0],
    max_v)) on device, the operands of ``query_counted``.  No host sync."""
    return _mesh_points("mesh_points_raw", [verts], [counts], None)[0]


def mesh_points_raw_batch(verts, counts, out=None):
    """mp_mesh_points_batch: ``[mesh_points_raw(v, c) for v, c in zip(verts, counts)]`` in one launch per MAX_FRAMES
    meshes: per mesh (points [3,max_v], count int32[1]), views of two tensors (``out`` = (points [n,3,max_v],
    count [n,1]) if given; else the points start as zeros, as ``mesh_points_raw``'s).  No host sync."""
    return _mesh_points("mesh_points_raw_batch", verts, counts, out)


# MP_NEAREST_* (include/monoport_hip.h): which depth is in front
NEAREST_MODES = {"max": _lib.NEAREST_MAX_Z, "min": _lib.NEAREST_MIN_Z}
RENDER_MAX_SIZE = 4096  # mp_mesh_render: H, W in 1..4096


def _nearest(mode):
    if isinstance(mode, str):
        if mode not in NEAREST_MODES:
            raise ValueError("nearest must be one of %s, got %r" % (sorted(NEAREST_MODES), mode))
        return NEAREST_MODES[mode]
    mode = int(mode)
    if mode not in NEAREST_MODES.values():
        raise ValueError("unknown nearest mode %d" % mode)
    return mode


def _render_size(who, res):
    """``res`` (an int, or (H, W)) -> (H, W), each in 1..RENDER_MAX_SIZE."""
    h, w = (res, res) if isinstance(res, (int, np.integer)) else tuple(res)
    h, w = int(h), int(w)
    if not (1 <= h <= RENDER_MAX_SIZE and 1 <= w <= RENDER_MAX_SIZE):
        raise ValueError("%s: image size %d x %d outside 1..%d" % (who, h, w, RENDER_MAX_SIZE))
    return h, w


def _view_calibs(who, calibs):
    """The cameras of one mesh ([4,4], [3,4] or [n_views,>=3,4]; tensor or array) -> host float32 [n_views,12], the
    rows of [R|t].  The C side reads them on the host: a device tensor costs a copy back."""
    c = calibs.detach().cpu().numpy() if torch.is_tensor(calibs) else np.asarray(calibs)
    c = np.asarray(c, np.float32)
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or c.shape[0] < 1 or c.shape[1] < 3 or c.shape[2] != 4:
        raise ValueError("%s: calibs must be [4,4], [3,4] or [n_views,>=3,4], got %s" % (who, tuple(c.shape)))
    return np.ascontiguousarray(c[:, :3, :]).reshape(c.shape[0], 12)


def _render_clip(who, projection, near, perspective_correct):
    """The (near, flags) of mp_mesh_render_clip, or None for the unclipped call (``near`` None)."""
    if near is None:
        if perspective_correct:
            raise ValueError("%s: perspective_correct needs near (the clipped call interpolates)" % who)
        return None
    if _projection(projection) != PROJECTIONS["perspective"]:
        raise ValueError("%s: near clips perspective cameras only, not projection=%r" % (who, projection))
    near = float(near)
    if not (math.isfinite(near) and near > 0):
        raise ValueError("%s: near must be finite and > 0, got %r" % (who, near))
    return near, (_lib.RENDER_PERSPECTIVE_CORRECT if perspective_correct else 0)


RESOLVE_MAX_SAMPLES = 4  # mp_picture_resolve: samples in 2..4 (1: no resolve)


class Raster(collections.namedtuple("Raster", ["res", "projection", "nearest", "background", "near",
                                               "perspective_correct"])):
    """How the rasteriser draws whatever it is given, validated by ``raster``: the size (H, W), the projection, which
    depth is in front, what uncovered pixels hold, and the near plane with its interpolation (None and False: the
    unclipped call).  Every pass of one picture -- colours, positions, normals, transfer, the scene -- takes the same
    record.  ``samples`` (1, the default: none) is the anti-aliasing of the FINAL picture: the passes then run under
    ``fine_raster`` of the record, at ``samples`` times ``res``, and ``picture_resolve_batch`` brings the result back
    to ``res``.  It is the record's last field but not one of the tuple's: the record still unpacks and compares as
    the six arguments of a pass, which is all a pass reads."""

    def __new__(cls, res, projection, nearest, background, near, perspective_correct, samples=1):
        self = super().__new__(cls, res, projection, nearest, background, near, perspective_correct)
        self.samples = samples
        return self

    def _replace(self, samples=None, **kwargs):
        return type(self)(*super()._replace(**kwargs), samples=self.samples if samples is None else samples)

    def __repr__(self):
        return super().__repr__()[:-1] + ", samples=%r)" % self.samples


def _samples(who, samples):
    """``samples`` of a render call: an int in 1..RESOLVE_MAX_SAMPLES."""
    if (isinstance(samples, bool) or not isinstance(samples, (int, np.integer))
            or not 1 <= samples <= RESOLVE_MAX_SAMPLES):
        raise ValueError("%s: samples must be an int in 1..%d, got %r" % (who, RESOLVE_MAX_SAMPLES, samples))
    return int(samples)


def raster(who, res, projection="orthogonal", nearest="max", background=1.0, near=None, perspective_correct=False,
           samples=1):
    """The ``Raster`` of a render call's arguments, or the ValueError of the first one it refuses."""
    res = _render_size(who, res)
    _projection(projection), _nearest(nearest)
    if near is not None or perspective_correct:
        _render_clip(who, projection, near, perspective_correct)
    samples = _samples(who, samples)
    if samples * max(res) > RENDER_MAX_SIZE:
        raise ValueError("%s: samples = %d renders %d x %d at %d x %d, outside 1..%d"
                         % (who, samples, res[0], res[1], samples * res[0], samples * res[1], RENDER_MAX_SIZE))
    return Raster(res, projection, nearest, float(background), None if near is None else float(near),
                  bool(perspective_correct), samples)


def fine_raster(ras):
    """THE record under which every pass of a picture of ``ras`` runs: ``ras`` itself without anti-aliasing, else the
    same camera, plane and background at ``ras.samples`` times the size -- pixel (s i + a, s j + b) of it is sample
    (a, b) of pixel (i, j), because a vertex lands at (x + 1) * 0.5 * H pixels.  The near-plane clip and the 2^22 snap
    guard act at that size; a light's shadow map keeps its own."""
    if ras.samples == 1:
        return ras
    return ras._replace(res=(ras.samples * ras.res[0], ras.samples * ras.res[1]), samples=1)


def _mesh_render(who, verts, faces, counts, attrs, calibs, res, projection, nearest, channel_major, scale, bias, lo, hi,
                 background, out, capacity=None, near=None, perspective_correct=False):
    """What mesh_render_raw and mesh_render_raw_batch do: per mesh (image [n_views,H,W,3] or None, depth
    [n_views,H,W], face [n_views,H,W]), rows of three tensors.  ``capacity`` = (max_v, max_f): the meshes' tensors may
    then be shorter than it (each at least as long as its own counts say; row-major attributes only).  ``near``: None
    = mp_mesh_render_batch, else mp_mesh_render_clip_batch."""
    clip = None  # the unclipped call pays nothing for the keywords
    if near is not None or perspective_correct:
        clip = _render_clip(who, projection, near, perspective_correct)
    n = len(verts)
    if capacity is None:
        n, max_v, max_f, dev = _mesh_frames(who, verts, faces, counts)
    else:
        if n == 0 or len(faces) != n or len(counts) != n:
            raise ValueError("%s wants at least one mesh, and faces and counts for each" % who)
        for f in range(n):
            _mesh_buffers(verts[f], faces[f], counts[f])
        (max_v, max_f), dev = capacity, verts[0].device
        if channel_major or any(v.device != dev for v in verts):
            raise ValueError("%s: meshes of unequal capacity take row-major attributes on one device" % who)
    h, w = _render_size(who, res)
    proj, near_mode = _projection(projection), _nearest(nearest)
    cams = [_view_calibs(who, c) for c in _calib_list(calibs, n, who)]
    nv = cams[0].shape[0]
    if any(c.shape[0] != nv for c in cams):
        raise ValueError("%s: every mesh of a call takes the same number of views" % who)
    cams = np.stack(cams)  # [n, nv, 12]
    if attrs is not None:
        if len(attrs) != n:
            raise ValueError("%s: %d meshes, %d attribute buffers" % (who, n, len(attrs)))
        for f, a in enumerate(attrs):
            rows = verts[f].shape[0]
            if (a.dtype != torch.float32 or a.device != dev or not a.is_contiguous()
                    or tuple(a.shape) != ((3, rows) if channel_major else (rows, 3))):
                raise ValueError("%s: attr must be a contiguous float32 %s tensor on the mesh's device"
                                 % (who, "[3,V]" if channel_major else "[V,3]"))
    if out is None:
        image = None if attrs is None else torch.empty((n, nv, h, w, 3), dtype=torch.float32, device=dev).unbind(0)
        depth = torch.empty((n, nv, h, w), dtype=torch.float32, device=dev).unbind(0)
        face = torch.empty((n, nv, h, w), dtype=torch.int32, device=dev).unbind(0)
    else:
        image, depth, face = out
        if image is None and depth is None and face is None:
            raise ValueError("%s: out names no output" % who)
        if image is not None and attrs is None:
            raise ValueError("%s: an image needs attr" % who)
        if image is not None:
            image = _frame_rows(who, "out[0] (image)", image, n, (nv, h, w, 3), torch.float32, dev)
        if depth is not None:
            depth = _frame_rows(who, "out[1] (depth)", depth, n, (nv, h, w), torch.float32, dev)
        if face is not None:
            face = _frame_rows(who, "out[2] (face)", face, n, (nv, h, w), torch.int32, dev)
    ctx = get_context(dev)
    vstep = min(nv, MAX_FRAMES)  # image slots of a call: frames x views <= MAX_FRAMES
    fstep = MAX_FRAMES // vstep
    hold = None  # what an empty tensor (no address) passes in its place: never read
    if any(t.numel() == 0 for rows in (verts, faces, attrs or ()) for t in rows):
        hold = torch.zeros(4, dtype=torch.float32, device=dev)

    def ptrs(rows, f0, f1, v0=None):
        if rows is None:
            return None
        return _ptr_array([(hold if r.numel() == 0 else r) if v0 is None else r[v0:] for r in rows[f0:f1]])

    for v0 in range(0, nv, vstep):
        v1 = min(v0 + vstep, nv)
        for f0 in range(0, n, fstep):
            f1 = min(f0 + fstep, n)
            cal = np.ascontiguousarray(cams[f0:f1, v0:v1]).reshape(-1)
            args = (ctx.handle, f1 - f0, ptrs(verts, f0, f1), max_v, ptrs(faces, f0, f1), max_f, ptrs(counts, f0, f1),
                    ptrs(attrs, f0, f1), int(channel_major), v1 - v0, cal.ctypes.data_as(_lib._pf32), proj, near_mode,
                    h, w, float(scale), float(bias), float(lo), float(hi), float(background),
                    ptrs(image, f0, f1, v0), ptrs(depth, f0, f1, v0), ptrs(face, f0, f1, v0))
            if clip is None:
                ctx.check(ctx.lib.mp_mesh_render_batch(*args, _stream(verts[0])), "mp_mesh_render_batch")
            else:
                ctx.check(ctx.lib.mp_mesh_render_clip_batch(*args, clip[0], clip[1], _stream(verts[0])),
                          "mp_mesh_render_clip_batch")
    return [(None if image is None else image[f], None if depth is None else depth[f],
             None if face is None else face[f]) for f in range(n)]


def _attr_pass(who, verts, faces, counts, attrs, calibs, ras, out=None, capacity=None, channel_major=False,
               paint=(1.0, 0.0, -math.inf, math.inf)):
    """One pass of the rasteriser under the ``Raster`` ``ras``: ``_mesh_render`` of the row-major attributes ``attrs``
    (None: depth and face ids alone) as they are -- positions, normals, uv, transfer shades.  Only a subject's own shade
    names another ``paint`` (scale, bias, lo, hi) or ``channel_major`` attributes."""
    return _mesh_render(who, verts, faces, counts, attrs, calibs, ras.res, ras.projection, ras.nearest, channel_major,
                        *paint, ras.background, out, capacity=capacity, near=ras.near,
                        perspective_correct=ras.perspective_correct)


def mesh_render_raw(verts, faces, counts, attr, calibs, res, projection="orthogonal", nearest="max",
                    channel_major=False, scale=1.0, bias=0.0, lo=-math.inf, hi=math.inf, background=1.0, out=None,
                    near=None, perspective_correct=False):
    """mp_mesh_render_batch with one mesh: the z-buffered picture of verts [max_v,3] f32, faces [max_f,3] int32, counts
    int32[2] on device (as ``marching_cubes_raw`` returns them) under every camera of ``calibs`` ([4,4], [3,4] or
    [n_views, ...], read on the host) at ``res`` (an int or (H, W)), defined bit for bit in include/monoport_hip.h.
    ``attr``: None, or per-vertex values [max_v,3] ([3,max_v] with ``channel_major``) painted as clamp(a * scale + bias,
    lo, hi).  ``nearest``: "max" (the viewer sits at +z, what ``forward_vertices("front")`` sees) or "min" (depth is a
    distance).  Returns (image [n_views,H,W,3] or None without ``attr``, depth [n_views,H,W], face int32
    [n_views,H,W]); uncovered pixels hold ``background``, +0.0 and -1.  ``out``: (image, depth, face) buffers to write
    into; an entry None is an output not computed.  ``near`` None (the default): no clipping, screen-space
    interpolation (mp_mesh_render_batch).  ``near`` > 0 (``projection="perspective"`` only): mp_mesh_render_clip_batch
    -- faces are clipped at the plane zc = near, and with ``perspective_correct`` depth and attributes are interpolated
    perspective-correctly; on a mesh wholly in front of the plane, without ``perspective_correct``, the same bits as
    the unclipped call.  No side or far planes, no back-face culling.  No host sync."""
    return _mesh_render("mesh_render_raw", [verts], [faces], [counts], None if attr is None else [attr], [calibs], res,
                        projection, nearest, channel_major, scale, bias, lo, hi, background,
                        None if out is None else tuple(None if o is None else [o] for o in out), near=near,
                        perspective_correct=perspective_correct)[0]


def mesh_render_raw_batch(verts, faces, counts, attrs, calibs, res, projection="orthogonal", nearest="max",
                          channel_major=False, scale=1.0, bias=0.0, lo=-math.inf, hi=math.inf, background=1.0, out=None,
                          near=None, perspective_correct=False):
    """mp_mesh_render_batch: ``[mesh_render_raw(v, f, c, a, cal, res, ...) for ...]`` (lists of per-mesh device tensors
    of one capacity, ``attrs`` None or a list, ``calibs`` one camera set per mesh, all of one n_views) in ONE set of
    launches per MAX_FRAMES images (meshes x views); bit for bit what the per-mesh call gives.  A mesh whose counts
    read 0 gives pure background.  ``out``: (image [n,n_views,H,W,3], depth [n,n_views,H,W], face [n,n_views,H,W])
    to write into, entries None = not computed.  ``near`` / ``perspective_correct`` as in ``mesh_render_raw``
    (mp_mesh_render_clip_batch).  No host sync."""
    return _mesh_render("mesh_render_raw_batch", verts, faces, counts, attrs, calibs, res, projection, nearest,
                        channel_major, scale, bias, lo, hi, background, out, near=near,
                        perspective_correct=perspective_correct)


def _picture_points(who, face_ids, positions, capacity, out):
    n = len(face_ids)
    if n == 0 or len(positions) != n:
        raise ValueError("%s: %d face-id pictures, %d position pictures" % (who, n, len(positions)))
    dev, npix = face_ids[0].device, face_ids[0].numel()
    for f, p in zip(face_ids, positions):
        if (f.dtype != torch.int32 or p.dtype != torch.float32 or f.numel() != npix or p.numel() != 3 * npix
                or f.device != dev or p.device != dev or not f.is_contiguous() or not p.is_contiguous()):
            raise ValueError("%s: per frame a contiguous int32 picture of %d face ids and a float32 one of positions "
                             "[..., 3], on one device" % (who, npix))
    cap = npix if capacity is None else int(capacity)
    if npix < 1 or cap < 1:
        raise ValueError("%s: at least one pixel and a capacity >= 1, got %d and %d" % (who, npix, cap))
    if out is None:
        points = torch.zeros((n, 3, cap), dtype=torch.float32, device=dev).unbind(0)
        pixels = torch.zeros((n, cap), dtype=torch.int32, device=dev).unbind(0)
        count = torch.empty((n, 2), dtype=torch.int32, device=dev).unbind(0)
    else:
        points = _frame_rows(who, "out[0] (points)", out[0], n, (3, cap), torch.float32, dev)
        pixels = _frame_rows(who, "out[1] (pixels)", out[1], n, (cap,), torch.int32, dev)
        count = _frame_rows(who, "out[2] (count)", out[2], n, (2,), torch.int32, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_picture_points_batch(
            ctx.handle, f1 - f0, _ptr_array(face_ids[f0:f1]), _ptr_array(positions[f0:f1]), npix, cap,
            _ptr_array(points[f0:f1]), _ptr_array(pixels[f0:f1]), _ptr_array(count[f0:f1]), _stream(face_ids[0])),
            "mp_picture_points_batch")
    return list(zip(points, pixels, count))


def picture_points(face_id, position, capacity=None, out=None):
    """mp_picture_points_batch with one frame: the covered pixels (face_id >= 0) of a frame's pictures -- face_id int32
    [...] of L pixels as ``mesh_render_raw`` wrote it, position float32 [..., 3] its image for ``attr = verts`` -- in
    ascending pixel order, bit for bit as include/monoport_hip.h defines it: (points [3,capacity] float32, the operand
    of ``query_counted``; pixels [capacity] int32; count int32[2] = (entries written, covered pixels)) on the device.
    ``capacity``: L unless given; ``count[1] > capacity`` tells a truncated list.  ``out``: (points, pixels, count)
    buffers to write into; fresh ones start as zeros.  No host sync."""
    return _picture_points("picture_points", [face_id], [position], capacity,
                           None if out is None else tuple([o] for o in out))[0]


def picture_points_batch(face_ids, positions, capacity=None, out=None):
    """mp_picture_points_batch: ``[picture_points(f, p, capacity) for f, p in zip(face_ids, positions)]`` (pictures of
    one size) in one set of three launches per MAX_FRAMES frames, the same bits.  ``out``: (points [n,3,capacity],
    pixels [n,capacity], count [n,2]) to write into.  No host sync."""
    return _picture_points("picture_points_batch", face_ids, positions, capacity, out)


def _picture_paint(who, values, pixels, counts, images, scale, bias, lo, hi):
    n = len(values)
    if n == 0 or len(pixels) != n or len(counts) != n or len(images) != n:
        raise ValueError("%s: %d value sets, %d pixel lists, %d counts, %d images"
                         % (who, n, len(pixels), len(counts), len(images)))
    dev, cap, size = values[0].device, pixels[0].numel(), images[0].numel()
    for v, p, k, im in zip(values, pixels, counts, images):
        if (tuple(v.shape) != (3, cap) or v.dtype != torch.float32 or p.numel() != cap or p.dtype != torch.int32
                or k.dtype != torch.int32 or k.numel() < 1 or im.dtype != torch.float32 or im.numel() != size
                or not (v.is_contiguous() and p.is_contiguous() and im.is_contiguous())
                or any(t.device != dev for t in (p, k, im))):
            raise ValueError("%s: per frame contiguous values float32 [3,%d], pixels int32 [%d], an int32 count and a "
                             "float32 image [..., 3] of one size, on one device" % (who, cap, cap))
    if cap < 1 or size < 3 or size % 3:
        raise ValueError("%s: a capacity >= 1 and images [..., 3], got %d and %d floats" % (who, cap, size))
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_picture_paint_batch(
            ctx.handle, f1 - f0, _ptr_array(values[f0:f1]), _ptr_array(pixels[f0:f1]), _ptr_array(counts[f0:f1]), cap,
            size // 3, float(scale), float(bias), float(lo), float(hi), _ptr_array(images[f0:f1]), _stream(values[0])),
            "mp_picture_paint_batch")
    return list(images)


def picture_paint(values, pixels, count, n_pixels=None, scale=0.5, bias=0.5, lo=-math.inf, hi=math.inf, background=1.0,
                  out=None):
    """mp_picture_paint_batch with one frame: out[pixels[k], :] = clamp(values[:, k] * scale + bias, lo, hi) for the
    first count[0] entries of a list of ``picture_points`` (values float32 [3,capacity], as the counted queries write
    them); an index outside the image is skipped and no other pixel is touched.  ``out``: the image float32 [..., 3] to
    paint into, which may be the buffer the positions were read from; None: a fresh [n_pixels,3] image of
    ``background``.  Returns the image.  No host sync."""
    if out is None:
        if n_pixels is None:
            raise ValueError("picture_paint: without out= it needs n_pixels")
        out = torch.full((int(n_pixels), 3), float(background), dtype=torch.float32, device=values.device)
    return _picture_paint("picture_paint", [values], [pixels], [count], [out], scale, bias, lo, hi)[0]


def picture_paint_batch(values, pixels, counts, n_pixels=None, scale=0.5, bias=0.5, lo=-math.inf, hi=math.inf,
                        background=1.0, out=None):
    """mp_picture_paint_batch: ``[picture_paint(v, p, c, ..., out=o) for ...]`` (lists of one capacity, images of one
    size) in one launch per MAX_FRAMES frames, the same bits.  ``out``: the images (a list, or [n, ..., 3]); None:
    fresh [n_pixels,3] images of ``background``.  No host sync."""
    if out is None:
        if n_pixels is None:
            raise ValueError("picture_paint_batch: without out= it needs n_pixels")
        out = torch.full((len(values), int(n_pixels), 3), float(background), dtype=torch.float32,
                         device=values[0].device)
    return _picture_paint("picture_paint_batch", values, pixels, counts, list(out), scale, bias, lo, hi)


def render_netc_batch(who, verts, faces, counts, calibs, ras, query, out=None, lists=None, capacity=None,
                      positions_hook=None):
    """Pictures coloured per pixel (deferred shading), no host value in between: (1) the rasteriser with ``attr =
    verts`` -- a picture of world-space surface positions -- under the pictures' own cameras and ``Raster`` ``ras``;
    (2) ``picture_points_batch`` over each mesh's views as one flat picture (capacity = its
    pixels: nothing truncates); (3) ``query(points, counts)``: the caller's counted colour query over all meshes (lists
    of [3,L] points and int32 counts -> list of raw predictions [3,L]), under the calibrations and projections its maps
    were made under, chunked by the caller to the query's frame limits; (4) ``picture_paint_batch`` with (0.5, 0.5,
    -inf, inf) into the picture the positions came from.  Returns what ``_mesh_render`` does: per mesh (image
    [n_views,H,W,3] = query * 0.5 + 0.5 at covered pixels and ``background`` elsewhere, depth, face).  ``out``: (image,
    depth or None, face) buffers; ``lists``: (points [n,3,L], pixels [n,L], count [n,2]) buffers.  ``capacity``: as in
    ``_mesh_render``.  ``positions_hook(positions, face_ids)``: called between (1) and (4), while the images still
    hold the positions -- what a self-shadow reads (``self_shades``), so that no second position pass is needed."""
    if out is not None and (out[0] is None or out[2] is None):
        raise ValueError("%s: a picture coloured per pixel needs the image and the face ids" % who)
    raws = _attr_pass(who, verts, faces, counts, list(verts), calibs, ras, out, capacity)
    images, face_ids = [r[0] for r in raws], [r[2] for r in raws]
    if positions_hook is not None:
        positions_hook(images, face_ids)
    paint_netc(who, face_ids, images, query, lists)
    return raws


def paint_netc(who, face_ids, images, query, lists=None):
    """Steps (2) to (4) of ``render_netc_batch`` on G-buffers that are already there -- per frame a face-id picture and
    an image [..., 3] that holds the world positions of its covered pixels, from the rasteriser (screen space) or from
    ``mesh_atlas_raw_batch`` (texture space): the covered pixels' point lists, ``query(points, counts)``, and the paint
    with (0.5, 0.5, -inf, inf) into ``images``, in place.  Returns ``images``."""
    found = _picture_points(who, face_ids, images, None, lists)
    preds = query([f[0] for f in found], [f[2] for f in found])
    _picture_paint(who, list(preds), [f[1] for f in found], [f[2] for f in found], images, 0.5, 0.5, -math.inf, math.inf)
    return images


# MP_WRAP_* / MP_COMPOSITE_* (include/monoport_hip.h)
WRAP_MODES = {"repeat": _lib.WRAP_REPEAT, "clamp": _lib.WRAP_CLAMP}
COMPOSITE_MODES = {"over": _lib.COMPOSITE_OVER, "depth": _lib.COMPOSITE_DEPTH}
TEXTURE_MAX_SIZE = 8192  # mp_texture_mips: ht, wt in 1..8192
TEXTURE_MAX_LEVELS = 14


def _named_mode(who, what, table, mode):
    if isinstance(mode, str) and mode in table:
        return table[mode]
    if not isinstance(mode, (str, bool)) and isinstance(mode, (int, np.integer)) and int(mode) in table.values():
        return int(mode)
    raise ValueError("%s: %s must be one of %s, got %r" % (who, what, sorted(table), mode))


def texture_levels(ht, wt):
    """The levels of the full mip chain of a ht x wt texture, down to 1 x 1."""
    return max(int(ht), int(wt)).bit_length()


def texture_pyramid_floats(ht, wt, levels=None):
    """mp_texture_pyramid_floats: the float count of a ht x wt texture's pyramid of ``levels`` levels (None: the full
    chain).  Host only."""
    ht, wt = int(ht), int(wt)
    if not (1 <= ht <= TEXTURE_MAX_SIZE and 1 <= wt <= TEXTURE_MAX_SIZE):
        raise ValueError("texture size %d x %d outside 1..%d" % (ht, wt, TEXTURE_MAX_SIZE))
    levels = texture_levels(ht, wt) if levels is None else int(levels)
    if not 1 <= levels <= min(TEXTURE_MAX_LEVELS, texture_levels(ht, wt)):
        raise ValueError("levels must be in 1..%d for a %d x %d texture, got %d"
                         % (min(TEXTURE_MAX_LEVELS, texture_levels(ht, wt)), ht, wt, levels))
    return int(_lib.load().mp_texture_pyramid_floats(ht, wt, levels))


def texture_mips(tex, levels=None, out=None):
    """mp_texture_mips: the mip pyramid of ``tex`` (float32 [Ht,Wt,3] on the device) as one flat float32 tensor, level 0
    (a copy of ``tex``) first, each level the 2x2 box of the one below, bit for bit as include/monoport_hip.h defines
    it.  ``levels``: None = the full chain down to 1 x 1.  Returns (pyramid, levels).  A set-up call: one launch per
    level.  No host sync."""
    if tex.dtype != torch.float32 or tex.dim() != 3 or tex.shape[2] != 3 or not tex.is_contiguous():
        raise ValueError("texture_mips: tex must be a contiguous float32 [Ht,Wt,3] tensor")
    ht, wt = int(tex.shape[0]), int(tex.shape[1])
    levels = texture_levels(ht, wt) if levels is None else int(levels)
    n = texture_pyramid_floats(ht, wt, levels)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=tex.device)
    elif out.dtype != torch.float32 or out.numel() != n or out.device != tex.device or not out.is_contiguous():
        raise ValueError("texture_mips: out must be a contiguous float32 tensor of %d elements on %s" % (n, tex.device))
    ctx = get_context(tex.device)
    ctx.check(ctx.lib.mp_texture_mips(ctx.handle, _ptr(tex), ht, wt, levels, _ptr(out), _stream(tex)), "mp_texture_mips")
    return out, levels


def _flat_pictures(who, what, rows, n, dtype, per_pixel, npix, dev):
    rows = list(rows)
    if len(rows) != n or any(r.dtype != dtype or r.numel() != per_pixel * npix or r.device != dev
                             or not r.is_contiguous() for r in rows):
        raise ValueError("%s: %s must be %d contiguous %s pictures of %d pixels on %s"
                         % (who, what, n, str(dtype).replace("torch.", ""), npix, dev))
    return rows


def picture_texture_batch(uvs, face_ids, pyramid, tex_size, levels, wrap="repeat", scale=1.0, bias=0.0, lo=-math.inf,
                          hi=math.inf, background=1.0, out=None, who="picture_texture_batch"):
    """mp_picture_texture_batch: per frame the textured picture of a UV picture.  ``uvs``: float32 [n_views,H,W,3] per
    frame (channels u, v, unused: the rasteriser's image for ``attr = (u, v, 0)``), ``face_ids`` its int32
    [n_views,H,W]; ``pyramid``, ``levels`` as ``texture_mips`` returns them for a texture of ``tex_size`` = (Ht, Wt).
    A covered pixel (face id >= 0, finite uv within +-65536) takes the nearest mip level for its uv steps to its
    neighbours, a bilinear lookup there (``wrap``: "repeat" or "clamp") and clamp(value * scale + bias, lo, hi); every
    other pixel takes ``background``.  Defined bit for bit in include/monoport_hip.h.  ``out``: the images to write
    (not the UV pictures: a pixel reads its neighbours); None: fresh ones.  One launch per MAX_FRAMES frames; no host
    sync.  Returns the list of images."""
    n = len(uvs)
    if n == 0 or uvs[0].dim() != 4 or uvs[0].shape[3] != 3:
        raise ValueError("%s: at least one UV picture [n_views,H,W,3]" % who)
    nv, h, w = (int(s) for s in uvs[0].shape[:3])
    dev, npix = uvs[0].device, nv * h * w
    uvs = _flat_pictures(who, "uvs", uvs, n, torch.float32, 3, npix, dev)
    face_ids = _flat_pictures(who, "face_ids", face_ids, n, torch.int32, 1, npix, dev)
    ht, wt = int(tex_size[0]), int(tex_size[1])
    if (pyramid.dtype != torch.float32 or pyramid.device != dev or not pyramid.is_contiguous()
            or pyramid.numel() != texture_pyramid_floats(ht, wt, levels)):
        raise ValueError("%s: pyramid must be the contiguous float32 pyramid of a %d x %d texture with %d levels on %s"
                         % (who, ht, wt, levels, dev))
    wrap = _named_mode(who, "wrap", WRAP_MODES, wrap)
    if out is None:
        out = torch.empty((n, nv, h, w, 3), dtype=torch.float32, device=dev).unbind(0)
    else:
        out = _flat_pictures(who, "out", out, n, torch.float32, 3, npix, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_picture_texture_batch(
            ctx.handle, f1 - f0, _ptr_array(uvs[f0:f1]), _ptr_array(face_ids[f0:f1]), nv, h, w, _ptr(pyramid), ht, wt,
            int(levels), wrap, float(scale), float(bias), float(lo), float(hi), float(background),
            _ptr_array(out[f0:f1]), _stream(uvs[0])), "mp_picture_texture_batch")
    return list(out)


def picture_composite_batch(fronts, backs, mode="depth", nearest="max", background=1.0, out=None,
                            who="picture_composite_batch"):
    """mp_picture_composite_batch: per frame the composite of ``fronts[f]`` over ``backs[f]``, each (image float32
    [...,3], depth float32 [...], face int32 [...]) of one size.  The front shows where it is covered (face >= 0) and
    the back is not, or ``mode`` is "over", or -- ``mode="depth"`` -- the back is not strictly nearer under ``nearest``
    ("max" / "min", as the renders take it); else the back shows where it is covered; else ``background`` and depth
    +0.0.  ``out``: (images, depths or None, masks or None) to write; the images / depths may be the fronts' own (the
    composite in place).  None: fresh ones.  Returns per frame (image, depth, mask uint8: 0 neither, 1 back, 2 front).
    One launch per MAX_FRAMES frames; no host sync."""
    n = len(fronts)
    if n == 0 or len(backs) != n:
        raise ValueError("%s: %d front pictures, %d back pictures" % (who, n, len(backs)))
    dev, npix = fronts[0][2].device, fronts[0][2].numel()
    if npix < 1:
        raise ValueError("%s: at least one pixel" % who)
    cols = []
    for what, pics in (("fronts", fronts), ("backs", backs)):
        if any(p is None or len(p) < 3 or p[0] is None for p in pics):
            raise ValueError("%s: every picture of %s needs an image, a depth and face ids" % (who, what))
        cols.append(_flat_pictures(who, what + " (image)", [p[0] for p in pics], n, torch.float32, 3, npix, dev))
        cols.append(_flat_pictures(who, what + " (depth)", [p[1] for p in pics], n, torch.float32, 1, npix, dev))
        cols.append(_flat_pictures(who, what + " (face)", [p[2] for p in pics], n, torch.int32, 1, npix, dev))
    mode = _named_mode(who, "composite", COMPOSITE_MODES, mode)
    near_mode = _nearest(nearest)
    shape = tuple(fronts[0][2].shape)
    if out is None:
        image = torch.empty((n,) + shape + (3,), dtype=torch.float32, device=dev).unbind(0)
        depth = torch.empty((n,) + shape, dtype=torch.float32, device=dev).unbind(0)
        mask = torch.empty((n,) + shape, dtype=torch.uint8, device=dev).unbind(0)
    else:
        image = _flat_pictures(who, "out[0] (image)", out[0], n, torch.float32, 3, npix, dev)
        depth = None if out[1] is None else _flat_pictures(who, "out[1] (depth)", out[1], n, torch.float32, 1, npix, dev)
        mask = None if out[2] is None else _flat_pictures(who, "out[2] (mask)", out[2], n, torch.uint8, 1, npix, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_picture_composite_batch(
            ctx.handle, f1 - f0, *[_ptr_array(c[f0:f1]) for c in cols], npix, mode, near_mode, float(background),
            _ptr_array(image[f0:f1]), None if depth is None else _ptr_array(depth[f0:f1]),
            None if mask is None else _ptr_array(mask[f0:f1]), _stream(fronts[0][2])), "mp_picture_composite_batch")
    return [(image[f], None if depth is None else depth[f], None if mask is None else mask[f]) for f in range(n)]


def picture_resolve_batch(images, depths, faces, masks, samples, nearest="max", out=None,
                          who="picture_resolve_batch"):
    """mp_picture_resolve_batch: per frame the final picture of one rendered at ``samples`` (2..4) times its size.
    ``images`` (float32 [n_views,s H,s W,3] per frame), ``depths`` (float32 [n_views,s H,s W]), ``faces`` (int32, the
    same) and ``masks`` (uint8, the same: a composite's 0 / 1 / 2): each a list with one tensor per frame, or None; a
    frame without a leading n_views ([s H,s W,...]) is one view.  Per output pixel over its s x s samples: the image is
    their mean (sequential f32 additions in row-major sample order, one division), ``coverage`` the fraction that is
    the subject's (mask == 2, or face >= 0 without masks), depth and face those of the nearest sample that shows
    (mask != 0, or face >= 0) under ``nearest`` ("max" / "min", as the renders take it; +0.0 and -1 where none does),
    the mask the largest.  Defined bit for bit in include/monoport_hip.h.  Returns per frame (image, depth, face, mask,
    coverage), each shaped as its frame's input at 1 / s the size, None for an output whose input is missing (image
    needs ``images``; depth and face need ``depths`` and ``faces``; mask needs ``masks``; coverage needs ``masks`` or
    ``faces``).  ``out``: None (fresh tensors for every output that can be made), or (images, depths, faces, masks,
    coverages) to write into, each a list / [n, ...] tensor or None = not computed.  One launch per MAX_FRAMES
    pictures (frames x views); no host sync."""
    if (isinstance(samples, bool) or not isinstance(samples, (int, np.integer))
            or not 2 <= samples <= RESOLVE_MAX_SAMPLES):
        raise ValueError("%s: samples must be an int in 2..%d, got %r" % (who, RESOLVE_MAX_SAMPLES, samples))
    s = int(samples)
    near_mode = _nearest(nearest)
    planes = [None if p is None else list(p) for p in (images, depths, faces, masks)]
    lead = next((p for p in planes[1:] + planes[:1] if p is not None), None)
    if lead is None or len(lead) == 0:
        raise ValueError("%s: at least one frame of images, depths, faces or masks" % who)
    n, dev = len(lead), lead[0].device
    shape = tuple(lead[0].shape[:-1]) if lead is planes[0] else tuple(lead[0].shape)
    if len(shape) not in (2, 3) or shape[-2] % s or shape[-1] % s or shape[-2] < s or shape[-1] < s:
        raise ValueError("%s: pictures [n_views,s H,s W] or [s H,s W] with s = %d, got %s" % (who, s, shape))
    nv, (h, w) = (shape[0] if len(shape) == 3 else 1), (shape[-2] // s, shape[-1] // s)
    if s * h > RENDER_MAX_SIZE or s * w > RENDER_MAX_SIZE:
        raise ValueError("%s: image size %d x %d outside 1..%d" % (who, s * h, s * w, RENDER_MAX_SIZE))
    fine, small = nv * s * h * s * w, shape[:-2] + (h, w)
    kinds = (("images", torch.float32, 3), ("depths", torch.float32, 1), ("faces", torch.int32, 1),
             ("masks", torch.uint8, 1))
    for k, (what, dtype, per) in enumerate(kinds):
        if planes[k] is not None:
            planes[k] = _flat_pictures(who, what, planes[k], n, dtype, per, fine, dev)
    have = (planes[0] is not None, planes[1] is not None and planes[2] is not None,
            planes[1] is not None and planes[2] is not None, planes[3] is not None,
            planes[3] is not None or planes[2] is not None)
    outs_of = (("image", torch.float32, 3), ("depth", torch.float32, 1), ("face", torch.int32, 1),
               ("mask", torch.uint8, 1), ("coverage", torch.float32, 1))
    if out is None:
        outs = [torch.empty((n,) + small + ((3,) if per == 3 else ()), dtype=dtype, device=dev).unbind(0) if ok else None
                for ok, (_, dtype, per) in zip(have, outs_of)]
    else:
        if len(out) != 5:
            raise ValueError("%s: out is (images, depths, faces, masks, coverages), entries None = not computed" % who)
        outs = []
        for k, (ok, (what, dtype, per)) in enumerate(zip(have, outs_of)):
            if out[k] is not None and not ok:
                raise ValueError("%s: out[%d] (%s) needs its input" % (who, k, what))
            outs.append(None if out[k] is None else
                        _flat_pictures(who, "out[%d] (%s)" % (k, what), out[k], n, dtype, per, nv * h * w, dev))
    if all(o is None for o in outs):
        raise ValueError("%s: out names no output" % who)
    ctx = get_context(dev)
    vstep = min(nv, MAX_FRAMES)  # pictures of a call: frames x views <= MAX_FRAMES
    fstep = MAX_FRAMES // vstep

    def ptrs(rows, f0, f1, v0, per_view):
        if rows is None:
            return None
        return _ptr_array([r.reshape(-1)[v0 * per_view:] for r in rows[f0:f1]])

    for v0 in range(0, nv, vstep):
        v1 = min(v0 + vstep, nv)
        for f0 in range(0, n, fstep):
            f1 = min(f0 + fstep, n)
            ctx.check(ctx.lib.mp_picture_resolve_batch(
                ctx.handle, f1 - f0, v1 - v0,
                *[ptrs(p, f0, f1, v0, s * h * s * w * per) for p, (_, _, per) in zip(planes, kinds)],
                h, w, s, near_mode,
                *[ptrs(o, f0, f1, v0, h * w * per) for o, (_, _, per) in zip(outs, outs_of)],
                _stream(lead[0])), "mp_picture_resolve_batch")
    return [tuple(None if o is None else o[f].view(small + ((3,) if per == 3 else ()))
                  for o, (_, _, per) in zip(outs, outs_of)) for f in range(n)]


SHADOW_MAX_RADIUS = 3  # mp_picture_shadow: radius in 0..3
SHADOW_MAX_SIZE = 4096  # its map: Hs, Ws in 1..4096


def shadow_params(who, bias, radius, strength):
    """(bias, radius, strength) of mp_picture_shadow as (float, int, float), or the ValueError of a value it refuses."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= SHADOW_MAX_RADIUS:
        raise ValueError("%s: radius must be an int in 0..%d, got %r" % (who, SHADOW_MAX_RADIUS, radius))
    bias, strength = float(bias), float(strength)
    if not (math.isfinite(bias) and bias >= 0):
        raise ValueError("%s: bias must be finite and >= 0, got %r" % (who, bias))
    if not 0.0 <= strength <= 1.0:
        raise ValueError("%s: strength must be in [0, 1], got %r" % (who, strength))
    return bias, int(radius), strength


def picture_shadow_batch(images, positions, face_ids, map_depths, map_faces, light_calibs, projection="orthogonal",
                         nearest="min", bias=0.0, radius=1, strength=0.6, out=None, with_shade=False,
                         who="picture_shadow_batch"):
    """mp_picture_shadow_batch: per frame the shadow that a shadow map casts on a picture.  ``positions``: float32
    [...,3] per frame, the world-space point every pixel shows (the rasteriser's image for ``attr = verts``, paint (1, 0,
    -inf, inf)), ``face_ids`` its int32 [...]; ``images``: the float32 [...,3] pictures to darken, or None (the shade
    alone).  ``map_depths`` / ``map_faces``: per frame the float32 / int32 [Hs,Ws] that the rasteriser wrote for the
    caster under the light (``nearest`` as it was rendered with); ``light_calibs``: one [4,4] / [3,4] for all frames, or
    one per frame (read on the host); ``projection`` the light's.  A covered pixel whose point lies behind the map's
    surface by more than ``bias`` -- over a (2 radius + 1)^2 box of bilinear lookups -- has shade 1, and the image is
    multiplied by 1 - strength * shade; a pixel with shade 0 keeps its bits.  Defined bit for bit in
    include/monoport_hip.h.  ``out``: (images or None, shades or None) to write; the images may be ``images`` themselves
    (in place).  None: fresh images (where ``images`` is given) and, with ``with_shade`` or without images, fresh
    shades.  Returns per frame (image or None, shade or None).  One launch per MAX_FRAMES frames; no host sync."""
    n = len(positions)
    if n == 0 or positions[0].dim() < 2 or positions[0].shape[-1] != 3:
        raise ValueError("%s: at least one position picture [...,3]" % who)
    shape = tuple(positions[0].shape[:-1])
    dev, npix = positions[0].device, positions[0].numel() // 3
    if npix < 1:
        raise ValueError("%s: at least one pixel" % who)
    positions = _flat_pictures(who, "positions", positions, n, torch.float32, 3, npix, dev)
    face_ids = _flat_pictures(who, "face_ids", face_ids, n, torch.int32, 1, npix, dev)
    if images is not None:
        images = _flat_pictures(who, "images", images, n, torch.float32, 3, npix, dev)
    map_depths, map_faces = list(map_depths), list(map_faces)
    if len(map_depths) != n or len(map_faces) != n or map_depths[0].dim() != 2:
        raise ValueError("%s: per frame a shadow map [Hs,Ws] of depths and one of face ids" % who)
    hs, ws = (int(s) for s in map_depths[0].shape)
    if not (1 <= hs <= SHADOW_MAX_SIZE and 1 <= ws <= SHADOW_MAX_SIZE):
        raise ValueError("%s: shadow map size %d x %d outside 1..%d" % (who, hs, ws, SHADOW_MAX_SIZE))
    map_depths = _frame_rows(who, "map_depths", map_depths, n, (hs, ws), torch.float32, dev)
    map_faces = _frame_rows(who, "map_faces", map_faces, n, (hs, ws), torch.int32, dev)
    proj, near_mode = _projection(projection), _nearest(nearest)
    bias, radius, strength = shadow_params(who, bias, radius, strength)
    lights = list(light_calibs) if isinstance(light_calibs, (list, tuple)) else [light_calibs] * n
    if len(lights) != n:
        raise ValueError("%s: %d frames, %d light calibrations" % (who, n, len(lights)))
    cal = np.stack([_view_calibs(who, c) for c in lights])
    if cal.shape[1] != 1:
        raise ValueError("%s: one light per frame" % who)
    cal = np.ascontiguousarray(cal.reshape(n, 12))
    if out is None:
        image = None if images is None else torch.empty((n,) + shape + (3,), dtype=torch.float32, device=dev).unbind(0)
        shade = (torch.empty((n,) + shape, dtype=torch.float32, device=dev).unbind(0)
                 if (with_shade or images is None) else None)
    else:
        image = None if out[0] is None else _flat_pictures(who, "out[0] (image)", out[0], n, torch.float32, 3, npix, dev)
        shade = None if out[1] is None else _flat_pictures(who, "out[1] (shade)", out[1], n, torch.float32, 1, npix, dev)
    if image is None and shade is None:
        raise ValueError("%s: out names no output" % who)
    if (image is None) != (images is None):
        raise ValueError("%s: an image is written exactly where images are given" % who)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_picture_shadow_batch(
            ctx.handle, f1 - f0, None if images is None else _ptr_array(images[f0:f1]), _ptr_array(positions[f0:f1]),
            _ptr_array(face_ids[f0:f1]), npix, _ptr_array(map_depths[f0:f1]), _ptr_array(map_faces[f0:f1]), hs, ws,
            np.ascontiguousarray(cal[f0:f1]).ctypes.data_as(_lib._pf32), proj, near_mode, bias, radius, strength,
            None if image is None else _ptr_array(image[f0:f1]), None if shade is None else _ptr_array(shade[f0:f1]),
            _stream(positions[0])), "mp_picture_shadow_batch")
    return [(None if image is None else image[f], None if shade is None else shade[f]) for f in range(n)]


def _finite_floats(who, what, value, shape):
    try:
        a = np.array(value.detach().cpu().numpy() if torch.is_tensor(value) else value, dtype=np.float32)
    except (TypeError, ValueError):
        a = None
    if a is None or a.shape != shape or not np.isfinite(a).all():
        raise ValueError("%s: %s must be finite float values of shape %s, got %r" % (who, what, shape, value))
    return np.ascontiguousarray(a)


def light_params(who, sh, direct=None, gamma=1.0, albedo_rgb=None):
    """(sh [9,3], direct_dir [3], direct_rgb [3], gamma, albedo_rgb [3] or None) of mp_picture_light as float32 host
    values, or the ValueError of a value it refuses.  ``direct``: None (no direct light: zeros), or a (direction the
    light travels, rgb) pair, passed on as given (the caller normalises the direction)."""
    sh = _finite_floats(who, "sh", sh, (9, 3))
    if direct is None:
        ddir, drgb = np.zeros(3, np.float32), np.zeros(3, np.float32)
    else:
        try:
            ddir, drgb = direct
        except (TypeError, ValueError):
            raise ValueError("%s: direct must be None or a (direction, rgb) pair, got %r" % (who, direct)) from None
        ddir = _finite_floats(who, "direct's direction", ddir, (3,))
        drgb = _finite_floats(who, "direct's rgb", drgb, (3,))
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)):
        raise ValueError("%s: gamma must be a number, got %r" % (who, gamma))
    gamma = float(np.float32(gamma))
    if not (math.isfinite(gamma) and gamma > 0):
        raise ValueError("%s: gamma must be finite and > 0, got %r" % (who, gamma))
    if albedo_rgb is not None:
        albedo_rgb = _finite_floats(who, "albedo", albedo_rgb, (3,))
    return sh, ddir, drgb, gamma, albedo_rgb


def normal_mats_of(who, calibs):
    """The [n_views,3,3] float32 normal matrices of one camera set: the 3x3 of each view's [R|t], which
    ``picture_light_batch`` applies to the unit normal and normalises again (so a scaled rotation is a rotation)."""
    return np.ascontiguousarray(_view_calibs(who, calibs).reshape(-1, 3, 4)[:, :, :3])


def picture_light_batch(normals, face_ids, albedos, sh, direct=None, gamma=1.0, normal_mats=None, visibilities=None,
                        albedo_rgb=None, n_views=None, background=1.0, out=None, with_shading=False,
                        who="picture_light_batch"):
    """mp_picture_light_batch: per frame the lit picture of a normal picture.  ``normals``: float32 [...,3] per frame,
    the rasteriser's image for ``attr = mesh normals`` with the paint (1, 0, -inf, inf), ``face_ids`` its int32 [...];
    ``albedos``: the float32 [...,3] pictures to light, or None with a constant ``albedo_rgb`` (r, g, b).  ``sh``: [9,3]
    second-order spherical-harmonic coefficients; ``direct``: None, or a (direction the light travels, rgb) pair;
    ``visibilities``: None, or per frame the float32 [...] ``shade`` of ``picture_shadow_batch`` (1 = the direct light
    is occluded); ``gamma``: 1.0 (nothing, the bit-exact form) or the exponent's inverse; ``normal_mats``: None (SH at
    the world normal) or host [n_views,3,3] for all frames / [n,n_views,3,3]: SH at the normal in each camera's frame;
    ``n_views``: the views of a frame's picture (None: the leading dimension of a [n_views,H,W,3] picture, else 1).
    Covered pixels hold clamp(albedo * shading, 0, 1), uncovered ones the albedo's bits (``background`` without albedo
    pictures) and shading 0.  Defined bit for bit in include/monoport_hip.h.  ``out``: (images or None, shadings or
    None) to write; the images may be ``albedos`` themselves (in place).  None: fresh images and, with
    ``with_shading``, fresh shadings [...,3].  Returns per frame (image or None, shading or None).  One launch per
    MAX_FRAMES frames (with ``normal_mats``: per MAX_FRAMES frames x views); no host sync."""
    n = len(normals)
    if n == 0 or normals[0].dim() < 2 or normals[0].shape[-1] != 3:
        raise ValueError("%s: at least one normal picture [...,3]" % who)
    shape = tuple(normals[0].shape[:-1])
    dev, npix = normals[0].device, normals[0].numel() // 3
    if npix < 1:
        raise ValueError("%s: at least one pixel" % who)
    if n_views is None:
        n_views = int(shape[0]) if len(shape) == 3 else 1
    if isinstance(n_views, bool) or not isinstance(n_views, (int, np.integer)) or n_views < 1 or npix % n_views:
        raise ValueError("%s: n_views must be an int >= 1 that divides the %d pixels, got %r" % (who, npix, n_views))
    nv = int(n_views)
    normals = _flat_pictures(who, "normals", normals, n, torch.float32, 3, npix, dev)
    face_ids = _flat_pictures(who, "face_ids", face_ids, n, torch.int32, 1, npix, dev)
    if albedos is not None:
        albedos = _flat_pictures(who, "albedos", albedos, n, torch.float32, 3, npix, dev)
    if visibilities is not None:
        visibilities = _flat_pictures(who, "visibilities", visibilities, n, torch.float32, 1, npix, dev)
    if (albedos is None) == (albedo_rgb is None):
        raise ValueError("%s: either albedo pictures or a constant albedo_rgb, not %s"
                         % (who, "neither" if albedos is None else "both"))
    sh, ddir, drgb, gamma, albedo_rgb = light_params(who, sh, direct, gamma, albedo_rgb)
    background = float(background)
    if not math.isfinite(background):
        raise ValueError("%s: background must be finite, got %r" % (who, background))
    mats = None
    if normal_mats is not None:
        mats = np.asarray(normal_mats, np.float32)
        if mats.shape == (nv, 3, 3):
            mats = np.broadcast_to(mats, (n, nv, 3, 3))
        if mats.shape != (n, nv, 3, 3) or not np.isfinite(mats).all():
            raise ValueError("%s: normal_mats must be finite [%d,3,3] or [%d,%d,3,3], got %s"
                             % (who, nv, n, nv, tuple(np.shape(normal_mats))))
    if out is None:
        image = torch.empty((n,) + shape + (3,), dtype=torch.float32, device=dev).unbind(0)
        shading = torch.empty((n,) + shape + (3,), dtype=torch.float32, device=dev).unbind(0) if with_shading else None
    else:
        image = None if out[0] is None else _flat_pictures(who, "out[0] (image)", out[0], n, torch.float32, 3, npix, dev)
        shading = (None if out[1] is None
                   else _flat_pictures(who, "out[1] (shading)", out[1], n, torch.float32, 3, npix, dev))
    if image is None and shading is None:
        raise ValueError("%s: out names no output" % who)
    ctx = get_context(dev)
    # with matrices a call holds frames x views <= MAX_FRAMES of them: a frame's views are then split as its pixels are
    vstep = nv if mats is None else min(nv, MAX_FRAMES)
    fstep = MAX_FRAMES if mats is None else MAX_FRAMES // vstep

    def ptrs(rows, f0, f1, v0, v1):
        if rows is None:
            return None
        return _ptr_array([r if (v0, v1) == (0, nv) else r.view(nv, -1)[v0:v1] for r in rows[f0:f1]])

    pf = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(_lib._pf32)  # noqa: E731
    for v0 in range(0, nv, vstep):
        v1 = min(v0 + vstep, nv)
        for f0 in range(0, n, fstep):
            f1 = min(f0 + fstep, n)
            m = None if mats is None else np.ascontiguousarray(mats[f0:f1, v0:v1])
            ctx.check(ctx.lib.mp_picture_light_batch(
                ctx.handle, f1 - f0, ptrs(normals, f0, f1, v0, v1), ptrs(face_ids, f0, f1, v0, v1),
                ptrs(albedos, f0, f1, v0, v1), pf(albedo_rgb), ptrs(visibilities, f0, f1, v0, v1),
                npix // nv * (v1 - v0), v1 - v0, pf(sh), pf(ddir), pf(drgb), gamma, pf(m), background,
                ptrs(image, f0, f1, v0, v1), ptrs(shading, f0, f1, v0, v1), _stream(normals[0])),
                "mp_picture_light_batch")
    return [(None if image is None else image[f], None if shading is None else shading[f]) for f in range(n)]


def self_shades(who, positions, face_ids, lighting, shadow, out=None):
    """Per subject the shade [n_views,H,W] of its own shadow map on its own surface: ``picture_shadow_batch`` for the
    shade alone on the position pictures, against ``shadow`` = (the scene's ``recon.Light``, map depths, map faces) with
    the bias ``lighting.self_shadow``.  ``out``: the shades' buffers."""
    light, map_depths, map_faces = shadow
    return [s[1] for s in picture_shadow_batch(
        None, list(positions), list(face_ids), map_depths, map_faces, light.calib, light.projection, light.nearest,
        lighting.self_shadow, light.radius, light.strength, out=None if out is None else (None, list(out)), who=who)]


def light_pictures_batch(who, verts, faces, counts, normals, calibs, ras, lighting, images, capacity=None, shadow=None,
                         buffers=None, shades=None, transfers=None):
    """The subjects' pictures ``images`` (per mesh [n_views,H,W,3], as ``_attr_pass`` / ``render_netc_batch`` left
    them) lit in place by ``lighting`` (a ``recon.Lighting``: sh, direct_dir, direct_rgb, gamma, frame, albedo,
    self_shadow), no host value in between: (1) a second pass of the rasteriser with ``attr = normals`` (per mesh
    [V,3]) under the pictures' own cameras and ``Raster`` ``ras``: the same faces, so the same face
    ids; (2) with ``lighting.self_shadow``: a pass with ``attr = verts`` and ``picture_shadow_batch`` for the shade
    alone, against ``shadow`` = (the scene's ``recon.Light``, map depths, map faces: one shadow map per mesh) with the
    bias ``self_shadow``; (3) ``picture_light_batch``: the images are the albedo and the output, or -- with a constant
    ``lighting.albedo`` -- the output only.  ``frame="camera"`` takes the 3x3 of every view's calib as its normal
    matrix.  ``buffers``: None (fresh), or a dict with ``normal`` [n,n_views,H,W,3], ``face`` [n,n_views,H,W] and, for
    the self-shadow, ``pos`` [n,n_views,H,W,3] and ``shade`` [n,n_views,H,W], for the transfer ``ambient``
    [n,n_views,H,W,3] and ``transfer_shade`` [n,max_v,3].  ``shades``: the self-shadow's shades
    where the caller has made them from a position picture it had (``render_netc_batch``'s hook): step (2) is then
    skipped.  ``transfers`` (with ``lighting.transfer``): per mesh the [V,9] radiance transfer of its vertices
    (``mesh_transfer_raw``); the SH term is then a third pass of the rasteriser with ``attr = mesh_transfer_shade`` and
    step (3) is ``picture_light_transfer_batch``.  Returns (per mesh the normal pass's (image, None, face), the shades or
    None)."""
    n = len(verts)
    cams = _calib_list(calibs, n, who)
    background = ras.background

    def attr_pass(attrs, image, face=None):
        """(image, None, face or None) per mesh: into the caller's buffers, or fresh (the depth that comes with fresh
        ones is dropped)."""
        out = None if buffers is None else (buffers[image], None, None if face is None else buffers[face])
        return [(r[0], None, r[2]) for r in _attr_pass(who, verts, faces, counts, attrs, cams, ras, out, capacity)]

    nraws = attr_pass(normals, "normal", "face")
    face_ids = [r[2] for r in nraws]
    if lighting.self_shadow is None:
        shades = None
    elif shades is None:
        shades = self_shades(who, [p[0] for p in attr_pass(list(verts), "pos")], face_ids, lighting, shadow,
                             None if buffers is None else buffers["shade"][:n])
    nv = nraws[0][0].shape[0]
    direct = None if lighting.direct is None else (lighting.direct_dir, lighting.direct_rgb)
    if transfers is not None:  # the SH term is the rasterised product of the vertices' transfer and sh
        sizes = [c.contiguous() for c in counts]
        if buffers is None:  # meshes of their own sizes: one launch per size (the call's spans are its capacity's)
            ts, by_size = [None] * n, {}
            for f, t in enumerate(transfers):
                by_size.setdefault(int(t.shape[0]), []).append(f)
            for fs in by_size.values():
                rows = _mesh_transfer_shade(who, [_f32c(transfers[f]) for f in fs], [sizes[f] for f in fs], lighting.sh,
                                            None)
                for f, row in zip(fs, rows):
                    ts[f] = row
        else:
            ts = _mesh_transfer_shade(who, list(transfers), sizes, lighting.sh, buffers["transfer_shade"])
        araws = attr_pass(ts, "ambient")
        picture_light_transfer_batch([r[0] for r in araws], [r[0] for r in nraws], face_ids,
                                     None if lighting.albedo is not None else list(images), direct, lighting.gamma,
                                     shades, lighting.albedo, background, out=(list(images), None), who=who)
        return nraws, shades
    mats = np.stack([normal_mats_of(who, c) for c in cams]) if lighting.frame == "camera" else None
    picture_light_batch([r[0] for r in nraws], face_ids, None if lighting.albedo is not None else list(images),
                        lighting.sh, direct, lighting.gamma, mats, shades, lighting.albedo, nv, background,
                        out=(list(images), None), who=who)
    return nraws, shades


TRANSFER_MAX_RES = 513  # MP_TRANSFER_MAX_RES
TRANSFER_MAX_DIRS = 512  # MP_TRANSFER_MAX_DIRS


def volume_bits_words(r):
    """mp_volume_bits_words: the 32-bit words of a ``volume_bits`` buffer at resolution ``r``: r * r * ceil(r / 32)
    words of occupancy bits, then the tracer's private block bits."""
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= r <= TRANSFER_MAX_RES:
        raise ValueError("volume_bits_words: resolution must be an int in 1..%d, got %r" % (TRANSFER_MAX_RES, r))
    nb = (r + 7) // 8
    return r * r * ((r + 31) // 32) + (nb ** 3 + 31) // 32


def _volume_bits(who, volumes, level, gates, out):
    vols, n, r, dev = _one_size_volumes(who, volumes)
    words = volume_bits_words(r)
    _gates(who, gates, n, dev)
    if out is None:
        out = torch.empty((n, words), dtype=torch.int32, device=dev).unbind(0)
    else:
        out = _frame_rows(who, "out", out, n, (words,), torch.int32, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_volume_bits_batch(
            ctx.handle, f1 - f0, _ptr_array(vols[f0:f1]), r, float(level), _ptr_array(out[f0:f1]),
            None if gates is None else _ptr_array(gates[f0:f1]), _stream(vols[0])), "mp_volume_bits_batch")
    _keep_until_done(dev, vols, gates)
    return list(out)


def volume_bits_raw(volume, level=0.5, out=None):
    """mp_volume_bits_batch with one frame: the occupancy bits of a cubic f32 volume [R,R,R], R <= 513, as int32
    [volume_bits_words(R)] on the device: bit x & 31 of word (z*R + y) * ceil(R/32) + (x >> 5) is set iff v > level (a
    NaN is empty, padding bits are 0); the words past R * R * ceil(R/32) are ``mesh_transfer``'s own.  No host sync."""
    return _volume_bits("volume_bits_raw", [volume], level, None, None if out is None else [out])[0]


def volume_bits_raw_batch(volumes, level=0.5, gates=None, out=None):
    """mp_volume_bits_batch: ``[volume_bits_raw(v, level) for v in volumes]`` in two launches per MAX_FRAMES volumes,
    the same bits.  ``gates``: as ``marching_cubes_raw_batch``; a gated-off frame is not read or written.  ``out``:
    int32 [n, words] to write into."""
    return _volume_bits("volume_bits_raw_batch", volumes, level, gates, out)


def transfer_params(who, r, b_min, b_max, n_dirs, dirs, basis, weight, bias_w, step_w, max_steps):
    """The host values of mp_mesh_transfer checked: the ValueError of one it refuses."""
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= r <= TRANSFER_MAX_RES:
        raise ValueError("%s: resolution must be an int in 1..%d, got %r" % (who, TRANSFER_MAX_RES, r))
    if (isinstance(n_dirs, bool) or not isinstance(n_dirs, (int, np.integer)) or n_dirs % 64
            or not 64 <= n_dirs <= TRANSFER_MAX_DIRS):
        raise ValueError("%s: n_dirs must be a multiple of 64 in 64..%d, got %r" % (who, TRANSFER_MAX_DIRS, n_dirs))
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or not 1 <= max_steps <= 1 << 24:
        raise ValueError("%s: max_steps must be an int in 1..2^24, got %r" % (who, max_steps))
    lo, hi = _finite_floats(who, "b_min", b_min, (3,)), _finite_floats(who, "b_max", b_max, (3,))
    if not (hi > lo).all():
        raise ValueError("%s: b_max must be > b_min on every axis, got %r and %r" % (who, b_min, b_max))
    vals = [float(np.float32(v)) for v in (weight, bias_w, step_w)]
    if not all(math.isfinite(v) for v in vals) or not vals[2] > 0:
        raise ValueError("%s: weight, bias_w and step_w must be finite and step_w > 0, got %r" % (who, vals))
    for what, t, k in (("dirs", dirs, 3), ("basis", basis, 9)):
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (n_dirs, k)
                or not t.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous float32 [%d,%d] tensor" % (who, what, n_dirs, k))
    return lo, hi, vals


def _mesh_transfer(who, verts, normals, counts, bits, r, b_min, b_max, dirs, basis, weight, bias_w, step_w, max_steps,
                   want, out):
    """``want``: (mask, prt) booleans; ``out``: None or (masks or None, prts or None) to write into."""
    n, max_v, _, dev = _mesh_frames(who, verts, None, counts)
    n_dirs = int(dirs.shape[0]) if torch.is_tensor(dirs) and dirs.dim() == 2 else 0
    lo, hi, (weight, bias_w, step_w) = transfer_params(who, r, b_min, b_max, n_dirs, dirs, basis, weight, bias_w,
                                                       step_w, max_steps)
    if dirs.device != dev or basis.device != dev:
        raise ValueError("%s: dirs and basis must live on the meshes' device" % who)
    normals = _frame_rows(who, "normals", normals, n, (max_v, 3), torch.float32, dev)
    bits = _frame_rows(who, "bits", bits, n, (volume_bits_words(r),), torch.int32, dev)
    words = n_dirs // 64
    if out is None:
        mask = torch.empty((n, max_v, words), dtype=torch.int64, device=dev).unbind(0) if want[0] else None
        prt = torch.empty((n, max_v, 9), dtype=torch.float32, device=dev).unbind(0) if want[1] else None
    else:
        mask = None if out[0] is None else _frame_rows(who, "out[0] (mask)", out[0], n, (max_v, words), torch.int64, dev)
        prt = None if out[1] is None else _frame_rows(who, "out[1] (prt)", out[1], n, (max_v, 9), torch.float32, dev)
    if mask is None and prt is None:
        raise ValueError("%s: no output requested" % who)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_transfer_batch(
            ctx.handle, f1 - f0, _ptr_array(verts[f0:f1]), _ptr_array(normals[f0:f1]), max_v,
            _ptr_array(counts[f0:f1]), _ptr_array(bits[f0:f1]), int(r), _float3(lo), _float3(hi), n_dirs, _ptr(dirs),
            _ptr(basis), weight, bias_w, step_w, int(max_steps), None if mask is None else _ptr_array(mask[f0:f1]),
            None if prt is None else _ptr_array(prt[f0:f1]), _stream(verts[0])), "mp_mesh_transfer_batch")
    _keep_until_done(dev, verts, normals, counts, bits, [dirs, basis])
    return [(None if mask is None else mask[f], None if prt is None else prt[f]) for f in range(n)]


def mesh_transfer_raw(verts, normals, counts, bits, r, b_min, b_max, dirs, basis, weight, bias_w, step_w, max_steps,
                      want=(True, True), out=None):
    """mp_mesh_transfer_batch with one frame: verts / normals [max_v,3] f32, counts int32[2], bits (``volume_bits_raw``
    at resolution ``r``) on the device; ``dirs`` [D,3] and ``basis`` [D,9] device f32 tables; weight, bias_w, step_w
    (world units) and max_steps host values -> (mask int64 [max_v, D/64]: the 64-bit visibility words, bit d & 63 of
    word d >> 6; prt f32 [max_v,9]); either is None where ``want`` = (mask, prt) says so.  Rows beyond counts[0] are
    not written.  Defined bit for bit in include/monoport_hip.h.  No host sync."""
    return _mesh_transfer("mesh_transfer_raw", [verts], [normals], [counts], [bits], r, b_min, b_max, dirs, basis,
                          weight, bias_w, step_w, max_steps, want,
                          None if out is None else tuple(None if o is None else [o] for o in out))[0]


def mesh_transfer_raw_batch(verts, normals, counts, bits, r, b_min, b_max, dirs, basis, weight, bias_w, step_w,
                            max_steps, want=(True, True), out=None):
    """mp_mesh_transfer_batch: ``mesh_transfer_raw`` per mesh (one capacity, one resolution, one parameter set) in one
    launch per MAX_FRAMES meshes, the same bits.  ``out``: (mask [n,max_v,D/64] int64 or None, prt [n,max_v,9] f32 or
    None)."""
    return _mesh_transfer("mesh_transfer_raw_batch", verts, normals, counts, bits, r, b_min, b_max, dirs, basis, weight,
                          bias_w, step_w, max_steps, want, out)


def _mesh_transfer_shade(who, prts, counts, sh, out):
    n = len(prts)
    if n == 0 or len(counts) != n:
        raise ValueError("%s: at least one mesh, and one counts per mesh" % who)
    sh = _finite_floats(who, "sh", sh, (9, 3))
    dev, max_v = prts[0].device, prts[0].shape[0]
    counts = _frame_rows(who, "counts", counts, n, (2,), torch.int32, dev)
    prts = _frame_rows(who, "prt", prts, n, (max_v, 9), torch.float32, dev)
    if out is None:
        out = torch.empty((n, max_v, 3), dtype=torch.float32, device=dev).unbind(0)
    else:
        out = _frame_rows(who, "out", out, n, (max_v, 3), torch.float32, dev)
    if max_v == 0:
        return list(out)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_mesh_transfer_shade_batch(
            ctx.handle, f1 - f0, _ptr_array(prts[f0:f1]), max_v, _ptr_array(counts[f0:f1]),
            sh.ctypes.data_as(_lib._pf32), _ptr_array(out[f0:f1]), _stream(prts[0])), "mp_mesh_transfer_shade_batch")
    _keep_until_done(dev, prts, counts)
    return list(out)


def mesh_transfer_shade_raw(prt, counts, sh, out=None):
    """mp_mesh_transfer_shade_batch with one frame: prt [max_v,9] f32 and ``sh`` [9,3] (host) -> t [max_v,3] f32, t_c =
    sum over k ascending of prt_k * sh[k][c] from 0.0f; rows beyond counts[0] are not written.  No host sync."""
    return _mesh_transfer_shade("mesh_transfer_shade_raw", [prt], [counts], sh, None if out is None else [out])[0]


def mesh_transfer_shade_raw_batch(prts, counts, sh, out=None):
    """mp_mesh_transfer_shade_batch: ``mesh_transfer_shade_raw`` per mesh in one launch per MAX_FRAMES meshes."""
    return _mesh_transfer_shade("mesh_transfer_shade_raw_batch", prts, counts, sh, out)


def picture_light_transfer_batch(ambients, normals, face_ids, albedos, direct=None, gamma=1.0, visibilities=None,
                                 albedo_rgb=None, background=1.0, out=None, with_shading=False,
                                 who="picture_light_transfer_batch"):
    """mp_picture_light_transfer_batch: ``picture_light_batch`` with the SH term given per pixel: ``ambients``, per frame
    float32 [...,3], the rasteriser's image for ``attr = mesh_transfer_shade_raw``'s t with the paint (1, 0, -inf, inf).
    ``normals`` may be None without a ``direct`` term.  No ``normal_mats``: the camera frame is not built.  Everything
    else, the outputs and the return value as ``picture_light_batch``."""
    n = len(ambients)
    if n == 0 or ambients[0].dim() < 2 or ambients[0].shape[-1] != 3:
        raise ValueError("%s: at least one ambient picture [...,3]" % who)
    shape = tuple(ambients[0].shape[:-1])
    dev, npix = ambients[0].device, ambients[0].numel() // 3
    if npix < 1:
        raise ValueError("%s: at least one pixel" % who)
    ambients = _flat_pictures(who, "ambients", ambients, n, torch.float32, 3, npix, dev)
    if normals is not None:
        normals = _flat_pictures(who, "normals", normals, n, torch.float32, 3, npix, dev)
    face_ids = _flat_pictures(who, "face_ids", face_ids, n, torch.int32, 1, npix, dev)
    if albedos is not None:
        albedos = _flat_pictures(who, "albedos", albedos, n, torch.float32, 3, npix, dev)
    if visibilities is not None:
        visibilities = _flat_pictures(who, "visibilities", visibilities, n, torch.float32, 1, npix, dev)
    if (albedos is None) == (albedo_rgb is None):
        raise ValueError("%s: either albedo pictures or a constant albedo_rgb, not %s"
                         % (who, "neither" if albedos is None else "both"))
    _, ddir, drgb, gamma, albedo_rgb = light_params(who, np.zeros((9, 3), np.float32), direct, gamma, albedo_rgb)
    if normals is None and drgb.any():
        raise ValueError("%s: the direct term needs the normal pictures" % who)
    background = float(background)
    if not math.isfinite(background):
        raise ValueError("%s: background must be finite, got %r" % (who, background))
    if out is None:
        image = torch.empty((n,) + shape + (3,), dtype=torch.float32, device=dev).unbind(0)
        shading = torch.empty((n,) + shape + (3,), dtype=torch.float32, device=dev).unbind(0) if with_shading else None
    else:
        image = None if out[0] is None else _flat_pictures(who, "out[0] (image)", out[0], n, torch.float32, 3, npix, dev)
        shading = (None if out[1] is None
                   else _flat_pictures(who, "out[1] (shading)", out[1], n, torch.float32, 3, npix, dev))
    if image is None and shading is None:
        raise ValueError("%s: out names no output" % who)
    ctx = get_context(dev)
    pf = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(_lib._pf32)  # noqa: E731
    pa = lambda rows, f0, f1: None if rows is None else _ptr_array(list(rows[f0:f1]))  # noqa: E731
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_picture_light_transfer_batch(
            ctx.handle, f1 - f0, pa(normals, f0, f1), pa(face_ids, f0, f1), pa(albedos, f0, f1), pf(albedo_rgb),
            pa(visibilities, f0, f1), pa(ambients, f0, f1), npix, pf(ddir), pf(drgb), gamma, background,
            pa(image, f0, f1), pa(shading, f0, f1), _stream(ambients[0])), "mp_picture_light_transfer_batch")
    return [(None if image is None else image[f], None if shading is None else shading[f]) for f in range(n)]


def render_scene_batch(who, scene, calibs, ras, out=None, uv=None, positions=None):
    """The textured pictures of ``scene`` (a ``recon.Scene``: verts, faces, counts, attr = (u, v, 0) per vertex, pyramid,
    tex_size, levels, wrap) under one camera set per frame (``calibs``: a list, all of one n_views), no host value in
    between: (1) the rasteriser with the scene's tensors repeated per frame and its uv as the attribute, under the
    pictures' own cameras and ``Raster`` ``ras``, into a UV picture; (2) ``picture_texture_batch`` into
    the image.  Returns what ``_mesh_render`` does: per frame (image [n_views,H,W,3], depth, face).  ``out``: (image,
    depth, face) buffers; ``uv``: the UV pictures' buffers [n,n_views,H,W,3] (scratch of the call).  ``positions``:
    None, or buffers [n,n_views,H,W,3] that a second pass of the rasteriser with ``attr = scene.verts`` fills with the
    world-space point of every pixel (what ``picture_shadow_batch`` reads); nothing more is enqueued without them."""
    n = len(calibs)
    if n == 0:
        raise ValueError("%s: at least one camera set" % who)
    if out is None:
        if uv is not None:
            raise ValueError("%s: uv= buffers go with out=" % who)
    else:
        if any(o is None for o in out):
            raise ValueError("%s: a scene picture has an image, a depth and face ids" % who)
        if uv is None:
            uv = [torch.empty_like(o) for o in out[0]]
    mesh = ([scene.verts] * n, [scene.faces] * n, [scene.counts] * n)
    raws = _attr_pass(who, *mesh, [scene.attr] * n, list(calibs), ras, None if out is None else (uv, out[1], out[2]))
    if positions is not None:  # the same faces under the same cameras and flags: the face ids are the UV pass's
        _attr_pass(who, *mesh, [scene.verts] * n, list(calibs), ras, (positions, None, None))
    images = picture_texture_batch([r[0] for r in raws], [r[2] for r in raws], scene.pyramid, scene.tex_size,
                                   scene.levels, scene.wrap, background=ras.background,
                                   out=None if out is None else out[0], who=who)
    return [(im, r[1], r[2]) for im, r in zip(images, raws)]


# MP_JPEG_* (include/monoport_hip.h)
JPEG_SUBSAMPLINGS = {"444": _lib.JPEG_444, "420": _lib.JPEG_420}
JPEG_MAX_SIDE = 4096  # MP_JPEG_MAX_SIDE
JPEG_HEADER_BYTES = 629


def picture_u8_raw(image, out=None):
    """mp_picture_u8: float32 [...,3] -> uint8 of the same shape, clamp(x, 0, 1) * 255 + 0.5 truncated (two f32
    operations, a NaN gives 0): step 1 of the JPEG definition in include/monoport_hip.h.  ``out``: a contiguous uint8
    tensor of that shape to write into.  No host sync."""
    who = "picture_u8_raw"
    if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() < 1 or image.shape[-1] != 3:
        raise ValueError("%s: image must be a float32 tensor [...,3]" % who)
    image = image.contiguous()
    if out is None:
        out = torch.empty(image.shape, dtype=torch.uint8, device=image.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != image.shape
          or not out.is_contiguous() or out.device != image.device):
        raise ValueError("%s: out must be a contiguous uint8 tensor %s on %s" % (who, tuple(image.shape), image.device))
    ctx = get_context(image.device)
    ctx.check(ctx.lib.mp_picture_u8(ctx.handle, _ptr(image), image.numel() // 3, _ptr(out), _stream(image)),
              "mp_picture_u8")
    return out


def jpeg_params(who, quality, subsampling, restart):
    """(quality, MP_JPEG_* subsampling, restart with 0 for the default) of mp_picture_jpeg as ints, checked."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError("%s: quality must be an int in 1..100, got %r" % (who, quality))
    sub = _named_mode(who, "subsampling", JPEG_SUBSAMPLINGS, subsampling)
    if restart is None:
        restart = 0
    elif isinstance(restart, bool) or not isinstance(restart, (int, np.integer)) or not 1 <= restart <= 65535:
        raise ValueError("%s: restart must be None (one MCU row) or an int in 1..65535 MCUs, got %r" % (who, restart))
    return int(quality), sub, int(restart)


def jpeg_max_bytes(h, w, subsampling="420", restart=None):
    """mp_jpeg_max_bytes: what no JPEG file of an [h,w,3] picture exceeds at any content and quality: the 629-byte
    header + 416 bytes per 8x8 block + 2 per restart interval.  Typical files are a small fraction of it."""
    who = "jpeg_max_bytes"
    _, sub, restart = jpeg_params(who, 90, subsampling, restart)
    for side in (h, w):
        if isinstance(side, bool) or not isinstance(side, (int, np.integer)) or not 1 <= side <= JPEG_MAX_SIDE:
            raise ValueError("%s: h and w must be ints in 1..%d, got %r x %r" % (who, JPEG_MAX_SIDE, h, w))
    return int(_lib.load().mp_jpeg_max_bytes(int(h), int(w), sub, restart))


def picture_jpeg_raw(images, quality=90, subsampling="420", restart=None, capacity=None, out=None, info=None):
    """mp_picture_jpeg: ``images`` float32 [n,H,W,3] (contiguous: one base pointer, any n up to 65535) -> (out uint8
    [n,capacity], info int32 [n,2]) on the device: file i is ``out[i, :info[i, 0]]`` where ``info[i, 1] == 0``; where it
    is 1 the file did not fit, nothing of it was written and ``info[i, 0]`` is the capacity it needs.  Baseline JFIF with
    restart intervals of ``restart`` MCUs (None: one MCU row), defined byte for byte in include/monoport_hip.h.
    ``capacity``: None = ``jpeg_max_bytes`` (never overflows), else bytes per picture (>= the 629-byte header).  ``out`` /
    ``info``: contiguous tensors to write into (``out`` gives the capacity).  One set of six launches; no host sync."""
    who = "picture_jpeg_raw"
    if (not isinstance(images, torch.Tensor) or images.dtype != torch.float32 or images.dim() != 4
            or images.shape[-1] != 3 or not images.is_contiguous()):
        raise ValueError("%s: images must be a contiguous float32 tensor [n,H,W,3]" % who)
    n, h, w = (int(v) for v in images.shape[:3])
    if n < 1 or not (1 <= h <= JPEG_MAX_SIDE and 1 <= w <= JPEG_MAX_SIDE):
        raise ValueError("%s: at least one picture with sides in 1..%d, got %s" % (who, JPEG_MAX_SIDE, tuple(images.shape)))
    quality, sub, restart = jpeg_params(who, quality, subsampling, restart)
    dev = images.device
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != n
                or not out.is_contiguous() or out.device != dev):
            raise ValueError("%s: out must be a contiguous uint8 tensor [%d,capacity] on %s" % (who, n, dev))
        if capacity is not None and int(capacity) != out.shape[1]:
            raise ValueError("%s: capacity %r against an out of %d bytes per picture" % (who, capacity, out.shape[1]))
        capacity = int(out.shape[1])
    elif capacity is None:
        capacity = jpeg_max_bytes(h, w, subsampling, restart or None)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < JPEG_HEADER_BYTES:
        raise ValueError("%s: capacity must be an int >= the header's %d bytes, got %r" % (who, JPEG_HEADER_BYTES, capacity))
    if info is None:
        info = torch.empty((n, 2), dtype=torch.int32, device=dev)
    elif (not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or info.shape != (n, 2)
          or not info.is_contiguous() or info.device != dev):
        raise ValueError("%s: info must be a contiguous int32 tensor [%d,2] on %s" % (who, n, dev))
    if out is None:
        out = torch.empty((n, int(capacity)), dtype=torch.uint8, device=dev)
    ctx = get_context(dev)
    ctx.check(ctx.lib.mp_picture_jpeg(ctx.handle, _ptr(images), n, h, w, quality, sub, restart, _ptr(out), int(capacity),
                                      _ptr(info), _stream(images)), "mp_picture_jpeg")
    _keep_until_done(dev, [images])
    return out, info


# MP_PNG_* (include/monoport_hip.h)
PNG_FORMATS = {"rgb8": _lib.PNG_RGB8, "rgba8": _lib.PNG_RGBA8, "gray16": _lib.PNG_GRAY16}
PNG_FILTERS = {"none": _lib.PNG_NONE, "sub": _lib.PNG_SUB, "up": _lib.PNG_UP, "average": _lib.PNG_AVERAGE,
               "paeth": _lib.PNG_PAETH, "adaptive": _lib.PNG_ADAPTIVE}
PNG_MAX_SIDE = 4096  # MP_PNG_MAX_SIDE
PNG_MIN_BYTES = 57   # MP_PNG_MIN_BYTES


def _finite_float(who, what, value):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not np.isfinite(np.float32(value)):
        raise ValueError("%s: %s must be a finite number, got %r" % (who, what, value))
    return float(np.float32(value))


def png_params(who, format="rgb8", filter="adaptive", lo=0.0, scale=1.0, unmatte=None):
    """(MP_PNG_* format, MP_PNG_* filter, lo, scale, unmatte flag, background) of mp_picture_png, checked.  ``unmatte``:
    None, or the background value the colour is freed of (RGBA8 only)."""
    fmt = _named_mode(who, "format", PNG_FORMATS, format)
    flt = _named_mode(who, "filter", PNG_FILTERS, filter)
    lo, scale = _finite_float(who, "lo", lo), _finite_float(who, "scale", scale)
    if unmatte is not None and fmt != _lib.PNG_RGBA8:
        raise ValueError("%s: unmatte needs an alpha (format 'rgba8')" % who)
    return fmt, flt, lo, scale, int(unmatte is not None), 0.0 if unmatte is None else _finite_float(who, "unmatte", unmatte)


def png_max_bytes(h, w, format="rgb8"):
    """mp_png_max_bytes: what no PNG file of an [h,w] picture in ``format`` exceeds at any content: 16 bits per filtered
    byte, 288 bytes per 4096-byte block, the container.  Typical files are a small fraction of it."""
    who = "png_max_bytes"
    fmt = _named_mode(who, "format", PNG_FORMATS, format)
    for side in (h, w):
        if isinstance(side, bool) or not isinstance(side, (int, np.integer)) or not 1 <= side <= PNG_MAX_SIDE:
            raise ValueError("%s: h and w must be ints in 1..%d, got %r x %r" % (who, PNG_MAX_SIDE, h, w))
    return int(_lib.load().mp_png_max_bytes(int(h), int(w), fmt))


def _sample_out(who, out, shape, dtype, dev):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != tuple(shape)
            or not out.is_contiguous() or out.device != dev):
        raise ValueError("%s: out must be a contiguous %s tensor %s on %s" % (who, dtype, tuple(shape), dev))
    return out


def picture_u16_raw(depth, lo=0.0, scale=1.0, out=None):
    """mp_picture_u16: float32 [...] -> uint16 of the same shape, clamp((d - lo) * scale, 0, 1) * 65535 + 0.5 truncated
    (separately rounded f32 operations, a NaN gives 0): the GRAY16 samples of the PNG definition.  No host sync."""
    who = "picture_u16_raw"
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32:
        raise ValueError("%s: depth must be a float32 tensor" % who)
    lo, scale = _finite_float(who, "lo", lo), _finite_float(who, "scale", scale)
    depth = depth.contiguous()
    out = _sample_out(who, out, depth.shape, torch.uint16, depth.device)
    ctx = get_context(depth.device)
    ctx.check(ctx.lib.mp_picture_u16(ctx.handle, _ptr(depth), depth.numel(), lo, scale, _ptr(out), _stream(depth)),
              "mp_picture_u16")
    _keep_until_done(depth.device, [depth])
    return out


def picture_rgba8_raw(image, alpha, unmatte=None, out=None):
    """mp_picture_rgba8: image float32 [...,3] and alpha float32 [...] -> uint8 [...,4]: the RGBA8 samples of the PNG
    definition; ``unmatte``: None, or the background value the colour is freed of.  No host sync."""
    who = "picture_rgba8_raw"
    if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() < 1 or image.shape[-1] != 3:
        raise ValueError("%s: image must be a float32 tensor [...,3]" % who)
    if (not isinstance(alpha, torch.Tensor) or alpha.dtype != torch.float32 or alpha.shape != image.shape[:-1]
            or alpha.device != image.device):
        raise ValueError("%s: alpha must be a float32 tensor %s on %s" % (who, tuple(image.shape[:-1]), image.device))
    bg = 0.0 if unmatte is None else _finite_float(who, "unmatte", unmatte)
    image, alpha = image.contiguous(), alpha.contiguous()
    out = _sample_out(who, out, tuple(alpha.shape) + (4,), torch.uint8, image.device)
    ctx = get_context(image.device)
    ctx.check(ctx.lib.mp_picture_rgba8(ctx.handle, _ptr(image), _ptr(alpha), alpha.numel(), int(unmatte is not None), bg,
                                       _ptr(out), _stream(image)), "mp_picture_rgba8")
    _keep_until_done(image.device, [image, alpha])
    return out


def picture_png_raw(images, alpha=None, format="rgb8", filter="adaptive", lo=0.0, scale=1.0, unmatte=None,
                    capacity=None, out=None, info=None):
    """mp_picture_png: ``images`` float32 [n,H,W,3] ([n,H,W] for 'gray16'; contiguous, any n up to 65535) and, for
    'rgba8', ``alpha`` float32 [n,H,W] -> (out uint8 [n,capacity], info int32 [n,2]) on the device, as
    ``picture_jpeg_raw`` returns them: file i is ``out[i, :info[i, 0]]`` where ``info[i, 1] == 0``; where it is 1 nothing
    of it was written and ``info[i, 0]`` is the capacity it needs.  The files are defined byte for byte in
    include/monoport_hip.h.  ``capacity``: None = ``png_max_bytes`` (never overflows).  One set of six launches; no host
    sync."""
    who = "picture_png_raw"
    fmt, flt, lo, scale, un, bg = png_params(who, format, filter, lo, scale, unmatte)
    gray = fmt == _lib.PNG_GRAY16
    if (not isinstance(images, torch.Tensor) or images.dtype != torch.float32 or images.dim() != (3 if gray else 4)
            or (not gray and images.shape[-1] != 3) or not images.is_contiguous()):
        raise ValueError("%s: images must be a contiguous float32 tensor %s" % (who, "[n,H,W]" if gray else "[n,H,W,3]"))
    n, h, w = (int(v) for v in images.shape[:3])
    if n < 1 or not (1 <= h <= PNG_MAX_SIDE and 1 <= w <= PNG_MAX_SIDE):
        raise ValueError("%s: at least one picture with sides in 1..%d, got %s" % (who, PNG_MAX_SIDE, tuple(images.shape)))
    dev = images.device
    if (fmt == _lib.PNG_RGBA8) != (alpha is not None):
        raise ValueError("%s: alpha goes with format 'rgba8' and with no other" % who)
    if alpha is not None and (not isinstance(alpha, torch.Tensor) or alpha.dtype != torch.float32
                              or tuple(alpha.shape) != (n, h, w) or not alpha.is_contiguous() or alpha.device != dev):
        raise ValueError("%s: alpha must be a contiguous float32 tensor [%d,%d,%d] on %s" % (who, n, h, w, dev))
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != n
                or not out.is_contiguous() or out.device != dev):
            raise ValueError("%s: out must be a contiguous uint8 tensor [%d,capacity] on %s" % (who, n, dev))
        if capacity is not None and int(capacity) != out.shape[1]:
            raise ValueError("%s: capacity %r against an out of %d bytes per picture" % (who, capacity, out.shape[1]))
        capacity = int(out.shape[1])
    elif capacity is None:
        capacity = png_max_bytes(h, w, fmt)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < PNG_MIN_BYTES:
        raise ValueError("%s: capacity must be an int >= the smallest file's %d bytes, got %r"
                         % (who, PNG_MIN_BYTES, capacity))
    if info is None:
        info = torch.empty((n, 2), dtype=torch.int32, device=dev)
    elif (not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or info.shape != (n, 2)
          or not info.is_contiguous() or info.device != dev):
        raise ValueError("%s: info must be a contiguous int32 tensor [%d,2] on %s" % (who, n, dev))
    if out is None:
        out = torch.empty((n, int(capacity)), dtype=torch.uint8, device=dev)
    ctx = get_context(dev)
    ctx.check(ctx.lib.mp_picture_png(ctx.handle, _ptr(images), None if alpha is None else _ptr(alpha), n, h, w, fmt, flt,
                                     lo, scale, un, bg, _ptr(out), int(capacity), _ptr(info), _stream(images)),
              "mp_picture_png")
    _keep_until_done(dev, [images, alpha])
    return out, info


# MP_CONN_* (include/monoport_hip.h): face neighbours / face, edge and corner neighbours
CONNECTIVITIES = (_lib.CONN_6, _lib.CONN_26)


def _keep_largest(who, sdfs, level, connectivity, fill, gates, out):
    """``out``: None or (volumes, stats), of which either may be None = allocated here."""
    vols, n, r, dev = _one_size_volumes(who, sdfs)
    if connectivity not in CONNECTIVITIES:
        raise ValueError("%s: connectivity must be one of %s, got %r" % (who, list(CONNECTIVITIES), connectivity))
    if not float(fill) <= float(level):  # a NaN fill fails this test too
        raise ValueError("%s: fill %r would be foreground at level %r" % (who, fill, level))
    _gates(who, gates, n, dev)
    cleaned, stats = (None, None) if out is None else out
    if cleaned is None:
        cleaned = torch.empty((n, r, r, r), dtype=torch.float32, device=dev).unbind(0)
    else:
        cleaned = _frame_rows(who, "out[0] (volumes)", cleaned, n, (r, r, r), torch.float32, dev)
    if stats is None:
        stats = torch.empty((n, 4), dtype=torch.int32, device=dev).unbind(0)
    else:
        stats = _frame_rows(who, "out[1] (stats)", stats, n, (4,), torch.int32, dev)
    ctx = get_context(dev)
    for f0, f1 in _frame_chunks(n):
        ctx.check(ctx.lib.mp_volume_keep_largest_batch(
            ctx.handle, f1 - f0, _ptr_array(vols[f0:f1]), r, float(level), int(connectivity), float(fill),
            _ptr_array(cleaned[f0:f1]), _ptr_array(stats[f0:f1]),
            None if gates is None else _ptr_array(gates[f0:f1]), _stream(vols[0])), "mp_volume_keep_largest_batch")
    _keep_until_done(dev, vols, gates)
    return list(zip(cleaned, stats))


def keep_largest_raw(sdf, level=0.5, connectivity=6, fill=0.0, out=None):
    """mp_volume_keep_largest_batch with one frame: the cubic volume with every voxel > level outside its largest
    connected body (``connectivity`` 6 or 26; ties: the smallest linear index) replaced by ``fill`` -> (volume [R,R,R]
    f32, stats int32[4] = foreground voxels, components, voxels kept, id of the kept component or -1) on device.
    ``out``: a contiguous f32 [R,R,R] tensor to write into (it may be the volume itself).  No host sync."""
    return _keep_largest("keep_largest_raw", [sdf], level, connectivity, fill, None,
                         None if out is None else ([out], None))[0]


def keep_largest_raw_batch(sdfs, level=0.5, connectivity=6, fill=0.0, gates=None, out=None):
    """mp_volume_keep_largest_batch: ``[keep_largest_raw(s, ...) for s in sdfs]`` (cubic volumes of one size on one
    device) in one set of six launches per MAX_FRAMES volumes: per volume (volume [R,R,R], stats int32[4]), views of
    two tensors and bit for bit what the per-volume call gives.  ``gates``: per-frame device int32 tensors (or None
    entries = frame on); a frame whose gate reads 0 gets stats (0, 0, 0, -1) and nothing else of it is read or
    written.  ``out``: (volumes [n,R,R,R] f32, stats [n,4] int32) to write into.  No host sync."""
    return _keep_largest("keep_largest_raw_batch", sdfs, level, connectivity, fill, gates, out)


def group_norm(x, groups, weight, bias, eps=1e-5, relu=False):
    """[relu](GroupNorm(x)) for x [N,C,H,W] f32 contiguous on the GPU (mp_group_norm)."""
    ctx = get_encoder_context(x.device)
    n, c = x.shape[0], x.shape[1]
    hw = x.shape[2] * x.shape[3]
    y = torch.empty_like(x)
    ctx.check(ctx.lib.mp_group_norm(ctx.handle, _ptr(x), n, c, hw, int(groups), _ptr(weight),
                                    _ptr(bias), float(eps), int(bool(relu)), _ptr(y), _stream(x)),
              "mp_group_norm")
    return y


def group_norm_supported(x):
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32
            and x.is_contiguous() and (x.shape[2] * x.shape[3]) % 4 == 0)


def upsample_bicubic2x(x, add=None):
    """[add +] F.interpolate(x, scale_factor=2, mode='bicubic', align_corners=True), x [N,C,H,W]
    (the batch is folded into the channel axis: every plane is resampled independently)."""
    ctx = get_encoder_context(x.device)
    n, c, h, w = x.shape
    y = torch.empty((n, c, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    ctx.check(ctx.lib.mp_upsample_bicubic2x(ctx.handle, _ptr(x), n * c, h, w,
                                            _ptr(add) if add is not None else None, _ptr(y),
                                            _stream(x)), "mp_upsample_bicubic2x")
    return y


def concat3_add_supported(a, b, c, shortcut):
    ts = (a, b, c, shortcut)
    return (all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in ts)
            and (a.shape[2] * a.shape[3]) % 4 == 0
            and a.shape[1] + b.shape[1] + c.shape[1] == shortcut.shape[1])


def concat3_add(a, b, c, shortcut):
    """torch.cat((a, b, c), 1) + shortcut in one pass (the tail of the encoders' ConvBlock)."""
    a, b, c, shortcut = _f32c(a), _f32c(b), _f32c(c), _f32c(shortcut)
    ctx = get_encoder_context(a.device)
    n, ca, h, w = a.shape
    y = torch.empty_like(shortcut)
    ctx.check(ctx.lib.mp_concat3_add(ctx.handle, _ptr(a), ca, _ptr(b), b.shape[1], _ptr(c),
                                     c.shape[1], _ptr(shortcut), n, h * w, _ptr(y), _stream(a)),
              "mp_concat3_add")
    return y


# MONOPORT_CONV_WINOGRAD=0: never pack Winograd-domain weights (every 3x3 convolution on the direct kernels)
CONV_WINOGRAD = os.environ.get("MONOPORT_CONV_WINOGRAD", "1") != "0"


class PackedConv3x3:
    """nn.Conv2d(Cin, Cout, 3, 1, 1, bias=False) weights in the MFMA fragment order of
    csrc/conv3x3.hip: exact f32 (mp_conv3x3_pack) or pre-split f16 halves for the "f16x3"
    arithmetic (mp_conv3x3_pack16; as accurate as f32, 5.3x fewer matrix cycles)."""

    def __init__(self, weight, precision="f32"):
        w = _f32c(weight.detach())
        self.cout, self.cin = int(w.shape[0]), int(w.shape[1])
        if tuple(w.shape[2:]) != (3, 3):
            raise ValueError("PackedConv3x3 wants a [Cout,Cin,3,3] weight, got %s" % (tuple(w.shape),))
        if precision not in ("f32", "f16x3"):
            raise ValueError("conv precision must be 'f32' or 'f16x3'")
        self.precision = precision
        ctx = get_encoder_context(w.device)
        self.data = torch.empty((w.numel(),), dtype=torch.float32, device=w.device)  # same bytes either way
        self.wmax = None
        self.wino = None  # Winograd-domain weights (csrc/conv_wino.hip) for the shapes that kernel serves
        if precision == "f32":
            ctx.check(ctx.lib.mp_conv3x3_pack(ctx.handle, _ptr(w), self.cout, self.cin, _ptr(self.data),
                                              _stream(w)), "mp_conv3x3_pack")
            if CONV_WINOGRAD and self.cout % 64 == 0:
                self.wino = torch.empty((16 * self.cout * self.cin,), dtype=torch.float32, device=w.device)
                ctx.check(ctx.lib.mp_conv3x3_pack_wino(ctx.handle, _ptr(w), self.cout, self.cin, _ptr(self.wino),
                                                       _stream(w)), "mp_conv3x3_pack_wino")
        else:
            self.wmax = torch.zeros((1,), dtype=torch.float32, device=w.device)
            ctx.check(ctx.lib.mp_conv3x3_pack16(ctx.handle, _ptr(w), self.cout, self.cin, _ptr(self.data),
                                                _ptr(self.wmax), _stream(w)), "mp_conv3x3_pack16")
        w.record_stream(torch.cuda.current_stream(w.device))


def conv3x3_supported(cin, cout, h, w):
    """True if csrc/conv3x3.hip is built for this shape (mp_conv3x3_supported)."""
    return bool(_lib.load().mp_conv3x3_supported(int(cin), int(cout), int(h), int(w)))


def conv3x3_stats_supported(cout):
    """True if the convolution kernels can emit the GroupNorm(32, Cout) statistics of their own output
    (mp_conv_stats_supported: Cout / 32 divides 32).  Other widths get y, and the launchers refuse ``stats``."""
    return bool(_lib.load().mp_conv_stats_supported(int(cout)))


def scale_shift_add(t, ss, res):
    """res + (t * scale + shift): x + GroupNorm(t) with (scale, shift) from ``gn_finalize``."""
    ctx = get_encoder_context(t.device)
    t, res = t.contiguous(), res.contiguous()
    n, c = t.shape[0], t.shape[1]
    y = torch.empty_like(t)
    ctx.check(ctx.lib.mp_scale_shift_add(ctx.handle, _ptr(t), _ptr(ss), _ptr(res), n, c,
                                         t.shape[2] * t.shape[3], _ptr(y), _stream(t)), "mp_scale_shift_add")
    return y


def conv3x3_gn(x, ss, packed, relu=True, want_stats=False, reflect=False):
    """y = conv3x3(relu?(x * scale + shift)) (stride 1, zero padding 1 -- or ReflectionPad2d(1) with
    ``reflect`` -- no bias) as one MFMA kernel; ``ss`` [N,Cin,2] from ``gn_finalize`` or None (plain
    x).  Returns (y, stats) where
    stats = (partial sums double [N,32,S,2], S) of GroupNorm(32, Cout) over y, or None."""
    ctx = get_encoder_context(x.device)
    n, cin, h, w = x.shape
    if cin != packed.cin:
        raise ValueError("conv3x3_gn: input has %d channels, weights expect %d" % (cin, packed.cin))
    y = torch.empty((n, packed.cout, h, w), dtype=torch.float32, device=x.device)
    stats = None
    if want_stats:
        s = ctx.lib.mp_conv3x3_stat_slices(packed.cout, n, h, w, int(packed.precision == "f16x3"))
        stats = (torch.empty((n, 32, s, 2), dtype=torch.float64, device=x.device), s)
    if packed.precision == "f32":
        ctx.check(ctx.lib.mp_conv3x3_gn(ctx.handle, _ptr(x), n, cin, h, w,
                                        _ptr(ss) if ss is not None else None, int(bool(relu)),
                                        int(bool(reflect)), _ptr(packed.data), packed.cout, _ptr(y),
                                        _ptr(stats[0]) if stats else None, _stream(x)), "mp_conv3x3_gn")
    else:
        ctx.check(ctx.lib.mp_conv3x3_gn16(ctx.handle, _ptr(x), n, cin, h, w,
                                          _ptr(ss) if ss is not None else None, int(bool(relu)),
                                          int(bool(reflect)), _ptr(packed.data), _ptr(packed.wmax),
                                          packed.cout, _ptr(y),
                                          _ptr(stats[0]) if stats else None, _stream(x)),
                  "mp_conv3x3_gn16")
    return y, stats


class PackedConv1x1:
    """Weights of one fused 1x1 convolution in MFMA fragment order: W1 [Cout,C1(,1,1)] and optionally
    W2 [Cout,C2(,1,1)] (second K segment), biases summed (``b1`` may be None).  Cout = 256 (the
    hourglass tail) or 128 / 256 (the projection shortcut of a pyramid block)."""

    def __init__(self, w1, b1=None, w2=None, b2=None, precision="f32"):
        w1 = _f32c(w1.detach().reshape(w1.shape[0], -1))
        self.cout = int(w1.shape[0])
        if self.cout not in (128, 256):
            raise ValueError("conv1x1 is built for 128 or 256 output channels, got %d" % self.cout)
        self.c1, self.c2 = int(w1.shape[1]), 0
        if w2 is not None:
            w2 = _f32c(w2.detach().reshape(w2.shape[0], -1))
            self.c2 = int(w2.shape[1])
        self.precision = precision
        ctx = get_encoder_context(w1.device)
        self.data = torch.empty((self.cout * (self.c1 + self.c2),), dtype=torch.float32, device=w1.device)
        self.wmax = torch.zeros((1,), dtype=torch.float32, device=w1.device)
        bias = None if b1 is None else b1.detach().float()
        if b2 is not None:
            bias = b2.detach().float() if bias is None else bias + b2.detach().float()
        self.bias = None if bias is None else bias.contiguous()
        ctx.check(ctx.lib.mp_conv1x1_pack(ctx.handle, _ptr(w1), self.c1, _ptr(w2) if w2 is not None else None,
                                          self.c2, self.cout, int(precision == "f16x3"), _ptr(self.data),
                                          _ptr(self.wmax), _stream(w1)), "mp_conv1x1_pack")
        stream = torch.cuda.current_stream(w1.device)
        w1.record_stream(stream)
        if w2 is not None:
            w2.record_stream(stream)


def conv1x1_supported(x):
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] % 64 == 0
            and (x.shape[2] * x.shape[3]) % 64 == 0)


def conv1x1(x1, ss1, relu1, x2, packed, res=None, want_nchw=True, y_hwc=None, want_stats=False):
    """y = W [relu?(x1 * scale + shift) ; x2] + bias (+ res) as one fused GEMM (mp_conv1x1).
    Returns (y [N,Cout,H,W] or None, stats or None); ``y_hwc`` [N,H,W,256] is filled when given."""
    ctx = get_encoder_context(x1.device)
    x1 = x1.contiguous()
    n, c1, h, w = x1.shape
    hw = h * w
    if c1 != packed.c1 or (x2 is None) != (packed.c2 == 0) or (x2 is not None and x2.shape[1] != packed.c2):
        raise ValueError("conv1x1: inputs do not match the packed weights")
    if x2 is not None:
        x2 = x2.contiguous()
    if res is not None:
        res = res.contiguous()
    y = torch.empty((n, packed.cout, h, w), dtype=torch.float32, device=x1.device) if want_nchw else None
    stats = None
    if want_stats:
        s = ctx.lib.mp_conv1x1_stat_slices(hw)
        stats = (torch.empty((n, 32, s, 2), dtype=torch.float64, device=x1.device), s)
    if y_hwc is not None:
        assert y_hwc.is_contiguous() and y_hwc.numel() == n * hw * 256 and y_hwc.dtype == torch.float32
    ctx.check(ctx.lib.mp_conv1x1(
        ctx.handle, _ptr(x1), _ptr(ss1) if ss1 is not None else None, int(bool(relu1)),
        _ptr(x2) if x2 is not None else None, n, c1, packed.c2, packed.cout, hw, _ptr(packed.data),
        int(packed.precision == "f16x3"), _ptr(packed.wmax),
        _ptr(packed.bias) if packed.bias is not None else None,
        _ptr(res) if res is not None else None, _ptr(y) if y is not None else None,
        _ptr(y_hwc) if y_hwc is not None else None, _ptr(stats[0]) if stats else None, _stream(x1)),
        "mp_conv1x1")
    return y, stats


def gn_stats(x, groups):
    """One read pass over x [N,C,H,W]: (partial sums double [N*groups, S, 2], S)."""
    ctx = get_encoder_context(x.device)
    n, c = x.shape[0], x.shape[1]
    hw = x.shape[2] * x.shape[3]
    s = ctx.lib.mp_gn_stat_slices()
    partial = torch.empty((n * groups, s, 2), dtype=torch.float64, device=x.device)
    ctx.check(ctx.lib.mp_gn_stats(ctx.handle, _ptr(x), n, c, hw, int(groups), _ptr(partial),
                                  _stream(x)), "mp_gn_stats")
    return partial, s


def gn_finalize(stats, n, c, groups, count, weight, bias, eps):
    """Partial sums -> ss [N,C,2] = (gamma rstd, beta - mean gamma rstd) of GroupNorm(groups, C)."""
    partial, slices = stats
    ctx = get_encoder_context(partial.device)
    ss = torch.empty((n, c, 2), dtype=torch.float32, device=partial.device)
    ctx.check(ctx.lib.mp_gn_finalize(ctx.handle, _ptr(partial), n, c, int(groups), int(slices),
                                     int(count), _ptr(weight), _ptr(bias), float(eps), _ptr(ss),
                                     _stream(partial)), "mp_gn_finalize")
    return ss


# ---- GroupNorm hand-over from producer to consumer (include/monoport_hip.h, csrc/gn_tail.h) ----
def gn_acc_zeros(device, n, slots=None):
    """Zeroed GroupNorm accumulator(s): int64 [R,N,32,4] (or [slots,R,N,32,4]), R = mp_gn_acc_replicas()."""
    r = _lib.load().mp_gn_acc_replicas()
    shape = (r, n, 32, 4) if slots is None else (slots, r, n, 32, 4)
    return torch.zeros(shape, dtype=torch.int64, device=device)


class GnArena:
    """Accumulators [slots, R, N, 32, 4] int64 for the GroupNorms of one encoder pass, zeroed by ONE fill
    kernel; ``take()`` hands out the next [R,N,32,4] slice.  A producing kernel adds the statistics of
    the tensor it writes into its slice, the consuming kernel reads them (``gn=(acc, module)``)."""

    def __init__(self, device, n, slots):
        self.buf = gn_acc_zeros(device, n, slots)
        self.used = 0
        rec = _recording()
        if rec is not None:  # a replay clears the same arena again
            m = _lib.PlanMemsetArgs()
            m.ptr, m.bytes, m.value = self.buf.data_ptr(), self.buf.numel() * 8, 0
            rec.add(_lib.PLAN_MEMSET, m, [self.buf])

    def take(self):
        if self.used >= self.buf.shape[0]:
            raise RuntimeError("GnArena: more GroupNorms than slots (%d)" % self.buf.shape[0])
        acc = self.buf[self.used]
        self.used += 1
        return acc


def gn_reference_ss(acc, gn, count):
    """(scale, shift) [N,C,2] a consumer derives from an accumulator -- host-side restatement of
    gn_load_stats / gn_scale_shift for tests and probes (not used by the product path)."""
    a = acc.sum(0).to(torch.float64)  # the replicas add up as integers
    lo_s = torch.where(a[..., 1] < 0, a[..., 1] + 2.0 ** 64, a[..., 1])
    lo_q = torch.where(a[..., 3] < 0, a[..., 3] + 2.0 ** 64, a[..., 3])
    s = a[..., 0] / 65536.0 + lo_s / 2.0 ** 64
    q = a[..., 2] / 65536.0 + lo_q / 2.0 ** 64
    mean = s / count
    var = torch.clamp(q / count - mean * mean, min=0.0)
    rstd = (1.0 / torch.sqrt(var + gn.eps)).float()
    mean = mean.float()
    cpg = gn.num_channels // 32
    sc = rstd.repeat_interleave(cpg, 1) * gn.weight[None]
    sh = gn.bias[None] - mean.repeat_interleave(cpg, 1) * sc
    return torch.stack((sc, sh), 2)


def _gn_in(dst, gn, c):
    """Fill a _lib.GnIn: ``gn`` = None (plain input), (acc [N,32,4] int64, GroupNorm module) or a
    precomputed ss [N,C,2] tensor (legacy, from gn_finalize)."""
    if gn is None:
        return
    if torch.is_tensor(gn):
        dst.ss = gn.data_ptr()
        return
    acc, mod = gn
    if mod.num_groups != 32 or mod.num_channels != c:
        raise ValueError("GroupNorm(%d, %d) does not match a %d-channel input" % (mod.num_groups, mod.num_channels, c))
    dst.acc = acc.data_ptr()
    dst.gamma = mod.weight.data_ptr()
    dst.beta = mod.bias.data_ptr()
    dst.eps = float(mod.eps)


def _gn_keep(gn):
    """Tensors a recorded command's GroupNorm input points at (accumulator; the module owns gamma / beta)."""
    if gn is None:
        return []
    if torch.is_tensor(gn):
        return [gn]
    return [gn[0], gn[1].weight, gn[1].bias]


def _gn_out(dst, acc):
    if acc is not None:
        assert acc.dtype == torch.int64 and acc.is_contiguous()
        dst.acc = acc.data_ptr()


def conv3x3_fused(x, gn, packed, relu=True, reflect=False, want_y=True, stats=None, out=None, res=None,
                  out_off=0, out_stats=None):
    """mp_conv3x3_ex: y = conv3x3(relu?(GroupNorm(x))) with the GroupNorm hand-over and, optionally, the
    pyramid block's tail fused into the epilogue.
      gn         GroupNorm of the input: None, (acc, module) or a legacy ss tensor
      stats      accumulator [R,N,32,4] that receives the statistics of y (for the GroupNorm reading y)
      out, res   [N,Ctot,H,W]: out[:, out_off:out_off+Cout] = y + res[:, same]  (cat + residual)
      out_stats  accumulator for GroupNorm(32, Ctot) over ``out`` (shared by the launches filling it)
    Returns y (or None with want_y=False)."""
    ctx = get_encoder_context(x.device)
    n, cin, h, w = x.shape
    if cin != packed.cin:
        raise ValueError("conv3x3: input has %d channels, weights expect %d" % (cin, packed.cin))
    a = _lib.Conv3x3Args()
    y = torch.empty((n, packed.cout, h, w), dtype=torch.float32, device=x.device) if want_y else None
    f16 = packed.precision == "f16x3"
    _gn_in(a.gn, gn, cin)
    _gn_out(a.fin, stats)
    if out is not None:
        assert out.is_contiguous() and res.is_contiguous() and out.shape == res.shape
        _gn_out(a.fin2, out_stats)
        a.y2, a.res = out.data_ptr(), res.data_ptr()
        a.y2_channels, a.y2_offset = out.shape[1], int(out_off)
    a.x, a.n, a.cin, a.h, a.w = x.data_ptr(), n, cin, h, w
    a.relu, a.reflect = int(bool(relu)), int(bool(reflect))
    a.packed = packed.data.data_ptr()
    a.wmax = packed.wmax.data_ptr() if f16 else None
    a.packed_wino = packed.wino.data_ptr() if packed.wino is not None else None
    a.cout = packed.cout
    a.y = y.data_ptr() if y is not None else None
    ctx.check(ctx.lib.mp_conv3x3_ex(ctx.handle, ctypes.byref(a), _stream(x)), "mp_conv3x3_ex")
    rec = _recording()
    if rec is not None:
        rec.add(_lib.PLAN_CONV3X3, a, [x, packed.data, packed.wmax, packed.wino, y, out, res, stats, out_stats] + _gn_keep(gn))
    return y


def conv1x1_fused(x1, gn1, relu1, x2, packed, res=None, want_nchw=True, y_hwc=None, stats=None):
    """mp_conv1x1_ex: ``conv1x1`` with the GroupNorm hand-over (gn1 / stats as in conv3x3_fused).
    Returns y (or None)."""
    ctx = get_encoder_context(x1.device)
    x1 = x1.contiguous()
    n, c1, h, w = x1.shape
    hw = h * w
    if c1 != packed.c1 or (x2 is None) != (packed.c2 == 0) or (x2 is not None and x2.shape[1] != packed.c2):
        raise ValueError("conv1x1: inputs do not match the packed weights")
    a = _lib.Conv1x1Args()
    y = torch.empty((n, packed.cout, h, w), dtype=torch.float32, device=x1.device) if want_nchw else None
    _gn_in(a.gn1, gn1, c1)
    _gn_out(a.fin, stats)
    if y_hwc is not None:
        assert y_hwc.is_contiguous() and y_hwc.numel() == n * hw * 256 and y_hwc.dtype == torch.float32
    a.x1 = x1.data_ptr()
    a.relu1 = int(bool(relu1))
    if x2 is not None:
        x2 = x2.contiguous()
        a.x2 = x2.data_ptr()
    if res is not None:
        res = res.contiguous()
        a.res = res.data_ptr()
    a.n, a.c1, a.c2, a.cout, a.hw = n, c1, packed.c2, packed.cout, hw
    a.packed = packed.data.data_ptr()
    a.f16 = int(packed.precision == "f16x3")
    a.wmax = packed.wmax.data_ptr()
    a.bias = packed.bias.data_ptr() if packed.bias is not None else None
    a.y = y.data_ptr() if y is not None else None
    a.y_hwc = y_hwc.data_ptr() if y_hwc is not None else None
    ctx.check(ctx.lib.mp_conv1x1_ex(ctx.handle, ctypes.byref(a), _stream(x1)), "mp_conv1x1_ex")
    rec = _recording()
    if rec is not None:
        rec.add(_lib.PLAN_CONV1X1, a, [x1, x2, res, packed.data, packed.wmax, packed.bias, y, y_hwc, stats] + _gn_keep(gn1))
    return y


class PackedConvK:
    """Weights of a 7x7 (3 -> 64) or 3x3 stride-2 convolution in the fragment order of
    csrc/convim2col.hip (mp_convk_pack); ``bias`` may be None."""

    def __init__(self, weight, bias=None):
        w = _f32c(weight.detach())
        self.cout, self.cin, self.ks = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        ctx = get_encoder_context(w.device)
        n = ctx.lib.mp_convk_packed_floats(self.cin, self.cout, self.ks)
        if n <= 0 or w.shape[2] != w.shape[3]:
            raise ValueError("PackedConvK: unsupported weight %s" % (tuple(w.shape),))
        self.data = torch.empty((n,), dtype=torch.float32, device=w.device)
        self.bias = None if bias is None else _f32c(bias.detach())
        ctx.check(ctx.lib.mp_convk_pack(ctx.handle, _ptr(w), self.cout, self.cin, self.ks, _ptr(self.data),
                                        _stream(w)), "mp_convk_pack")
        w.record_stream(torch.cuda.current_stream(w.device))


def convk_supported(cin, cout, ks, stride, h, w):
    return bool(_lib.load().mp_convk_supported(int(cin), int(cout), int(ks), int(stride), int(h), int(w)))


def convk(x, gn, relu, packed, stride, reflect=False, stats=None):
    """mp_convk: y = conv_ks(relu?(GroupNorm(x))) (+ bias), stride 1 / 2, padding ks // 2 (zero or
    reflect); gn / stats as in conv3x3_fused.  Returns y."""
    ctx = get_encoder_context(x.device)
    x = x.contiguous()
    n, cin, h, w = x.shape
    a = _lib.ConvKArgs()
    y = torch.empty((n, packed.cout, h // stride, w // stride), dtype=torch.float32, device=x.device)
    _gn_in(a.gn, gn, cin)
    _gn_out(a.fin, stats)
    a.x, a.n, a.cin, a.h, a.w = x.data_ptr(), n, cin, h, w
    a.relu, a.reflect = int(bool(relu)), int(bool(reflect))
    a.packed = packed.data.data_ptr()
    a.bias = packed.bias.data_ptr() if packed.bias is not None else None
    a.cout, a.ks, a.stride = packed.cout, packed.ks, int(stride)
    a.y = y.data_ptr()
    ctx.check(ctx.lib.mp_convk(ctx.handle, ctypes.byref(a), _stream(x)), "mp_convk")
    rec = _recording()
    if rec is not None:
        rec.add(_lib.PLAN_CONVK, a, [x, packed.data, packed.bias, y, stats] + _gn_keep(gn))
    return y


def avgpool2_gn(x, stats=None):
    """F.avg_pool2d(x, 2, stride=2), adding the statistics of the result into ``stats``."""
    ctx = get_encoder_context(x.device)
    x = x.contiguous()
    n, c, h, w = x.shape
    y = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    fin = _lib.GnOut()
    _gn_out(fin, stats)
    ctx.check(ctx.lib.mp_avgpool2_gn(ctx.handle, _ptr(x), n, c, h, w, _ptr(y), ctypes.byref(fin), _stream(x)),
              "mp_avgpool2_gn")
    rec = _recording()
    if rec is not None:
        a = _lib.PlanPoolArgs()
        a.x, a.n, a.c, a.h, a.w, a.y, a.fin = x.data_ptr(), n, c, h, w, y.data_ptr(), fin
        rec.add(_lib.PLAN_AVGPOOL2, a, [x, y, stats])
    return y


def upsample_add_gn(x, add, stats=None):
    """add + bicubic x2 of x (HGFilters.py:108-111), adding the statistics of the result into ``stats``."""
    ctx = get_encoder_context(x.device)
    x = x.contiguous()
    n, c, h, w = x.shape
    y = torch.empty((n, c, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    if add is not None:
        add = add.contiguous()
    fin = _lib.GnOut()
    _gn_out(fin, stats)
    ctx.check(ctx.lib.mp_upsample_bicubic2x_gn(ctx.handle, _ptr(x), n, c, h, w,
                                               _ptr(add) if add is not None else None, _ptr(y),
                                               ctypes.byref(fin), _stream(x)), "mp_upsample_bicubic2x_gn")
    rec = _recording()
    if rec is not None:
        a = _lib.PlanUpsampleArgs()
        a.x, a.n, a.c, a.h, a.w, a.y, a.fin = x.data_ptr(), n, c, h, w, y.data_ptr(), fin
        a.add = add.data_ptr() if add is not None else None
        rec.add(_lib.PLAN_UPSAMPLE2X, a, [x, add, y, stats])
    return y


def upsample_banded(c, h, w):
    """True if ``upsample_add_gn`` runs an [N,c,h,w] input on the banded kernel, False if on the one-output-per-thread
    kernel (mp_upsample_gn_banded: the launcher's own rule)."""
    return bool(_lib.load().mp_upsample_gn_banded(int(c), int(h), int(w)))


def gn_apply(x, gn, relu=True, res=None, stats=None):
    """[res +] relu?(GroupNorm(x)) materialised (gn = (acc, module) or a legacy ss tensor), adding the
    statistics of the result into ``stats``."""
    ctx = get_encoder_context(x.device)
    x = x.contiguous()
    n, c = x.shape[0], x.shape[1]
    hw = x.shape[2] * x.shape[3]
    y = torch.empty_like(x)
    g = _lib.GnIn()
    _gn_in(g, gn, c)
    fin = _lib.GnOut()
    _gn_out(fin, stats)
    if res is not None:
        res = res.contiguous()
    ctx.check(ctx.lib.mp_gn_apply(ctx.handle, _ptr(x), ctypes.byref(g), int(bool(relu)), n, c, hw,
                                  _ptr(res) if res is not None else None, _ptr(y), ctypes.byref(fin),
                                  _stream(x)), "mp_gn_apply")
    rec = _recording()
    if rec is not None:
        a = _lib.PlanGnApplyArgs()
        a.x, a.gn, a.relu, a.n, a.c, a.hw, a.y, a.fin = x.data_ptr(), g, int(bool(relu)), n, c, hw, y.data_ptr(), fin
        a.res = res.data_ptr() if res is not None else None
        rec.add(_lib.PLAN_GN_APPLY, a, [x, res, y, stats] + _gn_keep(gn))
    return y


def memory_stats(device):
    """mp_memory_stats: device memory the contexts of ``device`` own (scratch arenas incl. outgrown blocks, packed MLP
    weights) and how many arenas / registered skip tables it tracks."""
    tot = [0, 0, 0, 0]
    for ctx in (get_context(device), get_encoder_context(device)):
        out = (ctypes.c_int64 * 4)()
        ctx.check(ctx.lib.mp_memory_stats(ctx.handle, out), "mp_memory_stats")
        tot = [a + int(b) for a, b in zip(tot, out)]
    return {"arena_bytes": tot[0], "weight_bytes": tot[1], "arenas": tot[2], "skip_tables": tot[3]}


def scratch_fill(device, nbytes, byte, role="query"):
    """mp_scratch_fill (a test hook): grow the scratch arena that the ``role`` ("query" | "encoder") context of
    ``device`` keeps for torch's current stream to at least ``nbytes``, set every byte of its current block to ``byte``
    on that stream, and return the block's size.  The next stage on the stream then starts on that residue."""
    if role not in ("query", "encoder"):
        raise ValueError("role must be 'query' or 'encoder', got %r" % (role,))
    ctx = get_context(device) if role == "query" else get_encoder_context(device)
    block = ctypes.c_int64(0)
    st = torch.cuda.current_stream(torch.device(device))
    ctx.check(ctx.lib.mp_scratch_fill(ctx.handle, int(nbytes), int(byte), ctypes.byref(block),
                                      ctypes.c_void_p(st.cuda_stream)), "mp_scratch_fill")
    return int(block.value)


def mfma_clock_probe(device, ms_target=20.0, stream=None):
    """What the f32 matrix pipe of ``device`` sustains right now (mp_mfma_clock_probe, csrc/clock_probe.hip):
    {"tflops", "shader_clock_mhz", "ms", "workgroups"} of a register-only MFMA loop of about ``ms_target`` ms."""
    ctx = get_context(device)
    out = (ctypes.c_double * 4)()
    st = stream if stream is not None else torch.cuda.current_stream(torch.device(device))
    ctx.check(ctx.lib.mp_mfma_clock_probe(ctx.handle, float(ms_target), out, ctypes.c_void_p(st.cuda_stream)),
              "mp_mfma_clock_probe")
    return {"tflops": out[0], "shader_clock_mhz": out[1], "ms": out[2], "workgroups": int(out[3])}


def profile_begin(device, max_records=4096):
    """Start bracketing fused-query launches on ``device`` with HIP events (bench.py roofline)."""
    ctx = get_context(device)
    ctx.check(ctx.lib.mp_profile_begin(ctx.handle, int(max_records)), "mp_profile_begin")


def profile_end(device, capacity=4096):
    """Stop and return the per-launch durations (ms, launch order) as a numpy array."""
    ctx = get_context(device)
    buf = (ctypes.c_float * capacity)()
    n = ctypes.c_int(0)
    ctx.check(ctx.lib.mp_profile_end(ctx.handle, buf, capacity, ctypes.byref(n)), "mp_profile_end")
    return np.array(buf[:min(n.value, capacity)], dtype=np.float64)
