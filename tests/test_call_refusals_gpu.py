"""The refusals of the query / reconstruction entry points, pinned: status code and message of every malformed call,
through the C-ABI directly (``_lib.load()``) and through the ``ops`` wrappers.  Needs an MI355X (a context).

Nothing here is launched: every row is one call that csrc/api.hip refuses in its argument checks, which all sit
before the entry point's first launch and before its scratch allocation (read the bodies: each one ends in
``DeviceGuard`` + ``launch_*`` / ``ensure_scratch`` only after the last check), or that the Python wrapper refuses
before it reaches the library.  Apart from its one fault every row is a well-formed call on real buffers of the
right size, and rows are single-fault: the order of two refusals of one call is not specified by the header.

The two deliberate accept-cases pin where an EMPTY call returns relative to the per-frame null checks:
mp_query_batch looks at the frames first (a null map with n = 0 is refused), mp_query_counted_batch_proj returns
first (a null map with capacity = 0 is MP_OK)."""
import ctypes

import pytest

from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, -1, -3  # MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED (include/monoport_hip.h)
H = W = 8
N = 64          # points / capacity
V = 3           # frames / views of a well-formed call
RES = [17, 33]
MAX_FRAMES, MAX_VIEWS = 32, 8

# C signatures after the context (include/monoport_hip.h), by argument name
ORDER = {
    "mp_query": "mlp feat c h w points n sn sc calib z out stream",
    "mp_query_batch": "mlp count feats c h w pointss n sn sc calibs projs z outs stream",
    "mp_mlp_forward": "mlp feature n out stream",
    "mp_query_views": "mlp count feats c h w pointss n sn sc calibs proj z outs stream",
    "mp_mlp_forward_views": "mlp count feature n out stream",
    "mp_query_counted": "mlp feat c h w points n npts calib z out stream",
    "mp_query_counted_batch_proj": "mlp count feats c h w pointss n nptss calibs projs z outs stream",
    "mp_recon_batch_proj": "mlp count feats c h w calibs projs z bmin bmax res levels balance final vols stats early "
                           "stream",
    "mp_recon_views": "mlp count feats c h w calibs proj z bmin bmax res levels balance final view vol stat early "
                      "stream",
}
BATCHED = ["mp_query_batch", "mp_query_counted_batch_proj", "mp_recon_batch_proj"]
VIEWS = ["mp_query_views", "mp_recon_views"]
WITH_MAP = ["mp_query", "mp_query_counted"] + BATCHED + VIEWS
RECON = ["mp_recon_batch_proj", "mp_recon_views"]


def ptrs(tensors, n=None):
    """void*[n] of the tensors' addresses (None -> NULL), the list repeated up to n entries."""
    tensors = list(tensors)
    picked = [tensors[i % len(tensors)] for i in range(len(tensors) if n is None else n)]
    return (ctypes.c_void_p * len(picked))(*[None if t is None else t.data_ptr() for t in picked])


def ints(values):
    return (ctypes.c_int * len(values))(*values)


class Env:
    """Heads, buffers and the well-formed arguments of every entry point."""

    def __init__(self):
        from monoport_amd import _lib, ops
        self.ops, self.lib_mod = ops, _lib
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        self.g = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("G", 61, 2.0), 1)
        self.g16 = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("G", 61, 2.0), 1)
        self.g16.set_precision("f16x3")
        self.netc = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("C", 3, 1.0), 2)  # C = 512, 3 outputs
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
        self.maps = [z(H, W, 256) for _ in range(V)]
        self.maps512 = [z(H, W, 512) for _ in range(V)]
        # a [H,W,C] view 4 bytes into a larger allocation: contiguous float32, not 16-byte aligned
        self.big = z(H * W * 256 + 4)
        self.misaligned = self.big[1:1 + H * W * 256].view(H, W, 256)
        assert self.misaligned.data_ptr() % 16 == 4 and self.misaligned.is_contiguous()
        self.points = z(V, 3, N)
        self.outs = z(V, 1, N)
        self.outs3 = z(V, 3, N)
        self.counts = [z(1, dtype=torch.int32) for _ in range(V)]
        self.calibs = torch.eye(4, device=DEV)[None].repeat(V, 1, 1).contiguous()
        self.feature = z(V, 257, N)
        self.vols = [z(RES[-1], RES[-1], RES[-1]) for _ in range(V)]
        self.stats = z(V, 1 + len(RES), dtype=torch.int32)
        self.level0 = z(RES[0], RES[0], RES[0])
        self.bmin, self.bmax = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def defaults(self, name):
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        count = V
        d = dict(mlp=self.g.id, count=count, c=256, h=H, w=W, n=N, sn=1, sc=N, z=1.0, proj=0, stream=self.stream,
                 feat=p(self.maps[0]), points=p(self.points[0]), calib=p(self.calibs[0]), out=p(self.outs[0]),
                 npts=p(self.counts[0]), feature=p(self.feature), feats=ptrs(self.maps), pointss=ptrs(self.points),
                 calibs=ptrs(self.calibs), projs=ints([0] * count), outs=ptrs(self.outs), nptss=ptrs(self.counts),
                 bmin=self.bmin, bmax=self.bmax, res=ints(RES), levels=len(RES), balance=0.5, final=0, view=0,
                 vols=ptrs(self.vols), stats=ptrs(self.stats), vol=p(self.vols[0]), stat=p(self.stats[0]), early=None)
        return {k: d[k] for k in ORDER[name].split()}

    def raw(self, name, **over):
        """-> (status code, message) of one direct call with ``over`` replacing well-formed arguments."""
        a = self.defaults(name)
        assert set(over) <= set(a), (name, sorted(over))
        a.update(over)
        rc = getattr(self.lib, name)(self.ctx.handle, *[a[k] for k in ORDER[name].split()])
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()

    def early(self, flags_dev=True):
        e = self.ops.EarlyFlags(DEV, 1)
        st = e.struct(None)
        if not flags_dev:
            st.flags_dev = None
        self._keep = (e, st)
        return ctypes.byref(st)


@pytest.fixture(scope="module")
def env():
    return Env()


def what(name):
    return "view" if name in VIEWS or name == "mp_mlp_forward_views" else "frame"


def reported(name):
    """The name an entry point's messages carry."""
    return {"mp_query_counted_batch_proj": "mp_query_counted_batch"}.get(name, name)


# (row id, entry point, overrides as a function of the Env, status code, part of the message)
RAW = []


def row(rid, name, over, code, text):
    RAW.append(pytest.param(name, over, code, text, id="%s-%s" % (name, rid)))


for _n in BATCHED + VIEWS + ["mp_mlp_forward_views"]:
    _most = MAX_VIEWS if what(_n) == "view" else MAX_FRAMES
    _code = UNSUPPORTED if what(_n) == "view" else ARG
    # mp_recon_batch_proj reports under one name since the entry points were consolidated: the name is pinned by
    # the `one-name` rows below, the other rows of it match the text after the name
    _who = "" if _n == "mp_recon_batch_proj" else reported(_n)
    row("count0", _n, lambda e: dict(count=0), _code, "%s: 1..%d %ss per call, got 0" % (_who, _most, what(_n)))
    row("count-max+1", _n, lambda e, m=_most, n=_n: dict(
        count=m + 1, **({} if n == "mp_mlp_forward_views" else dict(feats=ptrs(e.maps, m + 1), calibs=ptrs(e.calibs, m + 1)))),
        _code, "%s: 1..%d %ss per call, got %d" % (_who, _most, what(_n), _most + 1))
for _n in BATCHED + VIEWS:
    _who = "" if _n == "mp_recon_batch_proj" else reported(_n)
    row("null-array", _n, lambda e: dict(feats=None), ARG, _who + ": bad argument")
    row("null-item1", _n, lambda e: dict(feats=ptrs([e.maps[0], None, e.maps[2]])), ARG,
        "%s: null buffer for %s 1" % (_who, what(_n)))
    row("null-calib2", _n, lambda e: dict(calibs=ptrs([e.calibs[0], e.calibs[1], None])), ARG,
        "%s: null buffer for %s 2" % (_who, what(_n)))
    row("misaligned-item1", _n, lambda e: dict(feats=ptrs([e.maps[0], e.misaligned, e.maps[2]])), ARG,
        _who + ": feat_hwc must be 16-byte aligned")
    row("h0", _n, lambda e: dict(h=0), ARG, _who + ": bad argument")
    row("w-negative", _n, lambda e: dict(w=-1), ARG, _who + ": bad argument")
for _n in ["mp_query", "mp_query_counted"]:
    row("null-map", _n, lambda e: dict(feat=None), ARG, _n + ": bad argument")
    row("misaligned", _n, lambda e: dict(feat=ctypes.c_void_p(e.misaligned.data_ptr())), ARG,
        _n + ": feat_hwc must be 16-byte aligned")
    row("h0", _n, lambda e: dict(h=0), ARG, _n + ": bad argument")
    row("null-calib", _n, lambda e: dict(calib=None), ARG, _n + ": bad argument")
    row("null-points", _n, lambda e: dict(points=None), ARG, _n + ": bad argument")
for _n in WITH_MAP:
    row("unknown-head", _n, lambda e: dict(mlp=99), ARG, "unknown mlp id")
    row("head-width", _n, lambda e: dict(c=512), ARG, "feature map has C=512 but the mlp was built for C=256")
row("unknown-head", "mp_mlp_forward", lambda e: dict(mlp=99), ARG, "mp_mlp_forward: unknown mlp id 99")
row("unknown-head", "mp_mlp_forward_views", lambda e: dict(mlp=99), ARG, "mp_mlp_forward_views: unknown mlp id 99")
row("null-feature", "mp_mlp_forward", lambda e: dict(feature=None), ARG, "mp_mlp_forward: bad argument")
row("null-out", "mp_mlp_forward_views", lambda e: dict(out=None), ARG, "mp_mlp_forward_views: bad argument")
row("negative-n", "mp_query", lambda e: dict(n=-1), ARG, "mp_query: bad argument")
row("null-count", "mp_query_counted", lambda e: dict(npts=None), ARG, "mp_query_counted: bad argument")
for _n in BATCHED:
    _who = "" if _n == "mp_recon_batch_proj" else reported(_n)
    row("projection7", _n, lambda e: dict(projs=ints([0, 7, 0])), ARG, _who + ": frame 1 has projection 7")
for _n in VIEWS:
    row("projection7", _n, lambda e: dict(proj=7), ARG, _n + ": frame 0 has projection 7")
row("null-projections", "mp_query_batch", lambda e: dict(projs=None), ARG, "mp_query_batch: bad argument")
for _n in VIEWS + ["mp_mlp_forward_views"]:
    row("f16x3-head", _n, lambda e: dict(mlp=e.g16.id), UNSUPPORTED, _n + ": the multi-view kernel is f32 only")
row("view-3-of-3", "mp_recon_views", lambda e: dict(view=V), ARG, "mp_recon_views: view 3 outside 0..2")
row("view-negative", "mp_recon_views", lambda e: dict(view=-1), ARG, "mp_recon_views: view -1 outside 0..2")
for _n, _code in [("mp_recon_batch_proj", UNSUPPORTED), ("mp_recon_views", ARG)]:  # the two families' own codes
    _who = "" if _n == "mp_recon_batch_proj" else _n
    row("final7", _n, lambda e: dict(final=7), ARG, _who + ": final_level must be MP_FINAL_DILATE3 / _UPSTREAM / "
        "_INTERPOLATE, got 7")
    row("res-17-34", _n, lambda e: dict(res=ints([17, 34])), _code,
        _who + ": resolutions must follow r -> 2r-1 (got 34 after 17)")
    row("res-1", _n, lambda e: dict(res=ints([1]), levels=1), _code, _who + ": resolution 1 outside [2,1023]")
    row("levels0", _n, lambda e: dict(levels=0), ARG, _who + ": bad argument")
    row("levels9", _n, lambda e: dict(levels=9), ARG, _who + ": bad argument")
    row("null-bmin", _n, lambda e: dict(bmin=None), ARG, _who + ": bad argument")
    row("early-null-flags", _n, lambda e: dict(early=e.early(flags_dev=False)), ARG, "flags_host are required")
row("null-volume1", "mp_recon_batch_proj", lambda e: dict(vols=ptrs([e.vols[0], None, e.vols[2]])), ARG,
    ": null buffer for frame 1")
row("null-volume", "mp_recon_views", lambda e: dict(vol=None), ARG, "mp_recon_views: bad argument")
row("netC-head", "mp_recon_batch_proj", lambda e: dict(mlp=e.netc.id, c=512, feats=ptrs(e.maps512)), ARG,
    ": needs a 1-channel (occupancy) mlp")
row("netC-head", "mp_recon_views", lambda e: dict(mlp=e.netc.id, c=512, feats=ptrs(e.maps512)), UNSUPPORTED,
    "mp_recon_views: needs a netG head (C=256, 1 occupancy channel); got C=512 Cout=3")
# where an empty call returns (module docstring)
row("empty-null-map", "mp_query_batch", lambda e: dict(n=0, feats=ptrs([e.maps[0], None, e.maps[2]])), ARG,
    "mp_query_batch: null buffer for frame 1")
row("empty-null-points-ok", "mp_query_batch", lambda e: dict(n=0, pointss=ptrs([None] * V), outs=ptrs([None] * V)), OK,
    "")
row("empty-null-map-ok", "mp_query_counted_batch_proj", lambda e: dict(n=0, feats=ptrs([e.maps[0], None, e.maps[2]])),
    OK, "")
row("empty-h0", "mp_query_counted_batch_proj", lambda e: dict(n=0, h=0), ARG, "mp_query_counted_batch: bad argument")
# the one name mp_recon, mp_recon_batch, _ex, _early and _proj report under
row("one-name-count", "mp_recon_batch_proj", lambda e: dict(count=0), ARG, "mp_recon_batch_proj: 1..32 frames")
row("one-name-early", "mp_recon_batch_proj", lambda e: dict(early=e.early(flags_dev=False)), ARG,
    "mp_recon_batch_proj: flags_dev and flags_host are required")


@pytest.mark.parametrize("name,over,code,text", RAW)
def test_c_abi_refusal(env, name, over, code, text):
    rc, msg = env.raw(name, **over(env))
    print("%s -> %d %r" % (name, rc, msg if rc else ""))
    assert rc == code
    if code != OK:
        assert text in msg


def test_the_older_recon_entry_points_share_the_refusals(env):
    """mp_recon / mp_recon_batch / _ex / _early are mp_recon_batch_proj with defaults: same code for the same fault."""
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    lib, h = env.lib, env.ctx.handle
    bad = ints([17, 34])
    one = (p(env.maps[0]), 256, H, W, p(env.calibs[0]), 1.0, env.bmin, env.bmax, bad, 2, 0.5)
    many = (V, ptrs(env.maps), 256, H, W, ptrs(env.calibs), 1.0, env.bmin, env.bmax, bad, 2, 0.5)
    out = (ptrs(env.vols), ptrs(env.stats))
    assert lib.mp_recon(h, env.g.id, *one, p(env.vols[0]), p(env.stats[0]), env.stream) == UNSUPPORTED
    assert lib.mp_recon_batch(h, env.g.id, *many, *out, env.stream) == UNSUPPORTED
    assert lib.mp_recon_batch_ex(h, env.g.id, *many, 0, *out, env.stream) == UNSUPPORTED
    assert lib.mp_recon_batch_early(h, env.g.id, *many, 0, *out, None, env.stream) == UNSUPPORTED
    assert "resolutions must follow r -> 2r-1 (got 34 after 17)" in lib.mp_last_error(h).decode()
    assert lib.mp_query_counted_batch(h, env.g.id, MAX_FRAMES + 1, ptrs(env.maps, MAX_FRAMES + 1), 256, H, W,
                                      ptrs(env.points), N, ptrs(env.counts), ptrs(env.calibs), 1.0, ptrs(env.outs),
                                      env.stream) == ARG
    assert "mp_query_counted_batch: 1..32 frames per call, got 33" in lib.mp_last_error(h).decode()


# ---- through the ops wrappers: what the library refuses surfaces as MonoportError "... failed (code): message" ----
def _wrapped():
    box = ([-1, -1, -1], [1, 1, 1])
    rows = [
        ("query-misaligned", lambda e: e.ops.query(e.g, e.misaligned, e.points[:1], e.calibs[0], 1.0), ARG,
         "mp_query: feat_hwc must be 16-byte aligned"),
        ("query_batch-misaligned", lambda e: e.ops.query_batch(e.g, [e.maps[0], e.misaligned], e.points[:2], e.calibs[:2],
                                                               [0, 0], 1.0), ARG, "mp_query_batch: feat_hwc must be"),
        ("query_views-f16x3", lambda e: e.ops.query_views(e.g16, e.maps, e.points, e.calibs, 0, 1.0), UNSUPPORTED,
         "mp_query_views: the multi-view kernel is f32 only"),
        ("mlp_forward_views-f16x3", lambda e: e.ops.mlp_forward_views(e.g16, e.feature), UNSUPPORTED,
         "mp_mlp_forward_views: the multi-view kernel is f32 only"),
        ("query_counted_batch-33", lambda e: e.ops.query_counted_batch(
            e.g, [e.maps[0]] * 33, [e.points[0]] * 33, [e.counts[0]] * 33, [e.calibs[0]] * 33, 1.0), ARG,
         "mp_query_counted_batch: 1..32 frames per call, got 33"),
        ("query_counted_batch-head-width", lambda e: e.ops.query_counted_batch(
            e.g, e.maps512, list(e.points), e.counts, list(e.calibs), 1.0), ARG, "feature map has C=512"),
        ("recon-res-17-34", lambda e: e.ops.recon(e.g, e.maps[0], e.calibs[0], 1.0, *box, [17, 34]), UNSUPPORTED,
         "resolutions must follow r -> 2r-1 (got 34 after 17)"),
        ("recon-res-1", lambda e: e.ops.recon(e.g, e.maps[0], e.calibs[0], 1.0, *box, [1]), UNSUPPORTED,
         "resolution 1 outside [2,1023]"),
        ("recon-netC", lambda e: e.ops.recon(e.netc, e.maps512[0], e.calibs[0], 1.0, *box, RES), ARG,
         "needs a 1-channel (occupancy) mlp"),
        ("recon-misaligned", lambda e: e.ops.recon(e.g, e.misaligned, e.calibs[0], 1.0, *box, RES), ARG,
         "feat_hwc must be 16-byte aligned"),
        ("recon_batch-33", lambda e: e.ops.recon_batch(e.g, [e.maps[0]] * 33, [e.calibs[0]] * 33, 1.0, *box, RES), ARG,
         "1..32 frames per call, got 33"),
        ("recon_views-res-17-34", lambda e: e.ops.recon_views(e.g, e.maps, e.calibs, 0, 1.0, *box, [17, 34]), ARG,
         "mp_recon_views: resolutions must follow r -> 2r-1 (got 34 after 17)"),
        ("recon_views-res-1", lambda e: e.ops.recon_views(e.g, e.maps, e.calibs, 0, 1.0, *box, [1]), ARG,
         "mp_recon_views: resolution 1 outside [2,1023]"),
        ("recon_views-view3", lambda e: e.ops.recon_views(e.g, e.maps, e.calibs, 0, 1.0, *box, RES, view=3), ARG,
         "mp_recon_views: view 3 outside 0..2"),
        ("recon_views-f16x3", lambda e: e.ops.recon_views(e.g16, e.maps, e.calibs, 0, 1.0, *box, RES), UNSUPPORTED,
         "mp_recon_views: the multi-view kernel is f32 only"),
        ("recon_views-netC", lambda e: e.ops.recon_views(e.netc, e.maps512, e.calibs, 0, 1.0, *box, RES), UNSUPPORTED,
         "mp_recon_views: needs a netG head"),
    ]
    return [pytest.param(fn, code, text, id=rid) for rid, fn, code, text in rows]


@pytest.mark.parametrize("call,code,text", _wrapped())
def test_wrapper_surfaces_the_refusal(env, call, code, text):
    with pytest.raises(env.lib_mod.MonoportError) as err:
        call(env)
    print(err.value)
    assert "(%d)" % code in str(err.value) and text in str(err.value)


# ---- what the wrappers refuse themselves: ValueError naming the function, before the library is reached ----
def _python_side():
    box = ([-1, -1, -1], [1, 1, 1])
    nc = lambda t: t.transpose(0, 1)  # noqa: E731  (a non-contiguous view of a square-faced tensor)
    rows = [
        ("query_batch-count0", "query_batch", lambda e: e.ops.query_batch(e.g, [], e.points[:0], [], [], 1.0)),
        ("query_batch-count33", "query_batch", lambda e: e.ops.query_batch(
            e.g, [e.maps[0]] * 33, e.points[:1].expand(33, 3, N), [e.calibs[0]] * 33, [0] * 33, 1.0)),
        ("query_batch-map-shape", "query_batch", lambda e: e.ops.query_batch(
            e.g, [e.maps[0], e.maps512[1]], e.points[:2], e.calibs[:2], [0, 0], 1.0)),
        ("query_batch-map-strides", "query_batch", lambda e: e.ops.query_batch(
            e.g, [e.maps[0], nc(e.maps[1])], e.points[:2], e.calibs[:2], [0, 0], 1.0)),
        ("query_batch-map-dtype", "query_batch", lambda e: e.ops.query_batch(
            e.g, [e.maps[0], e.maps[1].double()], e.points[:2], e.calibs[:2], [0, 0], 1.0)),
        ("query_batch-calibs", "query_batch", lambda e: e.ops.query_batch(
            e.g, e.maps, e.points, e.calibs[:2], [0] * V, 1.0)),
        ("query_batch-projections", "query_batch", lambda e: e.ops.query_batch(
            e.g, e.maps, e.points, e.calibs, [0, 0], 1.0)),
        ("query_batch-out", "query_batch", lambda e: e.ops.query_batch(
            e.g, e.maps, e.points, e.calibs, [0] * V, 1.0, out=e.outs3)),
        ("query_views-count9", "query_views", lambda e: e.ops.query_views(
            e.g, [e.maps[0]] * 9, e.points[:1].expand(9, 3, N), [e.calibs[0]] * 9, 0, 1.0)),
        ("query_views-calibs", "query_views", lambda e: e.ops.query_views(e.g, e.maps, e.points, e.calibs[:2], 0, 1.0)),
        ("query_views-map-shape", "query_views", lambda e: e.ops.query_views(
            e.g, [e.maps[0], e.maps512[1], e.maps[2]], e.points, e.calibs, 0, 1.0)),
        ("query_views-out", "query_views", lambda e: e.ops.query_views(
            e.g, e.maps, e.points, e.calibs, 0, 1.0, out=e.outs.double())),
        # AssertionError before the wrappers were consolidated
        ("query_counted_batch-map-shape", "query_counted_batch", lambda e: e.ops.query_counted_batch(
            e.g, [e.maps[0], e.maps512[1]], list(e.points[:2]), e.counts[:2], list(e.calibs[:2]), 1.0)),
        ("query_counted_batch-points-strides", "query_counted_batch", lambda e: e.ops.query_counted_batch(
            e.g, e.maps[:1], [torch.zeros(N, 3, device=DEV).t()], e.counts[:1], [e.calibs[0]], 1.0)),
        ("query_counted_batch-projections", "query_counted_batch", lambda e: e.ops.query_counted_batch(
            e.g, e.maps, list(e.points), e.counts, list(e.calibs), 1.0, projections=[0])),
        ("recon_batch-status-shape", "recon_batch", lambda e: e.ops.recon_batch(
            e.g, e.maps, e.calibs, 1.0, *box, RES, status=e.stats[:2])),
        ("recon_batch-map-strides", "recon_batch", lambda e: e.ops.recon_batch(
            e.g, [e.maps[0], nc(e.maps[1])], e.calibs[:2], 1.0, *box, RES)),
        ("recon_batch-map-dtype", "recon_batch", lambda e: e.ops.recon_batch(
            e.g, [e.maps[0].double()], e.calibs[:1], 1.0, *box, RES)),
        ("recon_batch-expect-size", "recon_batch", lambda e: e.ops.recon_batch(
            e.g, e.maps[:1], e.calibs[:1], 1.0, *box, RES, early=e.ops.EarlyFlags(DEV, 1), expect_level0=[e.vols[0]])),
        ("recon_views-expect-size", "recon_views", lambda e: e.ops.recon_views(
            e.g, e.maps, e.calibs, 0, 1.0, *box, RES, early=e.ops.EarlyFlags(DEV, 1), expect_level0=e.vols[0])),
        # not checked at all before: a [1,4,4] tensor for two frames (never a short LIST against the old wrapper --
        # its pointer array would be read past the end)
        ("recon_batch-calibs", "recon_batch", lambda e: e.ops.recon_batch(e.g, e.maps[:2], e.calibs[:1], 1.0, *box, RES)),
        ("recon_batch-projections", "recon_batch", lambda e: e.ops.recon_batch(
            e.g, e.maps, e.calibs, 1.0, *box, RES, projections=[0])),
        ("recon_batch-early-frames", "recon_batch", lambda e: e.ops.recon_batch(
            e.g, e.maps, e.calibs, 1.0, *box, RES, early=e.ops.EarlyFlags(DEV, 2))),
        ("recon_views-count9", "recon_views", lambda e: e.ops.recon_views(
            e.g, [e.maps[0]] * 9, [e.calibs[0]] * 9, 0, 1.0, *box, RES)),
        ("recon_views-count0", "recon_views", lambda e: e.ops.recon_views(e.g, [], [], 0, 1.0, *box, RES)),
        ("recon_views-calibs", "recon_views", lambda e: e.ops.recon_views(e.g, e.maps, e.calibs[:2], 0, 1.0, *box, RES)),
        ("recon_views-map-dtype", "recon_views", lambda e: e.ops.recon_views(
            e.g, [e.maps[0], e.maps[1].double(), e.maps[2]], e.calibs, 0, 1.0, *box, RES)),
        ("recon_views-early-frames", "recon_views", lambda e: e.ops.recon_views(
            e.g, e.maps, e.calibs, 0, 1.0, *box, RES, early=e.ops.EarlyFlags(DEV, 2))),
    ]
    return [pytest.param(who, fn, id=rid) for rid, who, fn in rows]


@pytest.mark.parametrize("who,call", _python_side())
def test_wrapper_refuses_with_value_error(env, who, call):
    with pytest.raises(ValueError) as err:
        call(env)
    print(err.value)
    assert who in str(err.value)
