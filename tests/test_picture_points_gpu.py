"""mp_picture_points / mp_picture_paint (csrc/picture.hip) and ops.picture_points(_batch) / ops.picture_paint(_batch) on
the GPU, bit for bit against the numpy restatement of the definition (tests/picture_ref.py): the covered pixels of
rendered and of synthetic pictures as counted lists in ascending pixel order, truncation, batches, the scatter back,
the refusals of the four entry points, and a scratch arena that starts dirty.  Needs an MI355X."""
import ctypes
import math

import numpy as np
import pytest

import picture_ref as ref
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, -1, -3  # MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED (include/monoport_hip.h)
INF = math.inf
FPOISON, IPOISON = -12345.0, -777  # what the output buffers hold before a call
FILLS = (0x00, 0xFF, 0x7F, 0x5A)


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _rotated():
    a, b = np.deg2rad(30.0), np.deg2rad(20.0)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = 0.9 * (rx @ ry)
    m[:3, 3] = [0.05, -0.1, 0.0]
    return m


def _perspective():
    m = np.eye(4, dtype=np.float32)
    m[0, 0] = m[1, 1] = 2.5
    m[:3, 3] = [0.2, -0.1, 3.0]  # the body at z = 2.3 .. 3.6, in front of the camera
    return m


CAMERAS = {"identity": (np.eye(4, dtype=np.float32), "orthogonal"), "rotated": (_rotated(), "orthogonal"),
           "perspective": (_perspective(), "perspective")}
SIZES = [(33, 33), (40, 24)]


def _views(cam, n_views):
    """The named camera and, for three views, two more of its kind: one shifted, one zoomed out."""
    m, projection = CAMERAS[cam]
    views = [m]
    if n_views == 3:
        shifted, wide = m.copy(), m.copy()
        shifted[0, 3] += 0.15
        wide[:2] *= 0.8
        views += [shifted, wide]
    return torch.from_numpy(np.stack(views)), projection


@pytest.fixture(scope="module")
def body33(ops):
    """The device's own marching cubes of blob_volume(33, 5): the body of test_mesh_render_gpu.py."""
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    verts, faces, counts = ops.marching_cubes_raw(vol)
    return dict(verts=verts, faces=faces, counts=counts, pictures={})


def rendered(ops, body33, cam, size, n_views):
    """(face ids [n_views,H,W], positions [n_views,H,W,3]) of the body: ops.mesh_render_raw with attr = verts."""
    key = (cam, size, n_views)
    if key not in body33["pictures"]:
        calibs, projection = _views(cam, n_views)
        b = body33
        image, _, face = ops.mesh_render_raw(b["verts"], b["faces"], b["counts"], b["verts"], calibs, size, projection,
                                             "max" if projection == "orthogonal" else "min", background=0.25)
        body33["pictures"][key] = (face, image)
    return body33["pictures"][key]


GUARD = 5


def poisoned(n, capacity):
    """Per-frame (points [3,capacity], pixels [capacity], count [2]) full of poison, each the front of a row that is
    GUARD words longer -> (the three lists of frames, the three larger tensors)."""
    big = (torch.full((n, 3 * capacity + GUARD), FPOISON, device=DEV),
           torch.full((n, capacity + GUARD), IPOISON, dtype=torch.int32, device=DEV),
           torch.full((n, 2 + GUARD), IPOISON, dtype=torch.int32, device=DEV))
    out = ([row[:3 * capacity].view(3, capacity) for row in big[0]], [row[:capacity] for row in big[1]],
           [row[:2] for row in big[2]])
    return out, big


def guards_untouched(big, capacity):
    return (bool((big[0][:, 3 * capacity:] == FPOISON).all()) and bool((big[1][:, capacity:] == IPOISON).all())
            and bool((big[2][:, 2:] == IPOISON).all()))


def want_points(face, pos, capacity):
    """The restatement into poisoned buffers: columns at or beyond count[0] keep the poison."""
    pts = np.full((3, capacity), FPOISON, np.float32)
    pix = np.full(capacity, IPOISON, np.int32)
    return ref.points(host(face), host(pos), capacity, pts, pix)


def host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def check_points(ops, faces, positions, capacity=None, what=""):
    """ops.picture_points_batch of the frames into poisoned buffers against the restatement, whole buffers on the bits;
    -> the device's (points, pixels, count) per frame."""
    n = len(faces)
    capacity = faces[0].numel() if capacity is None else capacity
    out, big = poisoned(n, capacity)
    got = ops.picture_points_batch(faces, positions, capacity, out=out)
    assert len(got) == n and guards_untouched(big, capacity), what
    for f in range(n):
        pts, pix, count = want_points(faces[f], positions[f], capacity)
        assert got[f][0].data_ptr() == out[0][f].data_ptr()
        assert bits(got[f][2]).tolist() == count.tolist(), (what, f)
        assert np.array_equal(bits(got[f][1]), pix), (what, f)
        assert np.array_equal(bits(got[f][0]), bits(pts)), (what, f)
    return got


# ---- points: rendered pictures ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cam", list(CAMERAS))
def test_rendered_pictures(ops, body33, cam, size, n_views):
    face, pos = rendered(ops, body33, cam, size, n_views)
    n_pix = n_views * size[0] * size[1]
    assert face.numel() == n_pix and pos.numel() == 3 * n_pix
    k_all = int(ref.points(host(face), host(pos))[2][1])
    print("%s %dx%d x%d: %d of %d pixels covered" % (cam, size[0], size[1], n_views, k_all, n_pix))
    assert k_all >= 100 and n_pix - k_all >= 100
    first = check_points(ops, [face], [pos], what="capacity = L")
    again = check_points(ops, [face], [pos], what="second run")
    for a, b in zip(first[0], again[0]):
        assert np.array_equal(bits(a), bits(b))
    # the positions in the list are the picture's at the listed pixels, and every listed pixel is covered
    pixels = first[0][1][:k_all].long()
    assert torch.equal(pos.reshape(-1, 3)[pixels].view(torch.int32), first[0][0][:, :k_all].t().view(torch.int32))
    assert bool((face.reshape(-1)[pixels] >= 0).all()) and bool((pixels[1:] > pixels[:-1]).all())
    for capacity in (k_all - 1, k_all, k_all + 1, 1, 64):
        got = check_points(ops, [face], [pos], capacity, what="capacity %d" % capacity)
        assert bits(got[0][2]).tolist() == [min(k_all, capacity), k_all]
    # the per-frame wrapper: fresh buffers start as zeros
    pts, pix, count = ops.picture_points(face, pos)
    want = ref.points(host(face), host(pos))
    assert np.array_equal(bits(pts), bits(want[0])) and np.array_equal(bits(pix), want[1])
    assert bits(count).tolist() == want[2].tolist()


# ---- points: synthetic pictures --------------------------------------------------------------------------------------

def synthetic(n_pixels, covered, seed=0):
    """face ids (-1, or a face index that may be 0) and positions of random 32-bit patterns: NaNs with payloads,
    infinities and denormals among them."""
    rng = np.random.RandomState(seed)
    face = np.full(n_pixels, -1, np.int32)
    face[covered] = rng.randint(0, 3, size=face[covered].shape)
    pos = rng.randint(0, 2 ** 32, size=(n_pixels, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return torch.from_numpy(face).to(DEV), torch.from_numpy(pos).to(DEV)


PATTERNS = {
    "L=1 covered": (1, slice(None)), "L=1 uncovered": (1, slice(0, 0)),
    "L=1025 all": (1025, slice(None)), "L=1025 none": (1025, slice(0, 0)),
    "L=1025 last only": (1025, slice(1024, None)), "L=1024 first of each wave": (1024, slice(0, None, 64)),
    "L=257*129 every 3rd": (257 * 129, slice(0, None, 3)),
    "L=2^20+7 every 5th": (2 ** 20 + 7, slice(2, None, 5)),  # 1,025 block sums: the scan of them loops twice
    "L=2^20+7 all": (2 ** 20 + 7, slice(None)),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_synthetic_pictures(ops, pattern):
    n_pixels, covered = PATTERNS[pattern]
    face, pos = synthetic(n_pixels, covered, seed=len(pattern))
    k_all = int((face >= 0).sum())
    got = check_points(ops, [face], [pos], what=pattern)
    assert bits(got[0][2]).tolist() == [k_all, k_all]
    for capacity in sorted({max(k_all - 1, 1), k_all + 1, max(k_all // 2, 1), n_pixels + 5}):
        check_points(ops, [face], [pos], capacity, what="%s, capacity %d" % (pattern, capacity))


def test_negative_face_ids_other_than_minus_one_are_uncovered(ops):
    face = torch.tensor([-1, 0, -2, 5, -(2 ** 31), 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    pos = torch.arange(18, dtype=torch.float32, device=DEV).reshape(6, 3)
    got = check_points(ops, [face], [pos])
    assert bits(got[0][2]).tolist() == [3, 3] and bits(got[0][1])[:3].tolist() == [1, 3, 5]


@pytest.mark.parametrize("n", [1, 2, 32, 33])
def test_batches(ops, n):
    """Frames with differing K, one of them with K = 0 (not the only frame of the 1-frame batch's bigger sisters); 33
    frames go through two calls of the C-ABI."""
    assert ops.MAX_FRAMES == 32
    n_pixels = 3 * 1024 + 17
    frames = []
    for f in range(n):
        step = 0 if f == 1 else 2 + f % 7
        covered = slice(0, 0) if step == 0 else slice(f % 5, None, step)
        frames.append(synthetic(n_pixels, covered, seed=100 + f))
    faces, positions = [fr[0] for fr in frames], [fr[1] for fr in frames]
    got = check_points(ops, faces, positions, what="n = %d" % n)
    if n > 1:
        assert bits(got[1][2]).tolist() == [0, 0]
    assert n == 1 or len({tuple(bits(g[2]).tolist()) for g in got}) > 1
    capacity = 300  # truncates most frames, not the empty one
    got = check_points(ops, faces, positions, capacity, what="n = %d, capacity %d" % (n, capacity))
    # frame f of the batch == the per-frame call on frame f
    for f in (0, n - 1):
        out, _ = poisoned(1, capacity)
        one = ops.picture_points(faces[f], positions[f], capacity, out=tuple(o[0] for o in out))
        for a, b in zip(one, got[f]):
            assert np.array_equal(bits(a), bits(b)), f


# ---- paint -----------------------------------------------------------------------------------------------------------

def test_paint_against_the_restatement(ops, body33):
    face, pos = rendered(ops, body33, "rotated", (40, 24), 3)
    n_pix = face.numel()
    pts, pix, count = ops.picture_points(face, pos)
    k_all = int(count[1])
    values = torch.from_numpy(np.random.RandomState(9).standard_normal((3, n_pix)).astype(np.float32) * 2).to(DEV)
    for paint in (dict(scale=0.5, bias=0.5, lo=-INF, hi=INF), dict(scale=0.5, bias=0.5, lo=0.0, hi=1.0),
                  dict(scale=3.0, bias=0.1, lo=-INF, hi=INF)):
        image = torch.full((3, 40, 24, 3), FPOISON, device=DEV)
        got = ops.picture_paint(values, pix, count, out=image, **paint)
        assert got.data_ptr() == image.data_ptr()
        want = ref.paint(host(values), host(pix), host(count), np.full((3, 40, 24, 3), FPOISON, np.float32),
                         **paint)
        assert np.array_equal(bits(image), bits(want)), paint
        # pixels outside the list keep the sentinel, pixels in it lost it
        covered = (face >= 0).reshape(-1)
        flat = image.reshape(-1, 3)
        assert bool((flat[~covered] == FPOISON).all()) and int(covered.sum()) == k_all
        assert bool((flat[covered] != FPOISON).all())
    # without out=: a fresh image of the background
    fresh = ops.picture_paint(values, pix, count, n_pixels=n_pix, background=0.25)
    want = ref.paint(host(values), host(pix), host(count), np.full((n_pix, 3), 0.25, np.float32))
    assert np.array_equal(bits(fresh), bits(want))


def test_paint_into_the_position_buffer(ops, body33):
    """image aliased to position: what the slot does.  Uncovered pixels keep the render's background."""
    face, pos = rendered(ops, body33, "perspective", (33, 33), 1)
    image = pos.clone()
    pts, pix, count = ops.picture_points(face, image)
    values = (pts * 0.5).contiguous()
    ops.picture_paint(values, pix, count, out=image)
    want = ref.paint(host(values), host(pix), host(count), host(pos).copy())
    assert np.array_equal(bits(image), bits(want))
    uncovered = (face < 0).reshape(-1)
    assert bool((image.reshape(-1, 3)[uncovered] == 0.25).all())


def test_paint_skips_pixels_outside_and_clamps_the_count(ops):
    n_pix, capacity = 50, 8
    values = torch.arange(3 * capacity, dtype=torch.float32, device=DEV).reshape(3, capacity)
    pixels = torch.tensor([7, -1, n_pix, 2 ** 31 - 1, -(2 ** 31), n_pix - 1, 0, 3], dtype=torch.int32, device=DEV)
    for count in ([8, 8], [5, 5], [0, 0], [-4, 9], [2 ** 31 - 1, 0], [9, 9]):
        k = torch.tensor(count, dtype=torch.int32, device=DEV)
        guarded = torch.full((n_pix + 2, 3), FPOISON, device=DEV)  # a row in front of the image and one behind it
        image = guarded[1:-1]
        ops.picture_paint(values, pixels, k, out=image, scale=1.0, bias=0.0)
        want = ref.paint(host(values), host(pixels), count, np.full((n_pix, 3), FPOISON, np.float32), 1.0, 0.0)
        assert np.array_equal(bits(image), bits(want)), count
        assert bool((guarded[0] == FPOISON).all()) and bool((guarded[-1] == FPOISON).all()), count
        n = min(max(count[0], 0), capacity)
        assert int((image[:, 0] != FPOISON).sum()) == sum(1 for p in pixels[:n].tolist() if 0 <= p < n_pix)


@pytest.mark.parametrize("n", [2, 33])
def test_paint_batches(ops, n):
    n_pixels = 1500
    frames = [synthetic(n_pixels, slice(0, 0) if f == 1 else slice(f % 3, None, 2 + f % 4), seed=7 + f) for f in range(n)]
    found = ops.picture_points_batch([fr[0] for fr in frames], [fr[1] for fr in frames])
    rng = np.random.RandomState(4)
    values = [torch.from_numpy(rng.standard_normal((3, n_pixels)).astype(np.float32)).to(DEV) for _ in range(n)]
    images = torch.full((n, n_pixels, 3), FPOISON, device=DEV)
    ops.picture_paint_batch(values, [f[1] for f in found], [f[2] for f in found], out=images)
    for f in range(n):
        want = ref.paint(host(values[f]), host(found[f][1]), host(found[f][2]),
                         np.full((n_pixels, 3), FPOISON, np.float32))
        assert np.array_equal(bits(images[f]), bits(want)), f
    assert bool((images[1] == FPOISON).all())  # the frame without a covered pixel


# ---- refusals of the C-ABI --------------------------------------------------------------------------------------------

class Env:
    """Well-formed arguments of the four entry points on tiny buffers, to be spoilt one at a time."""
    ORDER = {
        "mp_picture_points": "face position n_pixels capacity points pixels count stream",
        "mp_picture_points_batch": "n face position n_pixels capacity points pixels count stream",
        "mp_picture_paint": "values pixels count capacity n_pixels scale bias lo hi image stream",
        "mp_picture_paint_batch": "n values pixels count capacity n_pixels scale bias lo hi image stream",
    }
    BUFFERS = {"points": ("face", "position", "points", "pixels", "count"),
               "paint": ("values", "pixels", "count", "image")}

    def __init__(self):
        from monoport_amd import ops
        self.ctx = ops.get_context(torch.device(DEV))
        self.lib = self.ctx.lib
        self.n, self.n_pixels, self.capacity = 2, 12, 12
        n, z = self.n, (lambda *s, **k: torch.zeros(*s, device=DEV, **k))
        self.face = torch.tensor([[0, -1, 2] * 4] * n, dtype=torch.int32, device=DEV)
        self.position = z(n, self.n_pixels, 3)
        self.odd = z(64)[1:].view(torch.uint8)[1:]  # an address that is not 4-byte aligned
        assert self.odd.data_ptr() % 4 == 1
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        self.reset()

    def reset(self):
        n = self.n
        self.points = torch.full((n, 3, self.capacity), FPOISON, device=DEV)
        self.pixels = torch.full((n, self.capacity), IPOISON, dtype=torch.int32, device=DEV)
        self.count = torch.full((n, 2), IPOISON, dtype=torch.int32, device=DEV)
        self.values = torch.ones((n, 3, self.capacity), device=DEV)
        # what paint reads: the first three pixels, in order
        self.list_pixels = torch.arange(self.capacity, dtype=torch.int32, device=DEV).repeat(n, 1)
        self.list_count = torch.full((n, 2), 3, dtype=torch.int32, device=DEV)
        self.image = torch.full((n, self.n_pixels, 3), FPOISON, device=DEV)

    def args(self, name):
        batch = name.endswith("_batch")
        one = (lambda t: ctypes.c_void_p(t[0].data_ptr()))
        many = (lambda t: (ctypes.c_void_p * self.n)(*[r.data_ptr() for r in t]))
        p = many if batch else one
        paint = "paint" in name
        a = dict(face=p(self.face), position=p(self.position), points=p(self.points),
                 pixels=p(self.list_pixels if paint else self.pixels),
                 count=p(self.list_count if paint else self.count), values=p(self.values), image=p(self.image), n_pixels=self.n_pixels,
                 capacity=self.capacity, scale=0.5, bias=0.5, lo=-INF, hi=INF, stream=self.stream, n=self.n)
        return a

    def call(self, name, **changed):
        a = self.args(name)
        a.update(changed)
        rc = getattr(self.lib, name)(self.ctx.handle, *[a[k] for k in self.ORDER[name].split()])
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.points == FPOISON).all()) and bool((self.pixels == IPOISON).all())
                and bool((self.count == IPOISON).all()) and bool((self.image == FPOISON).all()))


@pytest.fixture()
def env():
    return Env()


ENTRIES = list(Env.ORDER)
REFUSED = [("n_pixels", dict(n_pixels=0), ARG), ("n_pixels", dict(n_pixels=-5), ARG), ("capacity", dict(capacity=0), ARG),
           ("capacity", dict(capacity=-1), ARG), ("n_pixels", dict(n_pixels=2 ** 31 // 3 + 1), UNSUPPORTED),
           ("n_pixels", dict(n_pixels=2 ** 40), UNSUPPORTED)]


@pytest.mark.parametrize("name", ENTRIES)
def test_a_well_formed_call_is_accepted(env, name):
    rc, msg = env.call(name)
    assert rc == OK, msg
    torch.cuda.synchronize()
    frames = env.n if name.endswith("_batch") else 1
    if "points" in name:
        assert env.count[:frames].cpu().tolist() == [[8, 8]] * frames
        assert env.pixels[0, :8].cpu().tolist() == [0, 2, 3, 5, 6, 8, 9, 11]
        assert bool((env.pixels[frames:] == IPOISON).all()) and bool((env.image == FPOISON).all())
    else:
        assert bool((env.image[:frames, :3] == 1.0).all()) and bool((env.image[:frames, 3:] == FPOISON).all())
        assert bool((env.image[frames:] == FPOISON).all()) and bool((env.points == FPOISON).all())


@pytest.mark.parametrize("what,changed,code", REFUSED, ids=[r[0] + str(i) for i, r in enumerate(REFUSED)])
@pytest.mark.parametrize("name", ENTRIES)
def test_refusals(env, name, what, changed, code):
    rc, msg = env.call(name, **changed)
    assert rc == code, (what, msg)
    assert msg.startswith(name + ":"), msg
    assert env.untouched()


@pytest.mark.parametrize("name", ENTRIES)
def test_null_and_misaligned_buffers(env, name):
    for buffer in Env.BUFFERS["points" if "points" in name else "paint"]:
        tensor = getattr(env, ("list_" + buffer) if "paint" in name and buffer in ("pixels", "count") else buffer)
        for address, word in ((env.odd.data_ptr(), "misaligned"), (None, "null")):
            if name.endswith("_batch"):
                rows = [r.data_ptr() for r in tensor]
                arg = (ctypes.c_void_p * env.n)(*(rows[:-1] + [address]))
            else:
                arg = ctypes.c_void_p(address)
            rc, msg = env.call(name, **{buffer: arg})
            assert rc == ARG and msg.startswith(name + ":") and word in msg, (buffer, word, msg)
    assert env.untouched()


@pytest.mark.parametrize("name", [e for e in ENTRIES if e.endswith("_batch")])
def test_frames_per_call(env, name):
    for n in (0, -1, 33):
        many = (lambda t: (ctypes.c_void_p * max(n, 1))(*([t[0].data_ptr()] * max(n, 1))))  # noqa: E731
        rc, msg = env.call(name, n=n, **{b: many(getattr(env, b)) for b in Env.BUFFERS["points" if "points" in name
                                                                                       else "paint"]})
        assert rc == ARG and msg.startswith(name + ":"), (n, msg)
    rc, msg = env.call(name, **{Env.BUFFERS["points" if "points" in name else "paint"][0]: None})  # the array itself
    assert rc == ARG and msg.startswith(name + ":"), msg
    assert env.untouched()


# ---- a scratch arena that starts dirty -------------------------------------------------------------------------------

@pytest.mark.parametrize("byte", FILLS, ids=["0x%02X" % b for b in FILLS])
def test_dirty_arena(ops, body33, byte):
    """The block sums live in the stream's scratch arena: they are written before they are read, whatever it held."""
    face, pos = rendered(ops, body33, "rotated", (33, 33), 3)
    big_face, big_pos = synthetic(2 ** 20 + 7, slice(1, None, 3), seed=5)  # block sums beyond one scan pass
    dev = torch.device(DEV)
    torch.cuda.synchronize(dev)  # the inputs were made on the default stream
    stream = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(stream):
            block = ops.scratch_fill(dev, 1 << 20, byte)
            before = ops.memory_stats(dev)
            small = check_points(ops, [face, face], [pos, pos], what="fill 0x%02X" % byte)
            ops.scratch_fill(dev, 1 << 20, byte)
            check_points(ops, [face], [pos], 150, what="fill 0x%02X, truncated" % byte)
            ops.scratch_fill(dev, 1 << 20, byte)
            check_points(ops, [big_face], [big_pos], what="fill 0x%02X, 2^20 pixels" % byte)
            after = ops.memory_stats(dev)
        stream.synchronize()
    finally:
        ops.stream_release(stream)
    assert block >= 1 << 20
    assert (after["arena_bytes"], after["arenas"]) == (before["arena_bytes"], before["arenas"])
    for a, b in zip(small[0], small[1]):
        assert np.array_equal(bits(a), bits(b))
