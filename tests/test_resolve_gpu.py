"""mp_picture_resolve(_batch) (csrc/resolve.hip) and ops.picture_resolve_batch on the GPU against the numpy restatement
of the definition (tests/resolve_ref.py): every comparison is on the bits.  Needs an MI355X."""
import ctypes
import itertools

import numpy as np
import pytest

import resolve_ref as rr
from test_mesh_render_gpu import ARG, DEV, OK, host

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
# 1 x 1; odd sizes, no multiple of the 256-thread block; more than one block; a full block grid; the widest row there is
SIZES = [(1, 1), (3, 5), (17, 33), (64, 64), (1, None)]
NAMES = ("image", "depth", "face", "mask", "coverage")


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


def pictures(seed, shape, uncovered=False):
    """Random fine pictures [..., s h, s w]: finite images over many binades with zeros of both signs and denormals,
    faces with -1 holes, depths from a few values (exact ties, +0 and -0 among them), masks 0 / 1 / 2."""
    rng = np.random.default_rng(seed)
    image = (rng.standard_normal(shape + (3,)) * np.exp2(rng.integers(-30, 30, shape + (3,)))).astype(F)
    special = np.array([0.0, -0.0, 1e-42, -3e-45, 2.0 ** -126, 1.0, 0.25, -1e30], F)
    pick = rng.random(shape + (3,)) < 0.15
    image[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    values = np.array([-1.5, -0.0, 0.0, 0.25, 0.25, 1.0, 1.0, 3.0, -2.0 ** -130], F)
    depth = values[rng.integers(0, len(values), shape)]
    face = rng.integers(0, 40, shape).astype(np.int32)
    face[rng.random(shape) < 0.35] = -1
    mask = rng.integers(0, 3, shape).astype(np.uint8)
    if uncovered:
        face[:], mask[:] = -1, 0
    return image, depth, face, mask


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def shifted(a):
    """The same values at an address that is 4-byte but not 8-byte aligned (1-byte for a mask): the narrow loads."""
    if a is None:
        return None
    flat = np.ascontiguousarray(a).reshape(-1)
    pad = 1 if a.dtype != np.uint8 else 3
    buf = torch.zeros(flat.size + 4, dtype=dev(flat).dtype, device=DEV)
    buf[pad:pad + flat.size] = dev(flat)
    out = buf[pad:pad + flat.size].view(a.shape)
    assert out.data_ptr() % 8 != 0
    return out


def check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert rr.same_bits(host(g), w), (what, name)


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("h,w", SIZES)
def test_kernel_against_the_restatement(ops, h, w, s):
    w = 4096 // s if w is None else w
    image, depth, face, mask = pictures(100 * s + h + w, (s * h, s * w))
    wants = {}
    for nearest, with_mask in itertools.product(("max", "min"), (True, False)):
        m = mask if with_mask else None
        want = wants[nearest, with_mask] = rr.resolve(image, depth, face, m, s, nearest)
        assert want[4].min() < want[4].max() or h * w == 1
        for place in (dev, shifted):  # wide loads (s = 2, 4) and dword loads
            got = ops.picture_resolve_batch([place(image)], [place(depth)], [place(face)],
                                            None if m is None else [place(m)], s, nearest)[0]
            check(got, want, (nearest, with_mask, place.__name__))
            assert tuple(got[0].shape) == (h, w, 3) and tuple(got[4].shape) == (h, w)
    # every optional output present and absent, each from no more inputs than it needs; the rest is left alone
    d_image, d_depth, d_face, d_mask = dev(image), dev(depth), dev(face), dev(mask)
    want = wants["max", True]
    for present in itertools.product((False, True), repeat=5):
        if not any(present):
            continue
        outs = [torch.full(tuple(np.shape(wv)), 77, dtype=dev(wv).dtype, device=DEV) if p else None
                for p, wv in zip(present, want)]
        got = ops.picture_resolve_batch([d_image] if present[0] else None,
                                        [d_depth] if present[1] or present[2] else None,
                                        [d_face] if present[1] or present[2] else None,
                                        [d_mask], s, "max", out=tuple(None if o is None else [o] for o in outs))[0]
        for name, p, g, o, wv in zip(NAMES, present, got, outs, want):
            assert (g is None) == (not p) and (not p or (g.data_ptr() == o.data_ptr() and rr.same_bits(host(o), wv))), name
    # without a mask the coverage needs the face ids alone, and the image nothing else
    got = ops.picture_resolve_batch(None, None, [d_face], None, s)[0]
    assert [g is None for g in got] == [True, True, True, True, False] and rr.same_bits(host(got[4]), wants["max", False][4])
    got = ops.picture_resolve_batch([d_image], None, None, None, s)[0]
    assert [g is None for g in got] == [False, True, True, True, True] and rr.same_bits(host(got[0]), want[0])


@pytest.mark.parametrize("s", [2, 3, 4])
def test_batched_equals_per_frame_and_repeats(ops, s):
    n, nv, h, w = 3, 2, 5, 9
    frames = [pictures(7 * s + f, (nv, s * h, s * w), uncovered=(f == 1)) for f in range(n)]
    cols = [[dev(fr[k]) for fr in frames] for k in range(4)]
    for nearest in ("max", "min"):
        batch = ops.picture_resolve_batch(*cols, s, nearest)
        again = ops.picture_resolve_batch(*cols, s, nearest)
        for f in range(n):
            want = rr.resolve(*frames[f], s, nearest)
            check(batch[f], want, ("batch", f))
            one = ops.picture_resolve_batch(*[[c[f]] for c in cols], s, nearest)[0]
            for a, b, c in zip(batch[f], one, again[f]):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                assert torch.equal(a.view(torch.uint8), c.view(torch.uint8))
            # a view of the frame alone: the views lie back to back
            v1 = ops.picture_resolve_batch(*[[c[f][1]] for c in cols], s, nearest)[0]
            check(v1, [wv[1] for wv in want], ("view", f))
    cov = host(batch[1][4])
    assert not cov.any() and (host(batch[1][2]) == -1).all() and not host(batch[1][1]).view(np.uint32).any()
    # the single-picture entry point gives the batched one's bits
    ctx = ops.get_context(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    outs = [torch.empty_like(t[0]) for t in batch[0]]
    rc = ctx.lib.mp_picture_resolve(ctx.handle, *[c[0][0].data_ptr() for c in cols], h, w, s, 1,
                                    *[o.data_ptr() for o in outs], stream)
    assert rc == OK
    for o, b in zip(outs, batch[0]):
        assert torch.equal(o.view(torch.uint8), b[0].view(torch.uint8))


def test_more_pictures_than_a_call_takes(ops):
    """Frames x views beyond mp_max_frames(): chunks of frames, and of the views of a frame."""
    s = 2
    for n, nv, h, w in ((5, 7, 2, 3), (1, ops.MAX_FRAMES + 1, 1, 2)):
        frames = [pictures(31 * n + f, (nv, s * h, s * w)) for f in range(n)]
        got = ops.picture_resolve_batch(*[[dev(fr[k]) for fr in frames] for k in range(4)], s, "min")
        for f in range(n):
            check(got[f], rr.resolve(*frames[f], s, "min"), (n, nv, f))


def test_ops_refuses_before_anything_is_enqueued(ops):
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)  # noqa: E731
    face = z(4, 6, dtype=torch.int32)
    for samples in (1, 5, 2.0, True):
        with pytest.raises(ValueError, match="samples must be"):
            ops.picture_resolve_batch(None, None, [face], None, samples)
    with pytest.raises(ValueError, match="at least one frame"):
        ops.picture_resolve_batch(None, None, None, None, 2)
    with pytest.raises(ValueError, match="s = 4"):
        ops.picture_resolve_batch(None, None, [face], None, 4)
    with pytest.raises(ValueError, match="nearest"):
        ops.picture_resolve_batch(None, None, [face], None, 2, "closest")
    with pytest.raises(ValueError, match="faces must be"):
        ops.picture_resolve_batch(None, [z(4, 8)], [face], None, 2)
    with pytest.raises(ValueError, match="masks must be"):
        ops.picture_resolve_batch(None, None, [face], [z(4, 6)], 2)
    with pytest.raises(ValueError, match="needs its input"):
        ops.picture_resolve_batch(None, None, [face], None, 2, out=(None, [z(2, 3)], None, None, None))
    with pytest.raises(ValueError, match="names no output"):
        ops.picture_resolve_batch(None, None, [face], None, 2, out=(None,) * 5)


class Env:
    """A well-formed mp_picture_resolve on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        z = lambda *shape, **k: torch.zeros(*shape, device=DEV, **k)  # noqa: E731
        self.h, self.w, self.s = 3, 4, 2
        fine, small = (2 * 3, 2 * 4), (3, 4)
        self.ins = dict(image=z(fine + (3,)), depth=z(fine), face=z(fine, dtype=torch.int32),
                        mask=z(fine, dtype=torch.uint8))
        self.outs = dict(image_out=z(small + (3,)), depth_out=z(small), face_out=z(small, dtype=torch.int32),
                         mask_out=z(small, dtype=torch.uint8), coverage=z(small))
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def fill(self, value):
        for t in self.outs.values():
            t.fill_(value)

    def untouched(self, value):
        torch.cuda.synchronize()
        return all(bool((t == value).all()) for t in self.outs.values())

    def call(self, **k):
        a = {name: t.data_ptr() for name, t in {**self.ins, **self.outs}.items()}
        a.update(h=self.h, w=self.w, samples=self.s, nearest=0)
        a.update(k)
        rc = self.lib.mp_picture_resolve(self.ctx.handle, a["image"], a["depth"], a["face"], a["mask"], a["h"], a["w"],
                                         a["samples"], a["nearest"], a["image_out"], a["depth_out"], a["face_out"],
                                         a["mask_out"], a["coverage"], self.stream)
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    env.fill(9)
    assert env.call()[0] == OK
    torch.cuda.synchronize()
    # a mask of zeros: nothing shows, whatever the face ids say
    assert (env.outs["coverage"] == 0).all() and (env.outs["face_out"] == -1).all() and (env.outs["image_out"] == 0).all()
    assert (env.outs["mask_out"] == 0).all() and (env.outs["depth_out"] == 0).all()
    # every output alone, each from the inputs it needs and no others
    none = dict(image_out=None, depth_out=None, face_out=None, mask_out=None, coverage=None)
    keep = lambda *names: {k: v for k, v in none.items() if k not in names}  # noqa: E731
    assert env.call(**keep("image_out"), depth=None, face=None, mask=None)[0] == OK
    assert env.call(**keep("depth_out"), image=None, mask=None)[0] == OK
    assert env.call(**keep("face_out"), image=None)[0] == OK
    assert env.call(**keep("mask_out"), image=None, depth=None, face=None)[0] == OK
    assert env.call(**keep("coverage"), image=None, depth=None, mask=None)[0] == OK
    assert env.call(**keep("coverage"), image=None, depth=None, face=None)[0] == OK
    assert env.call(nearest=1)[0] == OK and env.call(samples=3, h=2, w=2)[0] == OK and env.call(samples=4, h=1, w=2)[0] == OK
    refused = [
        (dict(samples=1), "samples"),
        (dict(samples=5), "samples"),
        (dict(samples=0), "samples"),
        (dict(samples=2, h=2049), "4096"),
        (dict(samples=3, w=1366), "4096"),
        (dict(samples=4, h=1025), "4096"),
        (dict(h=0), "4096"),
        (dict(w=-1), "4096"),
        (dict(nearest=2), "nearest"),
        (dict(nearest=-1), "nearest"),
        (none, "no output"),
        (dict(image=None), "image_out needs image"),
        (dict(depth=None), "need depth and face_id"),
        (dict(face=None), "need depth and face_id"),
        (dict(keep("face_out"), depth=None), "need depth and face_id"),
        (dict(mask=None), "mask_out needs mask"),
        (dict(keep("coverage"), mask=None, face=None), "coverage needs"),
        (dict(image=env.ins["image"].data_ptr() + 2), "misaligned"),
        (dict(face=env.ins["face"].data_ptr() + 1), "misaligned"),
        (dict(coverage=env.outs["coverage"].data_ptr() + 2), "misaligned"),
        (dict(image_out=env.ins["image"].data_ptr()), "aliases"),
        (dict(coverage=env.ins["depth"].data_ptr() + 8), "aliases"),
        (dict(mask_out=env.ins["mask"].data_ptr() + 5), "aliases"),
        (dict(depth_out=env.ins["face"].data_ptr()), "aliases"),
    ]
    env.fill(5)
    for changed, word in refused:
        rc, msg = env.call(**changed)
        assert rc == ARG and msg.startswith("mp_picture_resolve:") and word in msg, (changed, msg)
    assert env.untouched(5)  # a refused call launches nothing
    # a mask at any address is taken
    odd = torch.zeros(6 * 8 + 1, dtype=torch.uint8, device=DEV)[1:]
    assert env.call(mask=odd.data_ptr())[0] == OK
    # the batched form carries its own name and refuses frames x views out of range and a frame without its buffer
    arr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())  # noqa: E731
    ins = [arr(env.ins[k]) for k in ("image", "depth", "face", "mask")]
    outs = [arr(env.outs[k]) for k in ("image_out", "depth_out", "face_out", "mask_out", "coverage")]
    env.fill(5)
    for frames, views in ((0, 1), (1, 0), (33, 1), (1, 33), (4, 9), (-1, -1)):
        rc = env.lib.mp_picture_resolve_batch(env.ctx.handle, frames, views, *ins, 3, 4, 2, 0, *outs, env.stream)
        msg = env.lib.mp_last_error(env.ctx.handle).decode()
        assert rc == ARG and msg.startswith("mp_picture_resolve_batch:") and "pictures" in msg, msg
    hole = (ctypes.c_void_p * 1)(None)
    rc = env.lib.mp_picture_resolve_batch(env.ctx.handle, 1, 1, *ins[:3], hole, 3, 4, 2, 0, *outs, env.stream)
    assert rc == ARG and "null buffer for frame 0" in env.lib.mp_last_error(env.ctx.handle).decode()
    rc = env.lib.mp_picture_resolve_batch(env.ctx.handle, 1, 1, *ins, 3, 4, 2, 0, hole, *outs[1:], env.stream)
    assert rc == ARG and "null buffer for frame 0" in env.lib.mp_last_error(env.ctx.handle).decode()
    assert env.untouched(5)
    assert env.lib.mp_picture_resolve_batch(env.ctx.handle, 1, 1, *ins, 3, 4, 2, 0, *outs, env.stream) == OK
    torch.cuda.synchronize()
