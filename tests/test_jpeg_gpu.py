"""mp_picture_u8 / mp_picture_jpeg (csrc/jpeg.hip) and ops.picture_u8_raw / picture_jpeg_raw / jpeg_max_bytes on the GPU:
every file and every info row equals the numpy restatement (tests/jpeg_ref.py) BYTE FOR BYTE, on a fresh and on a dirty
scratch arena, in every run; a capacity one byte short reports the size and writes nothing; every refusal launches
nothing.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import jpeg_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, -1, -3  # MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED (include/monoport_hip.h)
F = np.float32
SHAPES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (40, 56), (61, 83), (160, 8)]
QUALITIES = [1, 50, 90, 100]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


def boundaries(count):
    """The exact k / 255 and (k + 0.5) / 255 of step 1 with their f32 neighbours, cycled to ``count`` values."""
    k = np.arange(256, dtype=np.float64)
    v = np.concatenate([k / 255.0, (k + 0.5) / 255.0]).astype(F)
    v = np.concatenate([v, np.nextafter(v, F(-1)), np.nextafter(v, F(2))])
    return np.resize(v, count).astype(F)


def pictures(h, w, n, seed):
    """n float pictures [h,w,3] of different content: noise beyond [0, 1] with NaN, +-inf and negative zero sprinkled
    in; the rounding boundaries of step 1; a smooth ramp (long zero runs at high quality); a hard checker."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    noise = rs.uniform(-0.25, 1.25, (h, w, 3)).astype(F)
    flat = noise.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 2.0, -3.0, 1.0, 0.0], F)
    idx = rs.choice(flat.size, size=min(flat.size, 8), replace=False)
    flat[idx] = special[:idx.size]
    smooth = np.stack([0.5 + 0.47 * np.sin(yy / 9.0 + xx / 13.0), 0.5 + 0.47 * np.cos(xx / 7.0),
                       0.5 + 0.4 * np.sin(yy / 5.0)], -1).astype(F)
    checker = np.repeat((((yy + xx) % 2) * 1.0)[..., None], 3, -1).astype(F)
    kinds = [noise, boundaries(h * w * 3).reshape(h, w, 3), smooth, checker]
    return np.stack([kinds[(seed + i) % 4] for i in range(n)])


def restarts(h, w, sub):
    _, mw, mh, _, _, _ = ref.geometry(h, w, sub)
    return [1, 3, None, min(mw * mh + 5, 65535)]


def device_files(ops, x, q, sub, restart, **kw):
    out, info = ops.picture_jpeg_raw(torch.from_numpy(x).to(DEV), q, sub, restart, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy()


def check(ops, x, q, sub, restart, **kw):
    out, info = device_files(ops, x, q, sub, restart, **kw)
    for i in range(x.shape[0]):
        want, _ = ref.encode(x[i], q, sub, restart)
        assert tuple(info[i]) == (len(want), 0), (x.shape, q, sub, restart, i, info[i], len(want))
        got = out[i, :len(want)].tobytes()
        if got != want:
            first = next(j for j in range(len(want)) if got[j] != want[j])
            raise AssertionError("picture %d of %s, q %d, %s, restart %r: byte %d of %d differs"
                                 % (i, x.shape, q, sub, restart, first, len(want)))
        assert len(want) <= ref.max_bytes(x.shape[1], x.shape[2], sub, restart)


@pytest.mark.parametrize("sub", ref.SUBSAMPLINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_files_equal_the_restatement(ops, shape, sub):
    """Every quality x restart of one shape and subsampling; n alternates between 1 and 3 and the contents rotate."""
    h, w = shape
    case = 0
    for q in QUALITIES:
        for restart in restarts(h, w, sub):
            n = 3 if case % 2 == 0 else 1
            check(ops, pictures(h, w, n, case), q, sub, restart)
            case += 1


def test_more_intervals_and_blocks_than_a_workgroup_scans_at_once(ops):
    """The scans of the interval and offset kernels carry over chunks of 256: 270 intervals of one MCU, and one interval
    of 270 MCUs (810 blocks)."""
    for restart in (1, 270):
        check(ops, pictures(24, 720, 2, 0), 50, "444", restart)
    check(ops, pictures(16, 4096, 1, 2), 90, "420", 1)  # the widest picture: 256 intervals, the last column of MCUs


def test_max_bytes_and_default_capacity(ops):
    for h, w in SHAPES + [(4096, 4096), (1024, 1024)]:
        for sub in ref.SUBSAMPLINGS:
            for restart in (None, 1, 7):
                assert ops.jpeg_max_bytes(h, w, sub, restart) == ref.max_bytes(h, w, sub, restart)
    lib = ops.get_context(DEV).lib
    assert lib.mp_jpeg_max_bytes(0, 8, 0, 0) == 0 and lib.mp_jpeg_max_bytes(8, 4097, 0, 0) == 0
    assert lib.mp_jpeg_max_bytes(8, 8, 2, 0) == 0 and lib.mp_jpeg_max_bytes(8, 8, 0, 65536) == 0


def test_picture_u8_equals_step_1(ops):
    for h, w in SHAPES:
        x = pictures(h, w, 4, 0)
        got = ops.picture_u8_raw(torch.from_numpy(x).to(DEV))
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref.to_u8(x))
    v = boundaries(3 * 4096).reshape(-1, 3)
    assert np.array_equal(ops.picture_u8_raw(torch.from_numpy(v).to(DEV)).cpu().numpy(), ref.to_u8(v))
    k = np.arange(256)
    assert np.array_equal(ref.to_u8((k / 255.0).astype(F)), k)  # the restatement itself: k / 255 gives k back
    # pointers off the vector path's alignment (16 bytes in, 4 bytes out), and a count that is no multiple of 4
    flat = torch.from_numpy(boundaries(3 * 1001 + 3)).to(DEV)
    buf = torch.full((3 * 1001 + 8,), SENTINEL, dtype=torch.uint8, device=DEV)
    for skip, off in ((3, 0), (0, 1), (3, 1), (0, 0)):
        buf.fill_(SENTINEL)
        x = flat[skip:skip + 3 * 1001].view(-1, 3)
        got = ops.picture_u8_raw(x, out=buf[off:off + 3 * 1001].view(-1, 3))
        assert np.array_equal(got.cpu().numpy(), ref.to_u8(x.cpu().numpy())), (skip, off)
        assert (buf[:off] == SENTINEL).all() and (buf[off + 3 * 1001:] == SENTINEL).all()


def test_three_runs_give_the_same_bytes(ops):
    x = torch.from_numpy(pictures(61, 83, 3, 0)).to(DEV)
    for sub in ref.SUBSAMPLINGS:
        runs = []
        for _ in range(3):
            out, info = ops.picture_jpeg_raw(x, 100, sub, 3)
            torch.cuda.synchronize()
            runs.append((out.cpu().numpy(), info.cpu().numpy()))
        sizes = runs[0][1][:, 0]
        for out, info in runs[1:]:
            assert np.array_equal(info, runs[0][1])
            for i, s in enumerate(sizes):
                assert np.array_equal(out[i, :s], runs[0][0][i, :s])


@pytest.mark.parametrize("sub", ref.SUBSAMPLINGS)
def test_capacity_exact_and_one_byte_short(ops, sub):
    """At picture 1's exact size the call succeeds for it; at one byte less info reports the same size with the overflow
    word set, nothing of that picture is written, and the guard behind ``out`` and the rest of ``out`` keep their fill."""
    x = pictures(40, 56, 3, 0)
    want = [ref.encode(x[i], 90, sub, 3)[0] for i in range(3)]
    sizes = [len(b) for b in want]
    guard = 8192
    for cap in (sizes[1], sizes[1] - 1):
        buf = torch.full((3 * cap + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
        out, info = device_files(ops, x, 90, sub, 3, out=buf[:3 * cap].view(3, cap))
        whole = buf.cpu().numpy()
        assert (whole[3 * cap:] == SENTINEL).all()
        for i in range(3):
            fits = sizes[i] <= cap
            assert tuple(info[i]) == (sizes[i], 0 if fits else 1), (cap, i, info[i])
            if fits:
                assert out[i, :sizes[i]].tobytes() == want[i] and (out[i, sizes[i]:] == SENTINEL).all()
            else:
                assert (out[i] == SENTINEL).all()
    # the smallest capacity the call takes: every picture overflows, nothing is written
    cap = ref.HEADER_BYTES
    buf = torch.full((3 * cap + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
    out, info = device_files(ops, x, 90, sub, 3, out=buf[:3 * cap].view(3, cap))
    assert (buf.cpu().numpy() == SENTINEL).all() and [tuple(r) for r in info] == [(s, 1) for s in sizes]


def test_a_file_larger_than_its_raw_bytes(ops):
    x = np.random.RandomState(5).uniform(0, 1, (1, 64, 64, 3)).astype(F)
    out, info = device_files(ops, x, 100, "444", None)
    assert info[0, 0] > 64 * 64 * 3 and info[0, 1] == 0
    assert out[0, :info[0, 0]].tobytes() == ref.encode(x[0], 100, "444", None)[0]


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_dirty_arena(ops, byte):
    for (h, w), sub, q, restart in (((61, 83), "420", 100, None), ((17, 23), "444", 50, 1), ((160, 8), "444", 90, None)):
        ops.scratch_fill(DEV, 4 << 20, byte)
        check(ops, pictures(h, w, 3, 1), q, sub, restart)


class Env:
    """A well-formed call of mp_picture_jpeg on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        self.x = torch.from_numpy(pictures(17, 23, 2, 2)).to(DEV)
        self.cap = 4096
        self.out = torch.full((2, self.cap), SENTINEL, dtype=torch.uint8, device=DEV)
        self.info = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
        self.u8 = torch.full((2 * 17 * 23, 3), SENTINEL, dtype=torch.uint8, device=DEV)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def done(self, rc):
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()

    def jpeg(self, **k):
        a = dict(images=self.x.data_ptr(), n=2, h=17, w=23, q=90, sub=1, restart=0, out=self.out.data_ptr(),
                 cap=self.cap, info=self.info.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_jpeg(self.ctx.handle, a["images"], a["n"], a["h"], a["w"], a["q"], a["sub"],
                                                  a["restart"], a["out"], a["cap"], a["info"], self.stream))

    def to_u8(self, **k):
        a = dict(image=self.x.data_ptr(), n=2 * 17 * 23, out=self.u8.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_u8(self.ctx.handle, a["image"], a["n"], a["out"], self.stream))


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    x_bytes = env.x.numel() * 4
    refused = [
        (dict(h=0), UNSUPPORTED, "sides"), (dict(h=4097), UNSUPPORTED, "sides"),
        (dict(w=0), UNSUPPORTED, "sides"), (dict(w=4097), UNSUPPORTED, "sides"),
        (dict(q=0), ARG, "quality"), (dict(q=101), ARG, "quality"),
        (dict(sub=2), UNSUPPORTED, "subsampling"), (dict(sub=-1), UNSUPPORTED, "subsampling"),
        (dict(restart=-1), ARG, "restart"), (dict(restart=65536), ARG, "restart"),
        (dict(n=0), ARG, "pictures"), (dict(n=-3), ARG, "pictures"), (dict(n=65536), UNSUPPORTED, "pictures"),
        (dict(cap=ref.HEADER_BYTES - 1), ARG, "capacity"), (dict(cap=0), ARG, "capacity"),
        (dict(images=None), ARG, "null"), (dict(out=None), ARG, "null"), (dict(info=None), ARG, "null"),
        (dict(images=env.x.data_ptr() + 2), ARG, "misaligned"), (dict(info=env.info.data_ptr() + 1), ARG, "misaligned"),
        (dict(out=env.x.data_ptr()), ARG, "aliases"), (dict(out=env.x.data_ptr() + x_bytes - 1), ARG, "aliases"),
        (dict(info=env.x.data_ptr() + 8), ARG, "aliases"), (dict(info=env.out.data_ptr() + 4), ARG, "aliases"),
    ]
    for changed, code, word in refused:
        rc, msg = env.jpeg(**changed)
        assert rc == code and msg.startswith("mp_picture_jpeg:") and word in msg, (changed, rc, msg)
    for changed, word in ((dict(n=-1), "n_pixels"), (dict(image=None), "null"), (dict(out=None), "null"),
                          (dict(image=env.x.data_ptr() + 1), "misaligned"), (dict(out=env.x.data_ptr() + 5), "aliases")):
        rc, msg = env.to_u8(**changed)
        assert rc == ARG and msg.startswith("mp_picture_u8:") and word in msg, (changed, rc, msg)
    rc, msg = env.to_u8(n=0x7fffffff // 3 + 1)
    assert rc == UNSUPPORTED and "2^31 / 3" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (env.out == SENTINEL).all() and (env.info == -7).all() and (env.u8 == SENTINEL).all()  # nothing was launched
    assert env.to_u8(n=0)[0] == OK
    # the context is still usable
    assert env.jpeg()[0] == OK and env.to_u8()[0] == OK
    torch.cuda.synchronize()
    x = env.x.cpu().numpy()
    info, out = env.info.cpu().numpy(), env.out.cpu().numpy()
    for i in range(2):
        want = ref.encode(x[i], 90, "420", None)[0]
        assert tuple(info[i]) == (len(want), 0) and out[i, :len(want)].tobytes() == want
    assert np.array_equal(env.u8.cpu().numpy(), ref.to_u8(x).reshape(-1, 3))


def test_wrapper_refusals(ops):
    x = torch.zeros((2, 8, 8, 3), device=DEV)
    for bad in (dict(quality=0), dict(quality=101), dict(quality=90.0), dict(subsampling="422"), dict(restart=0),
                dict(restart=65536), dict(capacity=100), dict(out=torch.zeros((3, 4096), dtype=torch.uint8, device=DEV)),
                dict(info=torch.zeros((2, 2), dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError, match="picture_jpeg_raw"):
            ops.picture_jpeg_raw(x, **bad)
    for bad in (x[:, :, :, :2], x.double(), x[0], x[:, ::2]):
        with pytest.raises(ValueError, match="picture_jpeg_raw"):
            ops.picture_jpeg_raw(bad)
    with pytest.raises(ValueError, match="picture_u8_raw"):
        ops.picture_u8_raw(x.double())
