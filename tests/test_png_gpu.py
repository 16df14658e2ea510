"""mp_picture_u16 / mp_picture_rgba8 / mp_picture_png (csrc/png.hip) and their ops wrappers on the GPU: every file and
every info row equals the numpy restatement (tests/png_ref.py) BYTE FOR BYTE on the cases of tests/png_cases.py, on a
fresh and on a dirty scratch arena, in every run, batched as alone; a capacity one byte short reports the size and writes
nothing; every refusal launches nothing.  Needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest

import png_cases as cases
import png_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, -1, -3  # MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED (include/monoport_hip.h)
F = np.float32
SENTINEL = 0xA5
FORMATS = sorted(ref.FORMATS)


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def small_cases(fmt):
    return tuple(cases.small_cases(fmt))


@functools.lru_cache(maxsize=None)
def restated(fmt, index, filt):
    """The restatement's file of a case, made once for all tests."""
    return cases.restated(small_cases(fmt)[index], filt)


def device_files(ops, c, filt, images=None, alpha=None, **kw):
    """mp_picture_png of one case (or of the given stacks of its kind) -> (out, info) on the host."""
    images = torch.from_numpy(c.image[None]).to(DEV) if images is None else images
    if alpha is None and c.alpha is not None:
        alpha = torch.from_numpy(c.alpha[None]).to(DEV)
    out, info = ops.picture_png_raw(images, alpha, c.format, filt, c.lo, c.scale, c.unmatte, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy()


def same(got, want, what):
    if got != want:
        first = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
        raise AssertionError("%s: byte %d of %d (got %d) differs" % (what, first, len(want), len(got)))


def check(ops, fmt, index, filt):
    c = small_cases(fmt)[index]
    want = restated(fmt, index, filt)
    out, info = device_files(ops, c, filt)
    assert tuple(info[0]) == (len(want), 0), (c.name, fmt, filt, info[0], len(want))
    same(out[0, :len(want)].tobytes(), want, "%s %s %s" % (c.name, fmt, filt))
    assert len(want) <= ops.png_max_bytes(c.image.shape[0], c.image.shape[1], fmt)


@pytest.mark.parametrize("filt", ref.FILTERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_files_equal_the_restatement(ops, fmt, filt):
    for index in range(len(small_cases(fmt))):
        check(ops, fmt, index, filt)


def test_more_blocks_than_a_workgroup_scans_at_once(ops):
    """png_sizes carries its scans over chunks of 256 blocks: 300 x 1200 RGBA is 352 blocks, 1.4 MB of noise-free
    content."""
    c = cases.smooth("rgba8", 300, 1200)
    out, info = device_files(ops, c, "paeth")
    want = cases.restated(c, "paeth")
    assert tuple(info[0]) == (len(want), 0)
    same(out[0, :len(want)].tobytes(), want, "352 blocks")


def test_samples_equal_their_restatement(ops):
    for c in small_cases("gray16"):
        got = ops.picture_u16_raw(torch.from_numpy(c.image).to(DEV), c.lo, c.scale)
        assert got.dtype == torch.uint16 and np.array_equal(got.cpu().numpy(), ref.to_u16(c.image, c.lo, c.scale)), c.name
    for c in small_cases("rgba8"):
        image, alpha = torch.from_numpy(c.image).to(DEV), torch.from_numpy(c.alpha).to(DEV)
        for unmatte in (None, 0.0, 0.75, 1.0):
            got = ops.picture_rgba8_raw(image, alpha, unmatte)
            assert got.dtype == torch.uint8 and tuple(got.shape) == c.alpha.shape + (4,)
            assert np.array_equal(got.cpu().numpy(), ref.to_rgba8(c.image, c.alpha, unmatte)), (c.name, unmatte)
    # every sixteenth of the 16-bit range's rounding boundaries and their f32 neighbours
    k = np.arange(0, 65536, 16, dtype=np.float64)
    v = np.concatenate([k / 65535.0, (k + 0.5) / 65535.0]).astype(F)
    v = np.concatenate([v, np.nextafter(v, F(-1)), np.nextafter(v, F(2))])
    assert np.array_equal(ops.picture_u16_raw(torch.from_numpy(v).to(DEV)).cpu().numpy(), ref.to_u16(v, 0.0, 1.0))


@pytest.mark.parametrize("fmt", FORMATS)
def test_batched_equals_per_picture_and_runs_repeat(ops, fmt):
    """Three pictures of one size in one call give the files of three calls, and a second run the same bytes."""
    base = [cases.noise(fmt, 40, 56, 1), cases.smooth(fmt, 40, 56), cases.constant(fmt, 40, 56)]
    images = torch.from_numpy(np.stack([c.image for c in base])).to(DEV)
    alpha = torch.from_numpy(np.stack([c.alpha for c in base])).to(DEV) if fmt == "rgba8" else None
    runs = [device_files(ops, base[0], "adaptive", images, alpha) for _ in range(2)]
    assert np.array_equal(runs[0][1], runs[1][1])
    for i, c in enumerate(base):
        want = cases.restated(c, "adaptive")
        assert tuple(runs[0][1][i]) == (len(want), 0)
        for out, _ in runs:
            same(out[i, :len(want)].tobytes(), want, "batched %s %d" % (fmt, i))
        alone, info = device_files(ops, c, "adaptive")
        assert tuple(info[0]) == (len(want), 0) and alone[0, :len(want)].tobytes() == want


@pytest.mark.parametrize("fmt", FORMATS)
def test_capacity_exact_and_one_byte_short(ops, fmt):
    """At picture 1's exact size the call succeeds for it; at one byte less info reports the same size with the overflow
    word set, nothing of that picture is written, and the guard behind ``out`` and the rest of ``out`` keep their fill."""
    base = [cases.noise(fmt, 40, 56, 1), cases.smooth(fmt, 40, 56), cases.constant(fmt, 40, 56)]
    images = torch.from_numpy(np.stack([c.image for c in base])).to(DEV)
    alpha = torch.from_numpy(np.stack([c.alpha for c in base])).to(DEV) if fmt == "rgba8" else None
    want = [cases.restated(c, "adaptive") for c in base]
    sizes = [len(b) for b in want]
    assert sizes[2] < sizes[1] < sizes[0]
    guard = 8192
    for cap in (sizes[1], sizes[1] - 1, ref.MIN_BYTES):
        buf = torch.full((3 * cap + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
        out, info = device_files(ops, base[0], "adaptive", images, alpha, out=buf[:3 * cap].view(3, cap))
        whole = buf.cpu().numpy()
        assert (whole[3 * cap:] == SENTINEL).all()
        for i in range(3):
            fits = sizes[i] <= cap
            assert tuple(info[i]) == (sizes[i], 0 if fits else 1), (cap, i, info[i])
            if fits:
                assert out[i, :sizes[i]].tobytes() == want[i] and (out[i, sizes[i]:] == SENTINEL).all()
            else:
                assert (out[i] == SENTINEL).all()


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x7F, 0x5A])
def test_dirty_arena(ops, byte):
    for fmt, name, filt in (("rgb8", "smooth_61x83", "adaptive"), ("rgba8", "noise_64x64", "sub"),
                            ("gray16", "constant_20x300", "up"), ("rgb8", "fibonacci", "none")):
        index = [c.name for c in small_cases(fmt)].index(name)
        ops.scratch_fill(DEV, 4 << 20, byte)
        check(ops, fmt, index, filt)


def test_input_views_off_by_four_pixels(ops):
    """The planes start four pixels into their buffers: 48 and 16 bytes, no multiple of a larger alignment."""
    for fmt in FORMATS:
        c = cases.smooth(fmt, 33, 45)
        per = 1 if fmt == "gray16" else 3
        flat = torch.zeros(4 * per + c.image.size, device=DEV)
        flat[4 * per:] = torch.from_numpy(c.image.reshape(-1)).to(DEV)
        images = flat[4 * per:].view((1,) + c.image.shape)
        alpha = None
        if fmt == "rgba8":
            aflat = torch.zeros(4 + c.alpha.size, device=DEV)
            aflat[4:] = torch.from_numpy(c.alpha.reshape(-1)).to(DEV)
            alpha = aflat[4:].view((1,) + c.alpha.shape)
        out, info = device_files(ops, c, "adaptive", images, alpha)
        want = cases.restated(c, "adaptive")
        assert tuple(info[0]) == (len(want), 0) and out[0, :len(want)].tobytes() == want, fmt


def test_max_bytes(ops):
    for h, w in ((1, 1), (61, 83), (1024, 1024), (4096, 4096)):
        for fmt in FORMATS:
            assert ops.png_max_bytes(h, w, fmt) == ref.max_bytes(h, w, fmt)
    lib = ops.get_context(DEV).lib
    assert lib.mp_png_max_bytes(0, 8, 0) == 0 and lib.mp_png_max_bytes(8, 4097, 0) == 0
    assert lib.mp_png_max_bytes(8, 8, 3) == 0 and lib.mp_png_max_bytes(8, 8, -1) == 0


class Env:
    """A well-formed call of mp_picture_png on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        self.c = cases.smooth("rgba8", 17, 23)
        self.x = torch.from_numpy(np.stack([self.c.image] * 2)).to(DEV)
        self.a = torch.from_numpy(np.stack([self.c.alpha] * 2)).to(DEV)
        self.cap = 4096
        self.out = torch.full((2, self.cap), SENTINEL, dtype=torch.uint8, device=DEV)
        self.info = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
        self.u16 = torch.from_numpy(np.full(2 * 17 * 23, 0xA5A5, np.uint16)).to(DEV)
        self.rgba = torch.full((2 * 17 * 23, 4), SENTINEL, dtype=torch.uint8, device=DEV)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def done(self, rc):
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()

    def png(self, **k):
        a = dict(images=self.x.data_ptr(), alpha=None, n=2, h=17, w=23, format=0, filter=5, lo=0.0, scale=1.0, unmatte=0,
                 bg=0.0, out=self.out.data_ptr(), cap=self.cap, info=self.info.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_png(self.ctx.handle, a["images"], a["alpha"], a["n"], a["h"], a["w"],
                                                 a["format"], a["filter"], a["lo"], a["scale"], a["unmatte"], a["bg"],
                                                 a["out"], a["cap"], a["info"], self.stream))

    def to_u16(self, **k):
        a = dict(depth=self.a.data_ptr(), n=2 * 17 * 23, lo=0.0, scale=1.0, out=self.u16.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_u16(self.ctx.handle, a["depth"], a["n"], a["lo"], a["scale"], a["out"],
                                                 self.stream))

    def to_rgba(self, **k):
        a = dict(image=self.x.data_ptr(), alpha=self.a.data_ptr(), n=2 * 17 * 23, unmatte=0, bg=0.0,
                 out=self.rgba.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_rgba8(self.ctx.handle, a["image"], a["alpha"], a["n"], a["unmatte"], a["bg"],
                                                   a["out"], self.stream))


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    x_bytes = env.x.numel() * 4
    rgba = dict(format=1, alpha=env.a.data_ptr())
    nan, inf = float("nan"), float("inf")
    refused = [
        (dict(h=0), UNSUPPORTED, "sides"), (dict(h=4097), UNSUPPORTED, "sides"),
        (dict(w=0), UNSUPPORTED, "sides"), (dict(w=4097), UNSUPPORTED, "sides"),
        (dict(format=3), UNSUPPORTED, "format"), (dict(format=-1), UNSUPPORTED, "format"),
        (dict(filter=6), UNSUPPORTED, "filter"), (dict(filter=-1), UNSUPPORTED, "filter"),
        (dict(n=0), ARG, "pictures"), (dict(n=-3), ARG, "pictures"), (dict(n=65536), UNSUPPORTED, "pictures"),
        (dict(cap=ref.MIN_BYTES - 1), ARG, "capacity"), (dict(cap=0), ARG, "capacity"),
        (dict(cap=2 ** 31 + 1), ARG, "capacity"),
        (dict(alpha=env.a.data_ptr()), ARG, "alpha for a format without it"),
        (dict(format=2, alpha=env.a.data_ptr()), ARG, "alpha for a format without it"),
        (dict(format=1), ARG, "without alpha"), (dict(unmatte=1), ARG, "unmatte without alpha"),
        (dict(lo=nan), ARG, "non-finite"), (dict(scale=inf), ARG, "non-finite"), (dict(bg=-inf), ARG, "non-finite"),
        (dict(images=None), ARG, "null"), (dict(out=None), ARG, "null"), (dict(info=None), ARG, "null"),
        (dict(images=env.x.data_ptr() + 2), ARG, "misaligned"), (dict(info=env.info.data_ptr() + 1), ARG, "misaligned"),
        (dict(format=1, alpha=env.a.data_ptr() + 2), ARG, "misaligned"),
        (dict(out=env.x.data_ptr()), ARG, "aliases"), (dict(out=env.x.data_ptr() + x_bytes - 1), ARG, "aliases"),
        (dict(info=env.x.data_ptr() + 8), ARG, "aliases"), (dict(info=env.out.data_ptr() + 4), ARG, "aliases"),
        (dict(rgba, out=env.a.data_ptr()), ARG, "aliases"), (dict(rgba, info=env.a.data_ptr() + 8), ARG, "aliases"),
    ]
    for changed, code, word in refused:
        rc, msg = env.png(**changed)
        assert rc == code and msg.startswith("mp_picture_png:") and word in msg, (changed, rc, msg)
    for changed, word in ((dict(n=-1), "n_pixels"), (dict(depth=None), "null"), (dict(out=None), "null"),
                          (dict(depth=env.a.data_ptr() + 1), "misaligned"), (dict(out=env.u16.data_ptr() + 1), "misaligned"),
                          (dict(out=env.a.data_ptr() + 6), "aliases"), (dict(lo=nan), "non-finite"),
                          (dict(scale=inf), "non-finite")):
        rc, msg = env.to_u16(**changed)
        assert rc == ARG and msg.startswith("mp_picture_u16:") and word in msg, (changed, rc, msg)
    for changed, word in ((dict(n=-1), "n_pixels"), (dict(image=None), "null"), (dict(alpha=None), "null"),
                          (dict(out=None), "null"), (dict(image=env.x.data_ptr() + 1), "misaligned"),
                          (dict(out=env.rgba.data_ptr() + 2), "misaligned"), (dict(out=env.x.data_ptr() + 8), "aliases"),
                          (dict(out=env.a.data_ptr()), "aliases"), (dict(bg=nan), "non-finite")):
        rc, msg = env.to_rgba(**changed)
        assert rc == ARG and msg.startswith("mp_picture_rgba8:") and word in msg, (changed, rc, msg)
    assert env.to_u16(n=2 ** 31)[0] == UNSUPPORTED and env.to_rgba(n=2 ** 31 // 4 + 1)[0] == UNSUPPORTED
    torch.cuda.synchronize()
    assert (env.out == SENTINEL).all() and (env.info == -7).all()  # nothing was launched
    assert (env.u16.view(torch.uint8) == SENTINEL).all() and (env.rgba == SENTINEL).all()
    assert env.to_u16(n=0)[0] == OK and env.to_rgba(n=0)[0] == OK
    # the context is still usable
    assert env.png()[0] == OK and env.to_u16()[0] == OK and env.to_rgba()[0] == OK
    torch.cuda.synchronize()
    info, out = env.info.cpu().numpy(), env.out.cpu().numpy()
    want = ref.encode(env.c.image, "rgb8")[0]
    for i in range(2):
        assert tuple(info[i]) == (len(want), 0) and out[i, :len(want)].tobytes() == want
    assert np.array_equal(env.u16.cpu().numpy(), ref.to_u16(np.stack([env.c.alpha] * 2), 0.0, 1.0).reshape(-1))
    assert np.array_equal(env.rgba.cpu().numpy(),
                          ref.to_rgba8(np.stack([env.c.image] * 2), np.stack([env.c.alpha] * 2)).reshape(-1, 4))


def test_wrapper_refusals(ops):
    x = torch.zeros((2, 8, 8, 3), device=DEV)
    a = torch.zeros((2, 8, 8), device=DEV)
    for bad in (dict(format="rgb16"), dict(filter="best"), dict(lo=np.nan), dict(scale=np.inf), dict(unmatte=0.5),
                dict(alpha=a), dict(format="rgba8"), dict(format="gray16"), dict(capacity=56),
                dict(out=torch.zeros((3, 4096), dtype=torch.uint8, device=DEV)),
                dict(info=torch.zeros((2, 2), dtype=torch.int64, device=DEV)),
                dict(format="rgba8", alpha=a[:1]), dict(format="rgba8", alpha=a.double()),
                dict(format="rgba8", alpha=a, unmatte=np.nan)):
        with pytest.raises(ValueError, match="picture_png_raw"):
            ops.picture_png_raw(x, **bad)
    for bad in (x[:, :, :, :2], x.double(), x[0], x[:, ::2]):
        with pytest.raises(ValueError, match="picture_png_raw"):
            ops.picture_png_raw(bad)
    with pytest.raises(ValueError, match="picture_u16_raw"):
        ops.picture_u16_raw(a.double())
    with pytest.raises(ValueError, match="picture_rgba8_raw"):
        ops.picture_rgba8_raw(x, a[:1])
