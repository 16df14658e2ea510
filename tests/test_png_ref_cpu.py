"""tests/png_ref.py, the numpy restatement of mp_picture_png (include/monoport_hip.h), judged by outsiders: zlib inflates
every stream to the filtered bytes, Pillow reads every file back to exactly the samples, zlib's CRC-32 and Adler-32 agree
with every chunk and trailer; the derivable size conditions; the size against Pillow's own encoder on a rendered, lit
picture; and the host-side surface of the feature (recon.Png, encode_png, the slots' encode_pictures) on stand-ins.
No GPU."""
import inspect
import io
import struct
import types
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases as cases
import png_ref as ref

F = np.float32
MODES = {"rgb8": "RGB", "rgba8": "RGBA", "gray16": "I;16"}
# File sizes of the restatement over Pillow's compress_level=6 file of the same samples, measured once on the lit
# sphere below (the definition is deterministic: the 5 % only absorb another Pillow / zlib)
SPHERE_RATIO = {"rgb8": 1.0471, "rgba8": 1.1438}  # 8513 / 8130 and 9974 / 8720 bytes


def idat(file):
    return b"".join(data for kind, data, _ in ref.chunks_of(file) if kind == b"IDAT")


def check_file(file, samples, filt):
    """Everything an outsider can say about one file."""
    fmt = ref.format_of(samples)
    h, w = samples.shape[:2]
    bpp, depth, colour = ref.FORMATS[fmt]
    chunks = ref.chunks_of(file)
    assert [k for k, _, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (len(chunks) - 2) + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 0)
    assert all(len(d) == ref.IDAT for _, d, _ in chunks[1:-2]) and 1 <= len(chunks[-2][1]) <= ref.IDAT
    for kind, data, crc in chunks:
        assert crc == zlib.crc32(kind + data)
    z = idat(file)
    stream = ref.filtered_stream(samples, filt).tobytes()
    assert zlib.decompress(z) == stream
    assert z[:2] == b"\x78\x01" and struct.unpack(">I", z[-4:])[0] == zlib.adler32(stream)
    rows, _ = ref.rows_of(samples)
    assert np.array_equal(ref.unfilter(stream, h, w, bpp), rows)
    picture = Image.open(io.BytesIO(file))
    picture.load()
    assert picture.mode == MODES[fmt] and picture.size == (w, h)
    assert np.array_equal(np.asarray(picture).astype(samples.dtype), samples)
    assert len(file) <= ref.max_bytes(h, w, fmt)


@pytest.mark.parametrize("filt", ref.FILTERS)
@pytest.mark.parametrize("fmt", sorted(ref.FORMATS))
def test_zlib_and_pillow_read_every_file_back_exactly(fmt, filt):
    for c in cases.small_cases(fmt):
        check_file(cases.restated(c, filt), cases.samples(c), filt)


def test_the_cases_exercise_what_they_are_for():
    def parse(c, filt="none"):
        x = ref.filtered_stream(cases.samples(c), filt).astype(np.int64)
        w = c.image.shape[1]
        best, dist = ref.matches(x, ref.candidates(w, ref.FORMATS[c.format][0]))
        return x, best, dist
    # no match at all: HDIST = 1 with a code of length zero, which zlib accepted above
    x, best, dist = parse(cases.no_match())
    assert best.max() == 0
    # the Fibonacci block: no match, 17 leaves, an unlimited tree deeper than 15, the limited one within it
    x, best, dist = parse(cases.fibonacci())
    assert len(x) <= ref.BLOCK and best.max() == 0
    hist = ref.block_tokens(x, 0, len(x), best, dist)[5]
    assert max(ref.huffman_lengths(hist, 99)) == 16 and max(ref.huffman_lengths(hist, 15)) <= 15
    # a constant picture: one distance symbol in a block (length 1), runs of 258 and runs cut by the block's end
    x, best, dist = parse(cases.constant("rgb8", 1, 2000))
    _, mlen, _, _, _, _, d_hist = ref.block_tokens(x, 0, ref.BLOCK, best, dist)
    assert (d_hist > 0).sum() == 1 and mlen.max() == 258 and (best[ref.BLOCK - 200:ref.BLOCK] < 258).all()
    # the zlib stream ends one byte before, on and one byte behind an IDAT boundary
    for delta in (-1, 0, 1):
        z = idat(cases.restated(cases.idat_edge(delta), "none"))
        assert len(z) == ref.IDAT + delta
    # strides below, on and above the block
    assert [1 + 3 * w for w in cases.EDGE_WIDTHS["rgb8"]] == [4093, 4096, 4099]
    assert [1 + 4 * w for w in cases.EDGE_WIDTHS["rgba8"]] == [4093, 4097]
    assert [1 + 2 * w for w in cases.EDGE_WIDTHS["gray16"]] == [4095, 4097]


def test_samples_of_special_values():
    v = np.asarray([np.nan, np.inf, -np.inf, -1, 2, 0, 1, 0.5], F)
    assert ref.to_u16(v, 0.0, 1.0).tolist() == [0, 65535, 0, 0, 65535, 0, 65535, 32768]
    hi = np.nextafter(F(1), F(2))
    assert ref.to_u16(np.asarray([1.0, hi], F), 1.0, float(F(1) / (hi - F(1)))).tolist() == [0, 65535]
    image = np.asarray([[0.5, 0.5, 0.5]] * 5, F)
    alpha = np.asarray([0.0, np.nan, -1.0, 1.0, 0.5], F)
    got = ref.to_rgba8(image, alpha, unmatte=1.0)
    assert got[:3].tolist() == [[0, 0, 0, 0]] * 3 and got[3].tolist() == [128, 128, 128, 255]
    assert got[4].tolist() == [0, 0, 0, 128]            # (0.5 - 0.5 * 1) / 0.5
    assert ref.to_rgba8(image, alpha)[:, :3].tolist() == [[128, 128, 128]] * 5  # without unmatte: the colour of RGB8
    assert ref.to_rgba8(image, alpha)[:, 3].tolist() == [0, 0, 0, 255, 128]


@pytest.mark.parametrize("fmt", sorted(ref.FORMATS))
def test_derivable_sizes(fmt):
    """A constant 256 x 256 picture: a match of 258 bytes costs at most 30 bits, a block header at most 288 bytes, so
    the file is below a fiftieth of the samples.  Noise stays within max_bytes."""
    bpp = ref.FORMATS[fmt][0]
    for filt in ("adaptive", "none"):
        assert len(cases.restated(cases.constant(fmt, 256, 256), filt)) <= 256 * 256 * bpp // 50
    c = cases.noise(fmt, 64, 64, 4)
    for filt in ref.FILTERS:
        assert len(cases.restated(c, filt)) <= ref.max_bytes(64, 64, fmt)
    assert ref.max_bytes(4096, 4096, "rgba8") < 2 ** 31


def test_huffman_rule_and_run_lengths():
    assert ref.huffman_lengths([0, 0, 0], 15) == [0, 0, 0] and ref.huffman_lengths([0, 7, 0], 15) == [0, 1, 0]
    assert ref.huffman_lengths([1, 1, 1, 1], 15) == [2, 2, 2, 2]
    assert ref.huffman_lengths([1, 1, 2], 15) == [2, 2, 1]      # the leaf 2 goes before the joined 2
    fib = [1, 1, 1, 3, 4, 7, 11, 18, 29, 47]
    assert max(ref.huffman_lengths(fib, 99)) == 9 and max(ref.huffman_lengths(fib, 7)) <= 7
    for lens in (ref.huffman_lengths(fib, 7), ref.huffman_lengths(list(range(1, 287)), 15)):
        assert sum(2.0 ** -v for v in lens if v) == 1.0          # a complete code
    assert ref.run_lengths([0] * 150 + [5] * 9 + [0] * 4 + [3, 3] + [0] * 2) == [
        (18, 7, 127), (18, 7, 1), (5, 0, 0), (16, 2, 3), (5, 0, 0), (5, 0, 0), (17, 3, 1), (3, 0, 0), (3, 0, 0), (0, 0, 0),
        (0, 0, 0)]


@pytest.fixture(scope="module")
def lit_sphere():
    """The 65^3 sphere, rendered at 129^2 by the rasteriser's restatement and lit by the lighting's: (image, alpha)."""
    import light_ref
    import mesh_render_ref
    import shadow_cases
    from monoport_amd import mesh_util
    verts, faces = shadow_cases.sphere_mesh()
    normals = np.ascontiguousarray(mesh_util.compute_normal(verts, faces, "accumulate"), F)
    r = mesh_render_ref.render(verts, faces, 129, 129, attr=normals, nearest="max")
    sh = np.random.RandomState(0).uniform(-0.2, 0.6, (9, 3)).astype(F)
    sh[0] = 0.8
    image, _ = light_ref.light(r.image, r.face, None, sh, np.asarray([0.3, -0.5, -0.8], F), np.asarray([0.6, 0.5, 0.4], F),
                               albedo_rgb=(0.9, 0.8, 0.7), background=1.0)
    return image.reshape(129, 129, 3), (r.face >= 0).astype(F)


@pytest.mark.parametrize("fmt", ["rgb8", "rgba8"])
def test_size_against_pillow_on_a_lit_sphere(lit_sphere, fmt):
    image, alpha = lit_sphere
    samples = ref.samples_of(image, fmt, alpha, 1.0 if fmt == "rgba8" else None)
    mine = ref.encode_samples(samples)
    check_file(mine, samples, "adaptive")
    buf = io.BytesIO()
    Image.fromarray(samples).save(buf, "PNG", compress_level=6)
    ratio = len(mine) / len(buf.getvalue())
    print("png size over Pillow's, %s: %d / %d = %.4f" % (fmt, len(mine), len(buf.getvalue()), ratio))
    assert ratio <= SPHERE_RATIO[fmt] * 1.05


# ---- the host-side surface --------------------------------------------------------------------------------------------
def test_png_options_are_validated():
    import torch
    from monoport_amd import ops, recon
    p = recon.Png()
    assert (p.filter, p.alpha, p.unmatte, p.plane, p.depth_range, p.capacity, p.format) == (
        "adaptive", None, None, "image", None, None, "rgb8")
    p = recon.Png(filter="paeth", alpha="coverage", unmatte=1, capacity=57)
    assert (p.filter, p.format, p.unmatte, p.capacity_for(1024, 1024)) == ("paeth", "rgba8", 1.0, 57)
    p = recon.Png(plane="depth", depth_range=(-1, 1))
    assert (p.format, p.lo, p.scale, p.depth_range) == ("gray16", -1.0, 0.5, (-1.0, 1.0))
    assert recon.Png().capacity_for(1024, 1024) == 4096 + 1024 * 1024 * 3 // 2
    assert recon.Png(alpha="subject").capacity_for(100, 100) == 4096 + 100 * 100 * 4 // 2
    assert recon.Png().capacity_for(1, 1) == ref.max_bytes(1, 1, "rgb8")  # never more than the provable bound
    for bad in (dict(filter="best"), dict(filter=None), dict(filter=6), dict(alpha="mask"), dict(alpha=True),
                dict(unmatte=1.0), dict(alpha="coverage", unmatte=np.nan), dict(alpha="coverage", unmatte="white"),
                dict(plane="normal"), dict(plane="depth"), dict(plane="depth", depth_range=(1, 1)),
                dict(plane="depth", depth_range=(0, np.inf)), dict(plane="depth", depth_range=(2, 1)),
                dict(plane="depth", depth_range=(0, 1), alpha="subject"), dict(depth_range=(0, 1)),
                dict(capacity=56), dict(capacity=1e6), dict(capacity=True), dict(capacity=2 ** 31 + 1)):
        with pytest.raises(ValueError, match="Png"):
            recon.Png(**bad)
    with pytest.raises(ValueError, match="recon.Png"):
        recon.encode_png(None, png={"filter": "none"})
    with pytest.raises(ValueError, match="shade=None"):
        recon.encode_png(recon.MeshRender(None, None, None))
    with pytest.raises(ValueError, match="float32"):
        recon.encode_png(np.zeros((4, 4, 3), F))
    with pytest.raises(ValueError, match="ResolvedPicture"):
        recon.encode_png(recon.MeshRender(torch.zeros(4, 4, 3), torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32)),
                         recon.Png(alpha="coverage"))
    with pytest.raises(ValueError, match="alpha keyword"):
        recon.encode_png(torch.zeros(4, 4, 3), recon.Png(alpha="subject"))
    with pytest.raises(ValueError, match="alpha keyword"):
        recon.encode_png(torch.zeros(4, 4, 3), recon.Png(), alpha=torch.zeros(4, 4))
    for (h, w), fmt in (((1, 1), "rgb8"), ((61, 83), "rgba8"), ((4096, 4096), "gray16")):
        assert ops.png_max_bytes(h, w, fmt) == ref.max_bytes(h, w, fmt)
    for bad in ((0, 8), (8, 4097), (8.0, 8), (8, 8, "rgb16")):
        with pytest.raises(ValueError, match="png_max_bytes"):
            ops.png_max_bytes(*bad)


def test_encode_pictures_takes_a_png_and_the_pins_hold():
    from monoport_amd import pipeline, recon
    # the pins of the existing tests: the new surface is a method, not a constructor keyword or a picture key
    assert list(inspect.signature(pipeline.FrameSlot.__init__).parameters)[-1] == "lighting"
    assert pipeline.PICTURE_KEYS == ("views", "res", "shade", "projection", "nearest", "near", "perspective_correct",
                                     "background", "scene", "composite")
    for cls in (pipeline.ViewsSlot, pipeline.ColorViewsSlot):
        assert cls.encode_pictures is pipeline.FrameSlot.encode_pictures and cls.pngs is pipeline.FrameSlot.pngs

    def slot(**k):
        s = object.__new__(pipeline.FrameSlot)
        s.picture_options = None
        s.__dict__.update(k)
        return s

    def options(**k):
        return types.SimpleNamespace(**dict(dict(shade="normals", views=1, res=(8, 8), samples=1), **k))
    assert slot().jpeg is None and slot().png is None
    with pytest.raises(ValueError, match="recon.Jpeg"):
        slot().encode_pictures({"filter": "none"})
    with pytest.raises(ValueError, match="without pictures"):
        slot().encode_pictures(recon.Png())
    with pytest.raises(ValueError, match="shade=None"):
        slot(picture_options=options(shade=None)).encode_pictures(recon.Png())
    with pytest.raises(ValueError, match="samples > 1"):
        slot(picture_options=options()).encode_pictures(recon.Png(alpha="coverage"))
    with pytest.raises(RuntimeError, match="before the first"):
        slot(picture_options=options(), _chained=True).encode_pictures(recon.Png())
    with pytest.raises(RuntimeError, match="before the first"):  # the depth needs no shade
        slot(picture_options=options(shade=None), _chained=True).encode_pictures(
            recon.Png(plane="depth", depth_range=(0, 1)))
    with pytest.raises(RuntimeError, match="encode_pictures"):
        slot().pngs()
    calls = []
    pipe = object.__new__(pipeline.FramePipeline)
    pipe.slots = [types.SimpleNamespace(encode_pictures=calls.append) for _ in range(3)]
    p = recon.Png()
    pipe.encode_pictures(p)
    assert calls == [p, p, p]
