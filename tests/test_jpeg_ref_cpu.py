"""tests/jpeg_ref.py, the numpy restatement of mp_picture_jpeg (include/monoport_hip.h), held to its own formulas, to
the committed tables (tests/golden/jpeg_tables.npz), to its own entropy decoder and -- where Pillow with JPEG support is
importable -- to Pillow's tables, decoder and encoder; and the host-side surface of the feature (recon.Jpeg, the slots'
encode_pictures) on stand-ins.  No GPU."""
import inspect
import io
import os
import types

import numpy as np
import pytest

import jpeg_ref as ref

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_tables.npz")
SHAPES = [(1, 1), (8, 8), (17, 23), (40, 56), (61, 83), (160, 8)]
CONTENTS = ("smooth", "noise", "checker", "constant")
PSNR_MARGIN = 0.5  # dB below Pillow's own encoder


def content(kind, h, w, seed=1):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "smooth":
        img = np.stack([127 + 120 * np.sin(yy / 9.0 + xx / 13.0), 127 + 120 * np.cos(xx / 7.0),
                        127 + 100 * np.sin(yy / 5.0)], -1)
    elif kind == "noise":
        img = np.random.RandomState(seed).randint(0, 256, (h, w, 3))
    elif kind == "checker":
        img = np.repeat((((yy + xx) % 2) * 255)[..., None], 3, -1)
    else:
        img = np.full((h, w, 3), 255)
    return img.astype(np.uint8)


def pillow():
    """PIL.Image where Pillow can write and read JPEG, else None."""
    try:
        from PIL import Image, features
    except ImportError:
        return None
    return Image if features.check("jpg") else None


needs_pillow = pytest.mark.skipif(pillow() is None, reason="Pillow with JPEG support is not importable")


def segments(data):
    """(quantisation tables by id, Huffman tables by class << 4 | id) of a JPEG file."""
    i, dqt, dht = 2, {}, {}
    while True:
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        seg = data[i + 4:i + 2 + n]
        j = 0
        while m == 0xDB and j < len(seg):
            dqt[seg[j]] = list(seg[j + 1:j + 65])
            j += 65
        while m == 0xC4 and j < len(seg):
            counts = list(seg[j + 1:j + 17])
            dht[seg[j]] = (counts, list(seg[j + 17:j + 17 + sum(counts)]))
            j += 17 + sum(counts)
        if m == 0xDA:
            return dqt, dht
        i += 2 + n


# ---- tables ---------------------------------------------------------------------------------------------------------
def test_literals_equal_their_formulas():
    assert np.array_equal(ref.DCT, ref.dct_matrix())
    assert np.array_equal(ref.ZIGZAG, ref.zigzag_order()) and sorted(ref.ZIGZAG) == list(range(64))
    # the two passes stay inside int32 at the extreme block
    for block in (np.full((1, 8, 8), 255), np.zeros((1, 8, 8)), content("checker", 8, 8)[None, :, :, 0]):
        ref.fdct_quant(block, np.ones(64, dtype=np.int64))
    assert ref.fdct_quant(np.full((1, 8, 8), 255), np.ones(64, dtype=np.int64))[0, 0] == 1016
    assert ref.fdct_quant(np.zeros((1, 8, 8)), np.ones(64, dtype=np.int64))[0, 0] == -1024


def test_tables_equal_the_golden_file():
    g = np.load(GOLDEN)
    for q in (1, 10, 50, 75, 90, 100):
        luma, chroma = ref.quant_tables(q)
        assert np.array_equal(luma, g["quant_luma_q%d" % q]) and np.array_equal(chroma, g["quant_chroma_q%d" % q]), q
    for name, table in (("dc_luma", ref.DC_LUMA), ("ac_luma", ref.AC_LUMA), ("dc_chroma", ref.DC_CHROMA),
                        ("ac_chroma", ref.AC_CHROMA)):
        assert list(g[name + "_counts"]) == table[0] and list(g[name + "_symbols"]) == table[1], name
        codes = ref.huffman_codes(table)
        assert len(codes) == len(table[1]) == sum(table[0]) and max(n for _, n in codes.values()) <= 16
    # a lane of the block-coding kernel holds at most 3 ZRL + one code + 10 magnitude bits in one 64-bit word
    for table in (ref.AC_LUMA, ref.AC_CHROMA):
        codes = ref.huffman_codes(table)
        assert 3 * codes[0xF0][1] + max(n for _, n in codes.values()) + 10 <= 59


@needs_pillow
def test_tables_equal_what_pillow_writes():
    image = pillow().fromarray(content("noise", 16, 16))
    for q in (1, 10, 50, 75, 90, 100):
        buf = io.BytesIO()
        image.save(buf, "JPEG", quality=q, optimize=False, subsampling=2)
        dqt, dht = segments(buf.getvalue())
        luma, chroma = ref.quant_tables(q)
        assert dqt[0] == list(luma) and dqt[1] == list(chroma), q
        assert {tc: (t[0], t[1]) for tc, t in ref.HUFFMAN} == dht
    # and our own header carries them
    dqt, dht = segments(ref.encode(content("noise", 16, 16), 75, "420")[0])
    assert dqt[0] == list(ref.quant_tables(75)[0]) and dht[0x11] == ref.AC_CHROMA


# ---- round trip -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_decode_returns_the_quantised_coefficients(shape):
    h, w = shape
    for kind in CONTENTS:
        img = content(kind, h, w)
        for sub in ref.SUBSAMPLINGS:
            for q, restart in ((50, None), (90, 1), (100, 3), (1, 65535)):
                data, stats = ref.encode(img, q, sub, restart)
                coef, hh, ww, ss, rr = ref.decode(data)
                want, _ = ref.coefficients(img, q, sub)
                assert (hh, ww, ss) == (h, w, sub) and rr == ref.geometry(h, w, sub, restart)[4]
                assert np.array_equal(coef, want), (kind, sub, q, restart)
                assert len(data) <= ref.max_bytes(h, w, sub, restart)
                assert data.count(b"\xff\xda") >= 1 and stats["intervals"] == ref.geometry(h, w, sub, restart)[5]


def test_float_input_goes_through_step_1():
    x = np.array([[[-1.0, 0.0, 1.0], [2.0, np.nan, np.inf], [-np.inf, 0.5, 127.5 / 255]]], F)
    assert ref.to_u8(x).tolist() == [[[0, 0, 255], [255, 0, 255], [0, 128, 128]]]
    assert np.array_equal(ref.to_u8((np.arange(256) / 255.0).astype(F)), np.arange(256))
    assert ref.encode(x, 90, "444")[0] == ref.encode(ref.to_u8(x), 90, "444")[0]


# ---- Pillow ---------------------------------------------------------------------------------------------------------
def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / max(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2), 1e-12))


@needs_pillow
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_pillow_decodes_every_file_and_the_psnr_is_pillows(shape):
    """Pillow (libjpeg-turbo) decodes every file at the right size, and the PSNR against the source is no more than
    PSNR_MARGIN = 0.5 dB below that of Pillow's own encoder at the same quality and subsampling.  Measured gaps (ours -
    Pillow's, dB) over q in {50, 90, 100}, both subsamplings, smooth / noise / checker, with Pillow 12.2:
    1x1 0.00 everywhere; 8x8 -0.31 .. +0.37; 17x23 -0.21 .. +0.24; 40x56 -0.34 .. +0.22 (the lowest: smooth, 420,
    q 100); 61x83 -0.17 .. +0.28; 160x8 -0.23 .. +0.25.  File sizes are within a few percent of Pillow's (the restart
    markers and their padding), e.g. 61x83 noise 444 q 100: 23,514 against 23,453 bytes."""
    image_mod = pillow()
    h, w = shape
    for kind in ("smooth", "noise", "checker"):
        img = content(kind, h, w)
        for sub, code in (("444", 0), ("420", 2)):
            for q in (50, 90, 100):
                data, _ = ref.encode(img, q, sub)
                ours = np.array(image_mod.open(io.BytesIO(data)).convert("RGB"))
                assert ours.shape == img.shape
                buf = io.BytesIO()
                image_mod.fromarray(img).save(buf, "JPEG", quality=q, subsampling=code)
                theirs = np.array(image_mod.open(io.BytesIO(buf.getvalue())).convert("RGB"))
                gap = psnr(ours, img) - psnr(theirs, img)
                print("%dx%d %s %s q%d: %d / %d bytes, gap %+.2f dB" % (h, w, kind, sub, q, len(data),
                                                                        len(buf.getvalue()), gap))
                assert gap >= -PSNR_MARGIN, (kind, sub, q, gap)
    for restart in (1, 3, 65535):  # and with other restart intervals
        data, _ = ref.encode(content("noise", h, w), 90, "420", restart)
        assert np.array(image_mod.open(io.BytesIO(data)).convert("RGB")).shape == (h, w, 3)


# ---- edge cases, asserted through stats -------------------------------------------------------------------------------
def test_every_edge_case_is_reached():
    _, s = ref.encode(content("smooth", 61, 83), 100, "444")
    assert s["zrl"] > 0
    _, s = ref.encode(content("checker", 3, 5), 100, "444")
    assert s["stuffed"] > 0
    _, s = ref.encode(content("constant", 8, 8), 100, "444")
    assert s["dc_category"] >= 10
    half = np.zeros((8, 8, 3), np.uint8)
    half[:, 4:] = 255
    _, s = ref.encode(half, 100, "444")
    assert s["ac_category"] == 10
    data, s = ref.encode(content("noise", 64, 64), 100, "444")
    assert s["no_eob"] and len(data) > 64 * 64 * 3  # a file larger than its raw bytes: raw size is no safe capacity
    data, s = ref.encode(content("noise", 160, 8), 90, "444")
    assert s["intervals"] == 20 > 8
    assert [data.count(bytes([0xFF, 0xD0 + m])) >= 1 for m in range(8)] == [True] * 8  # the marker number wraps
    assert s["block_bits"] <= ref.BLOCK_MAX_BITS


def test_the_worst_block_fits_its_slot():
    """Every AC coefficient at category 10 behind the longest code, the DC at category 11: 1660 bits at most."""
    for dc, ac in ((ref.DC_LUMA, ref.AC_LUMA), (ref.DC_CHROMA, ref.AC_CHROMA)):
        dcc, acc = ref.huffman_codes(dc), ref.huffman_codes(ac)
        worst = max(n for _, n in dcc.values()) + 11 + 63 * (max(n for _, n in acc.values()) + 10)
        assert worst <= ref.BLOCK_MAX_BITS <= 26 * 64
    assert ref.max_bytes(8, 8, "444") == ref.HEADER_BYTES + 416 * 3 + 2
    assert ref.max_bytes(4096, 4096, "444", 1) < 2 ** 31


# ---- the host-side surface --------------------------------------------------------------------------------------------
def test_jpeg_options_are_validated():
    from monoport_amd import recon
    j = recon.Jpeg()
    assert (j.quality, j.subsampling, j.restart, j.capacity) == (90, "420", None, None)
    j = recon.Jpeg(quality=1, subsampling="444", restart=65535, capacity=629)
    assert (j.quality, j.subsampling, j.restart, j.capacity_for(1024, 1024)) == (1, "444", 65535, 629)
    assert recon.Jpeg().capacity_for(1024, 1024) == 4096 + 1024 * 1024 * 3 // 4
    assert recon.Jpeg().capacity_for(1, 1) == ref.max_bytes(1, 1, "420")  # never more than the provable bound
    for bad in (dict(quality=0), dict(quality=101), dict(quality=90.5), dict(quality=True), dict(quality=None),
                dict(subsampling="422"), dict(subsampling=None), dict(subsampling=2), dict(restart=0),
                dict(restart=65536), dict(restart=1.0), dict(restart=True), dict(capacity=628), dict(capacity=-1),
                dict(capacity=1e6), dict(capacity=2 ** 31 + 1)):
        with pytest.raises(ValueError, match="Jpeg"):
            recon.Jpeg(**bad)
    with pytest.raises(ValueError, match="recon.Jpeg"):
        recon.encode_jpeg(None, jpeg={"quality": 90})
    with pytest.raises(ValueError, match="shade=None"):
        recon.encode_jpeg(recon.MeshRender(None, None, None))
    with pytest.raises(ValueError, match="float32"):
        recon.encode_jpeg(np.zeros((4, 4, 3), F))


def test_max_bytes_needs_no_device():
    from monoport_amd import ops
    for (h, w), sub, restart in (((1, 1), "444", None), ((61, 83), "420", 3), ((4096, 4096), "444", 1)):
        assert ops.jpeg_max_bytes(h, w, sub, restart) == ref.max_bytes(h, w, sub, restart)
    for bad in ((0, 8), (8, 4097), (8.0, 8)):
        with pytest.raises(ValueError, match="jpeg_max_bytes"):
            ops.jpeg_max_bytes(*bad)


def test_encode_pictures_refusals_and_the_pins_hold():
    from monoport_amd import pipeline, recon
    # the pins of the existing tests: the new surface is a method, not a constructor keyword or a picture key
    assert list(inspect.signature(pipeline.FrameSlot.__init__).parameters)[-1] == "lighting"
    assert pipeline.PICTURE_KEYS == ("views", "res", "shade", "projection", "nearest", "near", "perspective_correct",
                                     "background", "scene", "composite")
    assert pipeline.PictureOptions._fields == pipeline.PICTURE_KEYS
    for cls in (pipeline.ViewsSlot, pipeline.ColorViewsSlot):
        assert cls.encode_pictures is pipeline.FrameSlot.encode_pictures and cls.jpegs is pipeline.FrameSlot.jpegs
    # stand-in slots: no device is touched before the refusals
    def slot(**k):
        s = object.__new__(pipeline.FrameSlot)
        s.picture_options = None
        s.__dict__.update(k)
        return s
    assert slot().jpeg is None
    with pytest.raises(ValueError, match="recon.Jpeg"):
        slot().encode_pictures({"quality": 90})
    with pytest.raises(ValueError, match="without pictures"):
        slot().encode_pictures(recon.Jpeg())
    with pytest.raises(ValueError, match="shade=None"):
        slot(picture_options=types.SimpleNamespace(shade=None, views=1, res=(8, 8))).encode_pictures(recon.Jpeg())
    with pytest.raises(RuntimeError, match="before the first"):
        slot(picture_options=types.SimpleNamespace(shade="normals", views=1, res=(8, 8)),
             _chained=True).encode_pictures(recon.Jpeg())
    with pytest.raises(RuntimeError, match="encode_pictures"):
        slot().jpegs()
    # the pipeline forwards to every slot
    calls = []
    pipe = object.__new__(pipeline.FramePipeline)
    pipe.slots = [types.SimpleNamespace(encode_pictures=calls.append) for _ in range(3)]
    j = recon.Jpeg(quality=50)
    pipe.encode_pictures(j)
    assert calls == [j, j, j]
